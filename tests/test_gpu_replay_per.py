"""Prioritised replay (finrl_amd.PrioritizedReplayBuffer, finenv_replay_per_* in include/finenv.h) on
the MI355X, against the NumPy restatement in tests/replay_per_model.py.  Tickets and sums are
integers and every batch output is a copy, so every comparison but the importance weights is exact."""
import ctypes as C

import numpy as np
import pytest

import replay_model as rm
import replay_nstep_model as nm
import replay_per_model as pm
from replay_cases import (POISON, RING_SEED, assert_batch, crypto_env, host_ring, need_gpu, outs, per_ring,
                          random_tickets, set_head, set_tickets)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# leaf counts at the edges of the fan-out: 15; 64, exactly one node; 65; 350; 4617, three levels,
# ragged at both
SHAPES = [(3, 5), (4, 16), (5, 13), (5, 70), (9, 513)]
TOP = pm.TOP


def _buffer(S, E, **kw):
    from finrl_amd import PrioritizedReplayBuffer
    return PrioritizedReplayBuffer(S, E, 5, 1, obs_pitch="packed", **kw)


def _tickets(buf):
    return buf.tickets.cpu().numpy().view(np.uint32)


def _tree(buf):
    return buf.tree.cpu().numpy().view(np.uint64)


def _max(buf):
    return int(buf.max_ticket.item()) & 0xFFFFFFFF


def _u_tensor(values):
    return torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).cuda()


def _assert_state(buf, t, tag, top=None):
    np.testing.assert_array_equal(_tickets(buf), t, err_msg=f"tickets {tag}")
    np.testing.assert_array_equal(_tree(buf), pm.build_tree(t), err_msg=f"tree {tag}")
    assert buf.total == pm.total(t), tag
    if top is not None:
        assert _max(buf) == top, tag


# ------------------------------------------------------------------------------------------------
# 1. rebuild and find
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,E,full", [(S, E, False) for S, E in SHAPES] + [(9, 513, True), (5, 13, True)])
def test_rebuild_and_find_equal_model(S, E, full):
    """The tree read back is the model's word for word (all leaves at 2^32 - 1: the sums pass 32
    bits), and find on both sides of every prefix-sum boundary, at total - 1, total and 2^64 - 1 is
    searchsorted's leaf: never a leaf at 0."""
    need_gpu()
    buf = _buffer(S, E)
    assert buf.tree.numel() == pm.tree_words(S * E) and buf.total == 0
    assert buf.find(_u_tensor([0, 7])).cpu().numpy().tolist() == [[0, 0], [0, 0]]     # total 0: pair (0, 0)
    t = np.full((S, E), TOP, np.uint32) if full else random_tickets(S, E, S * E)
    set_tickets(buf, t)
    _assert_state(buf, t, f"S={S} E={E}")
    flat = t.reshape(-1)
    c = np.cumsum(flat.astype(np.uint64), dtype=np.uint64)
    tot = int(c[-1])
    assert not full or tot > 2 ** 32
    u = sorted({int(x) - 1 for x in c if x > 0} | {int(x) for x in c} | {0, tot - 1, tot, 2 ** 64 - 1})
    want = pm.find_leaves(flat, u)
    assert (flat[want] != 0).all()
    got = buf.find(_u_tensor(u)).cpu().numpy()
    np.testing.assert_array_equal(got, pm.pairs_of(want, E))


# ------------------------------------------------------------------------------------------------
# 2. the fill rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,E", SHAPES)
def test_put_equals_model(S, E):
    """finenv_replay_per_put at every pos (the wrap S-1 -> 0 included: two separate runs of level-1
    nodes; neighbours: runs that share a node), pos_next == pos (nothing zeroed), a far pos_next, and
    max_ticket 0 taken as 1."""
    need_gpu()
    from finrl_amd import _native as nat
    buf = _buffer(S, E)
    t = random_tickets(S, E, 7 * S + E)
    set_tickets(buf, t)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    moves = [(p, (p + 1) % S) for p in range(S)] + [(1, 1), (0, 2), (S - 1, S - 1)]
    for n, (pos, nxt) in enumerate(moves):
        top = (0, 1, TOP, 77777)[n % 4]
        buf.max_ticket.fill_(top - 2 ** 32 if top >= 2 ** 31 else top)
        assert nat.lib().finenv_replay_per_put(C.byref(buf._per), S, E, pos, nxt, stream) == 0
        t = pm.put(t, top, pos, nxt)
        _assert_state(buf, t, f"put {pos} -> {nxt}")


def test_step_fills_tickets():
    """3 S steps of a real env: after each, the nonzero slots are exactly the valid ones, all their
    leaves hold max_ticket (raised once on the way by an update), and the tree is the model's."""
    need_gpu()
    from finrl_amd import PrioritizedReplayBuffer
    E, S = 70, 4
    env = crypto_env(E)
    D, A = env.obs.shape[1], env.action_dim
    buf = PrioritizedReplayBuffer(S, E, D, A, obs_pitch="packed", seed=3, frac_bits=10)
    assert _max(buf) == 1 << 10
    with pytest.raises(ValueError):
        buf.sample(4)
    rng = np.random.default_rng(7)
    buf.start(env, env.reset())
    t, top = np.zeros((S, E), np.uint32), 1 << 10
    for n in range(1, 3 * S + 1):
        a = torch.from_numpy(rng.uniform(-1, 1, (E, A)).astype(np.float32)).cuda()
        pos = buf.pos
        buf.step(env, a)
        t = pm.put(t, top, pos, buf.pos)
        _assert_state(buf, t, f"step {n}", top)
        pos, n_valid = rm.head_after(n, S)
        assert buf.head.tolist() == [pos, n_valid]
        live = sorted(rm.valid_slots(pos, n_valid, S))
        assert [s for s in range(S) if t[s].any()] == live
        if n < S + 2:
            assert (t[live] == top).all()
        if n == S + 1:                                   # a large TD error: later steps enter at it
            idx = torch.tensor([[live[0]], [5]], dtype=torch.int32)
            buf.update_priorities(idx, torch.tensor([3.0]), shaped=True)
            t, top = pm.update(t, top, idx.numpy(), np.array([3.0], np.float32), 10)
            assert top == 3 << 10
            _assert_state(buf, t, "after the update", top)
    assert t.max() == 3 << 10 and (t[(buf.pos - 1) % S] == 3 << 10).all()


# ------------------------------------------------------------------------------------------------
# 3. the write-back
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,E", SHAPES)
def test_update_priorities_equals_model(S, E):
    need_gpu()
    F = 16
    buf = _buffer(S, E, frac_bits=F)
    rng = np.random.default_rng(S + E)
    t = random_tickets(S, E, 3 * S + E)
    set_tickets(buf, t)
    top = _max(buf)
    assert top == 1 << F
    N = S * E
    # distinct indices, zero leaves among them (dropped), small weights: max_ticket stays
    leaves = rng.permutation(N)[:max(N // 2, 4)]
    pairs = pm.pairs_of(leaves, E)
    w = rng.uniform(0.001, 0.9, leaves.size).astype(np.float32)
    assert (t.reshape(-1)[leaves] == 0).any() and (t.reshape(-1)[leaves] != 0).any()
    buf.update_priorities(torch.from_numpy(pairs), torch.from_numpy(w), shaped=True)
    t2, top = pm.update(t, top, pairs, w, F)
    assert top == 1 << F and (t2.reshape(-1)[leaves][t.reshape(-1)[leaves] == 0] == 0).all()
    _assert_state(buf, t2, "distinct", top)
    # an entry aimed at a zero leaf is dropped, yet raises max_ticket
    corners = (E - 1, (S - 1) * E)
    live = np.array([k for k in np.flatnonzero(t2.reshape(-1)) if k not in corners])
    dead = np.flatnonzero(t2.reshape(-1) == 0)
    buf.update_priorities(torch.from_numpy(pm.pairs_of(dead[:1], E)), torch.tensor([40000.0]), shaped=True)
    top = 40000 << 16
    _assert_state(buf, t2, "dropped", top)
    # duplicates with equal values, the specials, and unclamped indices -> (0, E-1), (S-1, 0)
    pick = np.concatenate([live[:5], live[:5], live[:2]])
    w = np.concatenate([[np.nan, 0.0, -2.5, np.inf, 1e-9], [np.nan, 0.0, -2.5, np.inf, 1e-9],
                        [np.nan, 0.0]]).astype(np.float32)
    pairs = pm.pairs_of(pick, E)
    pairs = np.concatenate([pairs, [[-3, S + 4], [E + 9, -1]]], axis=1).astype(np.int32)
    w = np.concatenate([w, np.float32([2.5, 2.5])])
    want_last = pm.ticket(np.float32(2.5), F)
    buf.update_priorities(torch.from_numpy(pairs), torch.from_numpy(w), shaped=True)
    t3, top = pm.update(t2, top, pairs, w, F)
    assert top == TOP                                            # the ticket of +inf
    for s, e in ((0, E - 1), (S - 1, 0)):
        assert t3[s, e] == (want_last if t2[s, e] else 0)
    assert [int(t3.reshape(-1)[k]) for k in live[2:5]] == [1, TOP, 1]
    _assert_state(buf, t3, "duplicates and specials", top)
    # duplicates with unequal values: one of the candidates; the tree follows the leaves read back
    k = int(live[0])
    pairs = pm.pairs_of([k] * 64 + [int(live[1])], E)
    w = np.concatenate([np.arange(1, 65) * 0.25, [0.5]]).astype(np.float32)
    buf.update_priorities(torch.from_numpy(pairs), torch.from_numpy(w), shaped=True)
    got = _tickets(buf)
    assert int(got.reshape(-1)[k]) in set(pm.ticket(w[:64], F).tolist())
    t4 = t3.copy()
    t4.reshape(-1)[k] = got.reshape(-1)[k]
    t4.reshape(-1)[int(live[1])] = pm.ticket(np.float32(0.5), F)
    _assert_state(buf, t4, "unequal duplicates", top)
    # shaped=False: the model is fed torch's own (|p| + eps) ** alpha
    p = torch.from_numpy(rng.normal(0, 3, live.size).astype(np.float32)).cuda()
    pairs = pm.pairs_of(live, E)
    buf.update_priorities(torch.from_numpy(pairs), p)
    w = ((p.abs() + buf.eps) ** buf.alpha).cpu().numpy()
    t5, top = pm.update(t4, top, pairs, w, F)
    _assert_state(buf, t5, "shaped=False", top)


# ------------------------------------------------------------------------------------------------
# 4. the fused draw
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 0x123456789ABCDEF])
@pytest.mark.parametrize("D,P,A", [(5, 16, 1), (13, 13, 3), (51, 51, 10), (301, 304, 30)])
def test_sample_equals_model(D, P, A, seed):
    """Every lane-group width (4, 8, 32, 64) and both row paths, one-step and n = 3: the pairs are the
    model's draw, the batch is the look-up of those pairs, the probabilities are q / total exactly,
    the draw word advances, and poisoned caller outputs keep their pad columns."""
    need_gpu()
    S, E, B, n, gamma = 5, 70, 257, 3, 0.9
    buf, host = per_ring(S, E, D, P, A, seed=seed, ring_seed=RING_SEED)
    pos = 1
    set_head(buf, pos, S - 1)
    t = random_tickets(S, E, D)
    t[pos] = 0
    set_tickets(buf, t)
    draws = 0
    for rep in range(2):
        want_idx, want_p = pm.draw_pairs(seed, draws, B, t, E)
        assert pos not in set(want_idx[0].tolist())
        smp = buf.sample(B)
        tag = f"sample draw={draws}"
        np.testing.assert_array_equal(buf.last_indices.cpu().numpy(), want_idx, err_msg=tag)
        assert_batch(smp, rm.lookup(*host, want_idx) + (want_p[:, None],), tag)
        assert type(smp).__name__ == "PrioritizedReplayBufferSamples" and smp.probabilities.shape == (B, 1)
        assert_batch(buf.gather(buf.last_indices), rm.lookup(*host, want_idx), "gather(last_indices)")
        draws += 1
        assert int(buf.draw.item()) == draws == buf.draws
        want_idx, want_p = pm.draw_pairs(seed, draws, B, t, E)
        smp = buf.sample_nstep(B, n, gamma)
        tag = f"sample_nstep draw={draws}"
        np.testing.assert_array_equal(buf.last_indices.cpu().numpy(), want_idx, err_msg=tag)
        want = nm.nstep_lookup(*host, want_idx, pos, n, gamma)
        assert_batch(smp, want[:6] + (want_p[:, None],), tag)
        np.testing.assert_array_equal(buf.last_steps.cpu().numpy(), want[6], err_msg=tag)
        assert type(smp).__name__ == "PrioritizedNStepReplayBufferSamples"
        draws += 1
    assert not np.array_equal(pm.draw_pairs(seed, 0, B, t, E)[0], pm.draw_pairs(seed, 2, B, t, E)[0])
    for kind in ("packed", "slice"):
        out, back = outs(B, D, A, kind, 6)
        want_idx, want_p = pm.draw_pairs(seed, draws, B, t, E)
        got = buf.sample(B, out=out)
        assert_batch(got, rm.lookup(*host, want_idx) + (want_p[:, None],), f"out={kind}")
        out7, back7 = outs(B, D, A, kind, 7)
        want_idx7, want_p7 = pm.draw_pairs(seed, draws + 1, B, t, E)
        got = buf.sample_nstep(B, n, gamma, out=out7)
        assert_batch(got, nm.nstep_lookup(*host, want_idx7, pos, n, gamma)[:6] + (want_p7[:, None],),
                      f"n-step out={kind}")
        draws += 2
        for b in back + back7:
            b = b.cpu().numpy()
            if kind == "packed":
                assert b[0] == POISON
            else:
                assert (b[:, :4] == POISON).all() and (b[:, 4 + D:] == POISON).all()
    with pytest.raises(ValueError):
        buf.sample_nstep(B, n, gamma, out=out)                   # seven tensors, not six


# ------------------------------------------------------------------------------------------------
# 5. an untrusted tree
# ------------------------------------------------------------------------------------------------
def test_corrupt_tree_words_do_not_leave_the_ring():
    """Root and inner words set to huge values and to 0 (the leaves untouched, all memory valid):
    whatever the descent then selects lies inside [0, S) x [0, E), and the batch is the look-up of
    the returned pairs."""
    need_gpu()
    S, E, D, A, B = 9, 513, 13, 3, 257
    buf, host = per_ring(S, E, D, D, A, seed=9)
    set_head(buf, 1, S - 1)
    t = random_tickets(S, E, 5)
    huge = 2 ** 64 - 1
    words = pm.tree_words(S * E)
    assert words == 76
    cases = [{0: huge}, {0: 0}, {0: huge, 1: huge, 2: huge}, {1: 0, 2: 0}, {2: huge}, {1: 0, 75: huge},
             {k: huge for k in range(words)}, {k: 0 for k in range(1, words)}, {0: 1, 1: 2 ** 63, 2: 2 ** 63},
             {k: 2 ** 63 + k for k in range(3, words)}]
    u = _u_tensor([0, 1, 2 ** 31, 2 ** 40, 2 ** 63, huge - 1, huge])
    for case in cases:
        set_tickets(buf, t)
        tree = pm.build_tree(t)
        for k, v in case.items():
            tree[k] = v
        buf.tree.copy_(torch.from_numpy(tree.view(np.int64)))
        for call in (lambda: buf.sample(B), lambda: buf.sample_nstep(B, 3, 0.9)):
            smp = call()
            idx = buf.last_indices.cpu().numpy()
            assert idx[0].min() >= 0 and idx[0].max() < S and idx[1].min() >= 0 and idx[1].max() < E, case
            np.testing.assert_array_equal(smp.observations.cpu().numpy(), host[0][idx[0], idx[1]])
        got = buf.find(u).cpu().numpy()
        assert got[0].min() >= 0 and got[0].max() < S and got[1].min() >= 0 and got[1].max() < E, case
        if case == {0: 0}:
            assert not got.any()                                 # total 0: pair (0, 0)


# ------------------------------------------------------------------------------------------------
# 6. inside a captured graph
# ------------------------------------------------------------------------------------------------
def test_captured_step_sample_update_follows_the_model():
    """step + sample + update_priorities captured once and replayed three times: each replay fills
    the captured slot again at the current max_ticket, draws with the device's draw word from the
    tickets as they are, and writes priorities back; pairs, probabilities, tickets, max_ticket and
    tree follow the model run forward."""
    need_gpu()
    from finrl_amd import PrioritizedReplayBuffer
    E, S, B, seed, F = 70, 8, 257, 5, 12
    env = crypto_env(E)
    D, A = env.obs.shape[1], env.action_dim
    buf = PrioritizedReplayBuffer(S, E, D, A, obs_pitch="packed", seed=seed, frac_bits=F)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    acts = [torch.rand(E, A, generator=gen, device="cuda") * 2 - 1 for _ in range(3)]

    def priorities():                   # a function of the pair and the draw word: duplicates agree
        idx = buf.last_indices.long()
        return ((idx[0] * E + idx[1] + buf.draw) % 7 + 1).float() * 0.75

    def model_w(pairs, draw):
        return (((pairs[0].astype(np.int64) * E + pairs[1] + draw) % 7 + 1) * 0.75).astype(np.float32)

    buf.start(env, env.reset())
    t, top = np.zeros((S, E), np.uint32), 1 << F
    for a in acts[:2]:
        pos = buf.pos
        buf.step(env, a)
        t = pm.put(t, top, pos, buf.pos)
    buf.sample(B)                                            # first calls outside the capture
    buf.update_priorities(buf.last_indices, priorities(), shaped=True)
    pairs, _ = pm.draw_pairs(seed, 0, B, t, E)
    t, top = pm.update(t, top, pairs, model_w(pairs, 1), F)
    torch.cuda.synchronize()
    _assert_state(buf, t, "before the capture", top)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pass
    pos = buf.pos
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.step(env, acts[2])
        smp = buf.sample(B)
        buf.update_priorities(buf.last_indices, priorities(), shaped=True)
    idx = buf.last_indices
    for rep in range(3):
        draw = int(buf.draw.item())
        g.replay()
        torch.cuda.synchronize()
        assert int(buf.draw.item()) == draw + 1
        t = pm.put(t, top, pos, (pos + 1) % S)
        pairs, prob = pm.draw_pairs(seed, draw, B, t, E)
        np.testing.assert_array_equal(idx.cpu().numpy(), pairs, err_msg=f"replay {rep}")
        assert_batch(smp, rm.lookup(*host_ring(buf), pairs) + (prob[:, None],), f"replay {rep}")
        t, top = pm.update(t, top, pairs, model_w(pairs, draw + 1), F)
        _assert_state(buf, t, f"replay {rep}", top)
    assert top == pm.ticket(np.float32(7 * 0.75), F)


# ------------------------------------------------------------------------------------------------
# 7. importance weights
# ------------------------------------------------------------------------------------------------
def test_importance_weights():
    """(n_valid E P)^-beta over its batch maximum against float64 NumPy; both sides of the comparison
    round a float32 pow, so this one is not exact."""
    need_gpu()
    S, E, B = 5, 70, 257
    buf = _buffer(S, E, seed=2)
    set_head(buf, 1, S - 1)
    t = random_tickets(S, E, 11)
    t[t == TOP] = 3                                          # a spread of probabilities, none dominant
    t[1] = 0
    set_tickets(buf, t)
    smp = buf.sample(B)
    p = smp.probabilities.cpu().numpy().astype(np.float64)
    for beta in (0.0, 0.4, 1.0):
        w = ((S - 1) * E * p) ** -beta
        got = buf.importance_weights(smp.probabilities, beta)
        assert got.shape == (B, 1) and got.dtype == torch.float32
        np.testing.assert_allclose(got.cpu().numpy(), w / w.max(), rtol=1e-6)
    buf.head.copy_(torch.tensor([1, 2], dtype=torch.int32))       # the device word, not the host mirror
    got = buf.importance_weights(smp.probabilities, 0.5)
    w = (2 * E * p) ** -0.5
    np.testing.assert_allclose(got.cpu().numpy(), w / w.max(), rtol=1e-6)
