"""The replay buffer's n-step sampler (ReplayBuffer.sample_nstep / .gather_nstep,
finenv_replay_sample_nstep / _gather_nstep in include/finenv.h) on the MI355X, against the NumPy
restatement in tests/replay_nstep_model.py.  Every output is a copy or the stated arithmetic (float32
powers of gamma, one float64 sum rounded once), so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import replay_model as rm
import replay_nstep_model as nm
from replay_cases import (POISON, RING_SEED, assert_batch, coded_ring, crypto_env, host_ring, need_gpu, outs,
                          set_head)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("observations", "actions", "next_observations", "dones", "rewards", "discounts")


def _ring(S, E, D, P, A, seed=0):
    """The coded ring with the seeded rewards (both signs, 1e-3 .. 1e6) and Bernoulli(0.25) dones."""
    return coded_ring(S, E, D, P, A, seed=seed, ring_seed=RING_SEED)


def _assert_nstep(smp, steps, want, tag):
    """The six fields of an NStepReplayBufferSamples and the steps block against the model's seven."""
    assert smp._fields == FIELDS
    assert_batch(smp, want, tag, steps=steps)


def _all_pairs(S, E):
    return np.stack([np.repeat(np.arange(S), E), np.tile(np.arange(E), S)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# 1. the gather over every pair of the ring
# ------------------------------------------------------------------------------------------------
S8, E70 = 8, 70
HEADS = (3, S8 - 1, S8 + 3)        # stored steps: ring not full; exactly S - 1; pos mid-ring, wrapping
N_STEPS = (1, 2, 3, 7)
GAMMAS = (0.99, 1.0, 0.0)


def _assert_every_ending_occurs(rew, done, pairs, pos, n):
    """On the model alone: every m in 1..n is reached by a done, every m < n by the head, and the
    full m = n without a done -- no branch of the kernel is left unexercised by luck of the seed."""
    m, by_done, by_head = nm.end_kinds(rew, done, pairs, pos, n)
    assert m.min() >= 1 and m.max() <= n
    for k in range(1, n + 1):
        assert (by_done & (m == k)).any(), f"pos={pos} n={n}: no return of length {k} ended by a done"
    for k in range(1, n):
        assert (by_head & (m == k)).any(), f"pos={pos} n={n}: no return of length {k} cut by the head"
    assert ((m == n) & ~by_done).any(), f"pos={pos} n={n}: no full-length return without a done"


@pytest.mark.parametrize("D,P,A", [(5, 16, 1), (5, 16, 6), (13, 13, 3), (301, 304, 30), (51, 51, 10)])
def test_gather_nstep_equals_model_on_every_pair(D, P, A):
    """(5, 16, 1) is the 4-lane group, where n = 7 exceeds the group and takes the chunk loop;
    (5, 16, 6) the same group with more action floats than lanes, the loop behind the stores;
    (13, 13, 3) the unaligned dword path; (301, 304, 30) a whole wave per sample in 16-byte units;
    (51, 51, 10) half a wave in dwords.  E = 70: one full wave of lanes and a 6-lane tail."""
    need_gpu()
    S, E = S8, E70
    buf, host = _ring(S, E, D, P, A)
    pairs = _all_pairs(S, E)
    idx = torch.from_numpy(pairs).cuda()
    for stored in HEADS:
        pos, n_valid = rm.head_after(stored, S)
        set_head(buf, pos, n_valid)
        for n in N_STEPS:
            _assert_every_ending_occurs(host[2], host[3], pairs, pos, n)
            for gamma in GAMMAS:
                want = nm.nstep_lookup(*host, pairs, pos, n, gamma)
                smp = buf.gather_nstep(idx, n, gamma)
                _assert_nstep(smp, buf.last_steps, want, f"stored={stored} n={n} gamma={gamma}")
    assert smp.observations.shape == (S * E, D) and smp.discounts.shape == (S * E, 1)
    assert buf.last_steps.dtype == torch.int32 and buf.last_steps.shape == (S * E,)


# ------------------------------------------------------------------------------------------------
# 2. n = 1 is the one-step sampler
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,P,A", [(13, 13, 3), (301, 304, 30)])
def test_nstep_1_is_the_one_step_sampler(D, P, A):
    need_gpu()
    S, E, B, seed = S8, E70, 257, 9
    buf, _ = _ring(S, E, D, P, A, seed=seed)
    for stored in HEADS:
        set_head(buf, *rm.head_after(stored, S))
        for draw, gamma in ((0, 0.99), (5, 1.0), (2 ** 33 + 1, 0.0), (7, 0.5)):
            buf.draw.fill_(draw)
            one = [t.clone() for t in buf.sample(B)]
            one_idx = buf.last_indices.clone()
            buf.draw.fill_(draw)
            got = buf.sample_nstep(B, 1, gamma)
            assert torch.equal(buf.last_indices, one_idx)
            for name, a, b in zip(FIELDS, one, got):
                assert torch.equal(a, b), f"{name} stored={stored} draw={draw}"
            assert (got.discounts.cpu().numpy() == np.float32(gamma)).all()
            assert (buf.last_steps == 1).all()


# ------------------------------------------------------------------------------------------------
# 3. the draw
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 0x123456789ABCDEF])
def test_sample_nstep_draws_the_one_step_pairs(seed):
    need_gpu()
    S, E, D, P, A, n, gamma = S8, E70, 13, 13, 3, 3, 0.99
    buf, host = _ring(S, E, D, P, A, seed=seed)
    with pytest.raises(ValueError):
        buf.sample_nstep(4, n, gamma)                                  # nothing stored yet
    draws = 0
    for stored in HEADS:
        pos, n_valid = rm.head_after(stored, S)
        set_head(buf, pos, n_valid)
        for B in (1, 3, 257):
            seen = []
            for _ in range(2):
                smp = buf.sample_nstep(B, n, gamma)
                want_idx = nm.draw_pairs(seed, draws, B, pos, n_valid, S, E)
                np.testing.assert_array_equal(buf.last_indices.cpu().numpy(), want_idx,
                                              err_msg=f"stored={stored} B={B} draw={draws}")
                want = nm.nstep_lookup(*host, want_idx, pos, n, gamma)
                _assert_nstep(smp, buf.last_steps, want, f"stored={stored} B={B} draw={draws}")
                kept = [t.clone() for t in smp]
                again = buf.gather_nstep(buf.last_indices, n, gamma)   # the same pairs, the gather form
                for k, g in zip(kept, again):
                    assert torch.equal(k, g)
                seen.append(want_idx)
                draws += 1
                assert buf.draws == draws and int(buf.draw.item()) == draws
            if B == 257:
                assert not np.array_equal(seen[0], seen[1])            # a second call draws other pairs
    with pytest.raises(ValueError):
        buf.sample_nstep(4, 0, gamma)
    with pytest.raises(ValueError):
        buf.sample_nstep(4, S, gamma)
    with pytest.raises(ValueError):
        buf.sample_nstep(4, 3, float("nan"))
    with pytest.raises(ValueError):
        buf.gather_nstep(buf.last_indices, 3, 1.5)


# ------------------------------------------------------------------------------------------------
# 4. untrusted head words
# ------------------------------------------------------------------------------------------------
def test_untrusted_head_words_do_not_leave_the_ring():
    """Whatever pos holds every slot is reduced mod S; n_valid is clamped into [1, S - 1] for the
    draw.  The outputs equal the model evaluated with the words reduced in that way."""
    need_gpu()
    S, E, D, P, A, B, n, gamma, seed = S8, E70, 13, 13, 3, 257, 3, 0.99, 21
    buf, host = _ring(S, E, D, P, A, seed=seed)
    all_pairs = _all_pairs(S, E)
    all_idx = torch.from_numpy(all_pairs).cuda()
    draws = 0
    for pos in (-5, S, 2 ** 31 - 1):
        for nv in (-1, 0, S + 7):
            set_head(buf, 2, 1)
            buf.head.copy_(torch.tensor([pos, nv], dtype=torch.int32))
            smp = buf.sample_nstep(B, n, gamma)
            torch.cuda.synchronize()
            idx = buf.last_indices.cpu().numpy()
            steps = buf.last_steps.cpu().numpy()
            assert idx[0].min() >= 0 and idx[0].max() < S and idx[1].min() >= 0 and idx[1].max() < E
            assert steps.min() >= 1 and steps.max() <= n
            np.testing.assert_array_equal(
                idx, nm.draw_pairs(seed, draws, B, pos, nm.clamp_n_valid(nv, S), S, E))
            _assert_nstep(smp, buf.last_steps, nm.nstep_lookup(*host, idx, pos, n, gamma),
                          f"sample head=({pos}, {nv})")
            draws += 1
            smp = buf.gather_nstep(all_idx, n, gamma)
            _assert_nstep(smp, buf.last_steps, nm.nstep_lookup(*host, all_pairs, pos, n, gamma),
                          f"gather head=({pos}, {nv})")


# ------------------------------------------------------------------------------------------------
# 5. caller indices are clamped
# ------------------------------------------------------------------------------------------------
def test_gather_nstep_clamps_indices():
    """The C ABI on a view of slots 1 .. 4 of a 7-slot ring: every address the kernel would form from
    the unclamped indices below lies inside the 7-slot tensors."""
    need_gpu()
    from finrl_amd import _native as nat
    E, D, P, A, B, n, gamma = 6, 12, 12, 3, 6, 3, 0.5
    big, host = _ring(7, E, D, P, A)
    Sv, pos = 4, 2
    view = nat.ReplayViewPtrs(big._obs_buf[1].data_ptr(), big.actions[1].data_ptr(),
                              big.rewards[1].data_ptr(), big.dones[1].data_ptr(), Sv, E, D, P, A, 0)
    host_v = tuple(h[1:1 + Sv] for h in host)
    raw = np.array([[-1, -1, Sv, Sv, 1, 2], [0, E + 1, -1, 3, -1, E + 1]], dtype=np.int32)
    clamped = np.array([[0, 0, Sv - 1, Sv - 1, 1, 2], [0, E - 1, 0, 3, 0, E - 1]], dtype=np.int32)
    out, _ = outs(B, D, A, "slice", 6)
    o, a_o, nx, d_o, r_o, g_o = out
    steps = torch.zeros(B, dtype=torch.int32, device="cuda")
    head = torch.tensor([pos, Sv - 1], dtype=torch.int32, device="cuda")
    batch = nat.ReplayBatchPtrs(o.data_ptr(), nx.data_ptr(), a_o.data_ptr(), r_o.data_ptr(),
                                d_o.data_ptr(), B, o.stride(0))
    ns = nat.ReplayNStepPtrs(head.data_ptr(), g_o.data_ptr(), steps.data_ptr(), n, gamma)
    idx = torch.from_numpy(raw).cuda()
    rc = nat.lib().finenv_replay_gather_nstep(C.byref(view), C.c_void_p(idx.data_ptr()), C.byref(batch),
                                              C.byref(ns), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    want = nm.nstep_lookup(*host_v, clamped, pos, n, gamma)
    for name, g, w in zip(FIELDS + ("steps",), out + (steps,), want):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    # steps = NULL is allowed: the same six outputs
    out2, _ = outs(B, D, A, "slice", 6)
    o, a_o, nx, d_o, r_o, g_o = out2
    batch = nat.ReplayBatchPtrs(o.data_ptr(), nx.data_ptr(), a_o.data_ptr(), r_o.data_ptr(),
                                d_o.data_ptr(), B, o.stride(0))
    ns = nat.ReplayNStepPtrs(head.data_ptr(), g_o.data_ptr(), None, n, gamma)
    rc = nat.lib().finenv_replay_gather_nstep(C.byref(view), C.c_void_p(idx.data_ptr()), C.byref(batch),
                                              C.byref(ns), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    for a, b in zip(out, out2):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# 6. out=
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,P,A", [(5, 16, 1), (13, 13, 3), (301, 304, 30)])
def test_out_tensors_and_their_pad_columns(D, P, A):
    """out= with a pitched slice (and with packed rows one float past an allocation) for the two
    observation outputs: nothing outside the D columns is written."""
    need_gpu()
    S, E, n, gamma = S8, E70, 3, 0.99
    buf, host = _ring(S, E, D, P, A, seed=2)
    pos, n_valid = rm.head_after(S + 3, S)
    set_head(buf, pos, n_valid)
    pairs = _all_pairs(S, E)[:, ::3]
    B = pairs.shape[1]
    idx = torch.from_numpy(np.ascontiguousarray(pairs)).cuda()
    want = nm.nstep_lookup(*host, pairs, pos, n, gamma)
    for kind in ("slice", "packed"):
        out, back = outs(B, D, A, kind, 6)
        got = buf.gather_nstep(idx, n, gamma, out=out)
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        _assert_nstep(got, buf.last_steps, want, f"gather out={kind}")
        out_s, back_s = outs(B, D, A, kind, 6)
        draw = buf.draws
        got = buf.sample_nstep(B, n, gamma, out=out_s)
        drawn = buf.last_indices.cpu().numpy()
        np.testing.assert_array_equal(drawn, nm.draw_pairs(2, draw, B, pos, n_valid, S, E))
        _assert_nstep(got, buf.last_steps, nm.nstep_lookup(*host, drawn, pos, n, gamma),
                      f"sample out={kind}")
        for b in back + back_s:
            b = b.cpu().numpy()
            if kind == "packed":
                assert b[0] == POISON
            else:
                assert (b[:, :4] == POISON).all() and (b[:, 4 + D:] == POISON).all()
    with pytest.raises(ValueError):
        buf.gather_nstep(idx, n, gamma, out=out[:5])                   # six tensors, not five
    bad = list(outs(B, D, A, "slice", 6)[0])
    bad[5] = torch.zeros(B, 2, device="cuda")[:, :1]                   # discounts not contiguous
    with pytest.raises(ValueError):
        buf.gather_nstep(idx, n, gamma, out=bad)


# ------------------------------------------------------------------------------------------------
# 7. inside a captured graph, and through a real env
# ------------------------------------------------------------------------------------------------
def test_captured_sample_nstep_follows_the_ring_and_the_draw_word():
    """One captured sample_nstep, replayed after further buf.step calls: each replay equals the model
    for the ring, the head and the draw number as they are at that replay, with the n and gamma of
    the capture."""
    need_gpu()
    from finrl_amd import ReplayBuffer
    E, S, B, seed, n, gamma = E70, S8, 257, 5, 3, 0.99
    env = crypto_env(E)
    D, A = env.obs.shape[1], env.action_dim
    buf = ReplayBuffer(S, E, D, A, obs_pitch="packed", seed=seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    acts = [torch.rand(E, A, generator=gen, device="cuda") * 2 - 1 for _ in range(11)]
    buf.start(env, env.reset())
    for a in acts[:2]:
        buf.step(env, a)
    buf.sample_nstep(B, n, gamma)                            # first call outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pass
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        smp = buf.sample_nstep(B, n, gamma)
    idx, steps = buf.last_indices, buf.last_steps
    stored, lengths = 2, set()
    for more in (0, 2, 7):                                   # 2, 4 and 11 = S + 3 stored steps
        for a in acts[stored:stored + more]:
            buf.step(env, a)
        stored += more
        draw = int(buf.draw.item())
        g.replay()
        torch.cuda.synchronize()
        assert int(buf.draw.item()) == draw + 1              # the bump is part of the capture
        pos, n_valid = rm.head_after(stored, S)
        assert buf.head.tolist() == [pos, n_valid]
        want_idx = nm.draw_pairs(seed, draw, B, pos, n_valid, S, E)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_idx, err_msg=f"after {stored} steps")
        want = nm.nstep_lookup(*host_ring(buf), want_idx, pos, n, gamma)
        _assert_nstep(smp, steps, want, f"after {stored} steps")
        lengths |= set(want[6].tolist())
    assert lengths == {1, 2, 3}


def test_gather_nstep_through_a_real_env():
    """S + 3 buf.step calls of VecCryptoEnv on a 7-row panel (episodes end inside the 8-slot ring),
    then the n-step batch of every pair against the model on host copies of the ring."""
    need_gpu()
    from finrl_amd import ReplayBuffer
    E, S = E70, S8
    env = crypto_env(E)
    D, A = env.obs.shape[1], env.action_dim
    buf = ReplayBuffer(S, E, D, A, obs_pitch="packed", seed=3)
    rng = np.random.default_rng(7)
    buf.start(env, env.reset())
    for _ in range(S + 3):
        buf.step(env, torch.from_numpy(rng.uniform(-1, 1, (E, A)).astype(np.float32)).cuda())
    pos, n_valid = rm.head_after(S + 3, S)
    assert buf.head.tolist() == [pos, n_valid]
    host = host_ring(buf)
    pairs = _all_pairs(S, E)
    idx = torch.from_numpy(pairs).cuda()
    valid = np.isin(pairs[0], rm.valid_slots(pos, n_valid, S))
    for n, gamma in ((3, 0.99), (5, 0.9), (S - 1, 1.0)):
        m, by_done, _ = nm.end_kinds(host[2], host[3], pairs, pos, n)
        assert (valid & by_done & (m >= 2)).any()            # a done lies inside a window, past its start
        if n == 3:
            assert (valid & ~by_done & (m == n)).any()       # and a full window without one
        want = nm.nstep_lookup(*host, pairs, pos, n, gamma)
        _assert_nstep(buf.gather_nstep(idx, n, gamma), buf.last_steps, want, f"n={n} gamma={gamma}")


# ------------------------------------------------------------------------------------------------
# 8. a ring past 4 GiB
# ------------------------------------------------------------------------------------------------
class _MarkerObs:
    """Host stand-in for the 4.33 GB obs tensor: obs[s, e] computed from the marker code."""

    def __init__(self, S, E, D, k_of):
        self.shape, self.k_of = (S, E, D), k_of

    def __getitem__(self, key):
        s, e = key
        c = np.arange(self.shape[2], dtype=np.float64)
        return np.stack([self.k_of[int(si)] * 1e6 + int(ei) * 512 + c for si, ei in zip(s, e)]).astype(np.float32)


def test_ring_past_4_gib():
    """obs of 870 slots x 4,096 envs x 304 floats (4.33 GB), marker rows in slots 0 and 866 .. 869
    only, head at pos = 1.  The late next-observation rows of the pairs below lie in slots 867, 868
    and 869, all beyond the 4 GiB offset, or wrap to slot 0; a 32-bit row offset would land elsewhere
    in the (unwritten) tensor."""
    need_gpu()
    from finrl_amd import _native as nat
    S, E, D, P, A, n, gamma = 870, 4096, 301, 304, 1, 3, 0.5
    assert 867 * E * P * 4 > 2 ** 32
    obs = torch.empty(S, E, P, dtype=torch.float32, device="cuda")
    act = torch.zeros(S, E, A, dtype=torch.float32, device="cuda")
    rew = torch.zeros(S, E, dtype=torch.float32, device="cuda")
    done = torch.zeros(S, E, dtype=torch.uint8, device="cuda")
    cols = torch.arange(P, dtype=torch.float32, device="cuda")
    envs = torch.arange(E, dtype=torch.float32, device="cuda")
    k_of = {0: 1, 866: 2, 867: 3, 868: 4, 869: 5}
    for s, k in k_of.items():
        obs[s] = k * 1e6 + envs[:, None] * 512 + cols[None, :]
        act[s] = -k * 1e4 - envs[:, None]
        rew[s] = k * 1e4 + envs
    done[867, 77] = 1                                        # m = 2 from slot 866: late row 868
    done[866, 2049] = 1                                      # m = 1: late row 867
    pairs = np.array([[866, 866, 866, 866, 867, 867], [0, E - 1, 77, 2049, 0, E - 1]], dtype=np.int32)
    B = pairs.shape[1]
    head = torch.tensor([1, S - 1], dtype=torch.int32, device="cuda")
    view = nat.ReplayViewPtrs(obs.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(),
                              S, E, D, P, A, 0)
    kw = dict(dtype=torch.float32, device="cuda")
    o, nx = torch.full((B, P), POISON, **kw), torch.full((B, P), POISON, **kw)
    a_o, r_o, d_o, g_o = (torch.zeros(B, 1, **kw) for _ in range(4))
    steps = torch.zeros(B, dtype=torch.int32, device="cuda")
    batch = nat.ReplayBatchPtrs(o.data_ptr(), nx.data_ptr(), a_o.data_ptr(), r_o.data_ptr(),
                                d_o.data_ptr(), B, P)
    ns = nat.ReplayNStepPtrs(head.data_ptr(), g_o.data_ptr(), steps.data_ptr(), n, gamma)
    idx = torch.from_numpy(pairs).cuda()
    rc = nat.lib().finenv_replay_gather_nstep(C.byref(view), C.c_void_p(idx.data_ptr()), C.byref(batch),
                                              C.byref(ns), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    want = nm.nstep_lookup(_MarkerObs(S, E, D, k_of), act.cpu().numpy(), rew.cpu().numpy(),
                           done.cpu().numpy(), pairs, 1, n, gamma)
    assert want[6].tolist() == [3, 3, 2, 1, 3, 3]
    late = (pairs[0] + want[6]) % S
    assert late.tolist() == [869, 869, 868, 867, 0, 0]
    got = (o[:, :D], a_o, nx[:, :D], d_o, r_o, g_o, steps)
    for name, g, w in zip(FIELDS + ("steps",), got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    assert (o[:, D:] == POISON).all() and (nx[:, D:] == POISON).all()
