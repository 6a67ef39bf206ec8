"""The device-resident replay buffer (finrl_amd/replay.py, finenv_replay_* in include/finenv.h) on the
MI355X, against the NumPy restatement in tests/replay_model.py.  Every output is a copy, so every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import replay_model as rm
from replay_cases import POISON, assert_batch, coded_ring, crypto_env, host_ring, need_gpu, outs, set_head

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------
# 1. the gather against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,P", [(5, 16), (13, 13), (12, 12), (301, 304), (51, 51), (100, 112)])
def test_gather_equals_model(D, P):
    """Both row paths (16-byte pieces: (5, 16), (12, 12), (301, 304), (100, 112); dwords: (13, 13),
    (51, 51) and every unaligned output), every lane-group width (4: 2 or 3 units; 8: 12 or 13; 16: the
    25 units of (100, 112); 32: 51; 64: 76, 100 and, looping past two units per lane, 301), a tail block,
    the wrap S-1 -> 0, and output pad columns that stay as they were."""
    need_gpu()
    rng = np.random.default_rng(D)
    for S in (2, 5):
        for E in (1, 70, 259):
            for A in (1, 3, 30):
                buf, host = coded_ring(S, E, D, P, A)
                for B in (1, 64, 257):
                    pairs = np.stack([rng.integers(0, S, B), rng.integers(0, E, B)]).astype(np.int32)
                    pairs[:, 0] = (S - 1, E - 1)                      # the wrap, the last env
                    if B > 1:
                        pairs[:, B - 1] = (0, 0)
                    want = rm.lookup(*host, pairs)
                    idx = torch.from_numpy(pairs).cuda()
                    tag = f"S={S} E={E} A={A} B={B}"
                    smp = buf.gather(idx)                              # the persistent outputs
                    assert_batch(smp, want, tag)
                    assert smp.observations.shape == (B, D) and smp.dones.shape == (B, 1)
                    for kind in ("packed", "slice"):
                        out, back = outs(B, D, A, kind, 5)
                        got = buf.gather(idx, out=out)
                        assert_batch(got, want, f"{tag} out={kind}")
                        for b in back:                                 # nothing outside the D columns
                            b = b.cpu().numpy()
                            if kind == "packed":
                                assert b[0] == POISON
                            else:
                                assert (b[:, :4] == POISON).all() and (b[:, 4 + D:] == POISON).all(), tag


# ------------------------------------------------------------------------------------------------
# 2. the draw against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 0x123456789ABCDEF])
def test_draw_equals_model(seed):
    need_gpu()
    S, E, D, P, A = 5, 70, 13, 13, 3
    buf, host = coded_ring(S, E, D, P, A, seed=seed)
    with pytest.raises(ValueError):
        buf.sample(4)                                                  # nothing stored yet
    draws = 0
    for pos, n_valid in ((3, 3), (1, 4)):                              # filling, full
        set_head(buf, pos, n_valid)
        assert len(buf) == n_valid
        for B in (1, 3, 257):
            for _ in range(3):                                         # consecutive draws differ
                smp = buf.sample(B)
                want_idx = rm.draw_pairs(seed, draws, B, pos, n_valid, S, E)
                np.testing.assert_array_equal(buf.last_indices.cpu().numpy(), want_idx,
                                              err_msg=f"pos={pos} B={B} draw={draws}")
                assert pos not in set(want_idx[0].tolist())
                want = rm.lookup(*host, want_idx)
                assert_batch(smp, want, f"sample B={B} draw={draws}")
                kept = [t.clone() for t in smp]
                assert_batch(buf.gather(buf.last_indices), want, "gather(last_indices)")
                for k, g in zip(kept, buf.gather(buf.last_indices)):
                    assert torch.equal(k, g)
                draws += 1
                assert buf.draws == draws and int(buf.draw.item()) == draws
    a = rm.draw_pairs(seed, 0, 257, 1, 4, S, E)
    assert not np.array_equal(a, rm.draw_pairs(seed, 1, 257, 1, 4, S, E))
    assert not np.array_equal(a, rm.draw_pairs(seed + 1, 0, 257, 1, 4, S, E))


def test_draw_covers_every_valid_pair_and_never_the_head_slot():
    need_gpu()
    S, E, B = 4, 3, 4096
    for pos in range(S):
        want = rm.draw_pairs(11, 0, B, pos, S - 1, S, E)
        valid = {(s, e) for s in range(S) if s != pos for e in range(E)}
        assert {tuple(p) for p in want.T.tolist()} == valid            # the model alone: all 9, no other
        buf, _ = coded_ring(S, E, 5, 5, 1, seed=11)
        set_head(buf, pos, S - 1)
        buf.sample(B)
        got = buf.last_indices.cpu().numpy()
        np.testing.assert_array_equal(got, want)
        assert pos not in set(got[0].tolist())


def test_untrusted_head_words_do_not_leave_the_ring():
    """n_valid < 1 is taken as 1; whatever pos holds, the slot is reduced mod S."""
    need_gpu()
    S, E = 5, 7
    buf, host = coded_ring(S, E, 5, 5, 1)
    for pos, nv in ((2, 0), (2, -5), (12, 3), (-9, 2), (1, 1000)):
        set_head(buf, 2, 1)
        buf.head.copy_(torch.tensor([pos, nv], dtype=torch.int32))
        smp = buf.sample(64)
        idx = buf.last_indices.cpu().numpy()
        assert idx[0].min() >= 0 and idx[0].max() < S and idx[1].min() >= 0 and idx[1].max() < E
        assert_batch(smp, rm.lookup(*host, idx), f"head=({pos}, {nv})")
        if nv < 1:
            assert (idx[0] == (pos - 1) % S).all()


# ------------------------------------------------------------------------------------------------
# 3. caller indices are clamped
# ------------------------------------------------------------------------------------------------
def test_gather_clamps_indices():
    """The C ABI on a view of slots 1 .. 4 of a 7-slot ring: every address the kernel would form from
    the unclamped indices below lies inside the 7-slot tensors."""
    need_gpu()
    from finrl_amd import _native as nat
    E, D, P, A, B = 6, 12, 12, 3, 6
    big, host = coded_ring(7, E, D, P, A)
    Sv = 4
    view = nat.ReplayViewPtrs(big._obs_buf[1].data_ptr(), big.actions[1].data_ptr(),
                              big.rewards[1].data_ptr(), big.dones[1].data_ptr(), Sv, E, D, P, A, 0)
    host_v = tuple(h[1:1 + Sv] for h in host)
    raw = np.array([[-1, -1, Sv, Sv, 1, 2], [0, E + 1, -1, 3, -1, E + 1]], dtype=np.int32)
    clamped = np.array([[0, 0, Sv - 1, Sv - 1, 1, 2], [0, E - 1, 0, 3, 0, E - 1]], dtype=np.int32)
    out, _ = outs(B, D, A, "slice", 5)
    o, a_o, n, d_o, r_o = out
    batch = nat.ReplayBatchPtrs(o.data_ptr(), n.data_ptr(), a_o.data_ptr(), r_o.data_ptr(),
                                d_o.data_ptr(), B, o.stride(0))
    idx = torch.from_numpy(raw).cuda()
    rc = nat.lib().finenv_replay_gather(C.byref(view), C.c_void_p(idx.data_ptr()), C.byref(batch),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    for name, g, w in zip(("observations", "actions", "next_observations", "dones", "rewards"), out,
                          rm.lookup(*host_v, clamped)):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)


# ------------------------------------------------------------------------------------------------
# 4. filling through the envs
# ------------------------------------------------------------------------------------------------
def _stock_pair(E, auto_reset=True):
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    rng = np.random.default_rng(0)
    T, N, K = 6, 30, 8
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    tech, risk = rng.normal(0, 1, (T, K, N)), np.abs(rng.normal(0, 30, T))
    kw = dict(hmax=100, initial_amount=100_000, turbulence_threshold=40.0, auto_reset=auto_reset)
    return [VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw) for _ in range(2)], None


def _crypto_pair(E, auto_reset=True):
    return [crypto_env(E, auto_reset) for _ in range(2)], "packed"


def _btc_pair(E, auto_reset=True):
    from finrl_amd.vec_btc import VecBitcoinEnv
    rng = np.random.default_rng(2)
    T, W = 6, 7
    p0 = 300.0 * np.exp(np.cumsum(rng.normal(0, 0.01, T)))
    price, tech = np.ascontiguousarray(np.stack([p0, p0 * 1.003], 1)), rng.normal(0, 3e3, (T, W))
    kw = dict(initial_account=1e3, transaction_fee_percent=1e-3, gamma=0.99, auto_reset=auto_reset)
    return [VecBitcoinEnv(price, tech, E, **kw) for _ in range(2)], "packed"


def _stocknp_pair(E, auto_reset=True):
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    rng = np.random.default_rng(3)
    T, N = 6, 5
    cfg = {"price_array": (100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))).astype(np.float32),
           "tech_array": rng.normal(0, 50, (T, N * 2)).astype(np.float32),
           "turbulence_array": np.abs(rng.normal(0, 20, T)).astype(np.float32), "if_train": False}
    return [VecStockTradingEnvNP(cfg, E, auto_reset=auto_reset) for _ in range(2)], None


def _portfolio_pair(E, auto_reset=True):
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    rng = np.random.default_rng(4)
    T, N, K = 6, 7, 3
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    panel = PortfolioPanel(close, rng.normal(0, 1e-4, (T, N, N)), rng.normal(0, 1, (T, K, N)))
    return [VecStockPortfolioEnv(panel, E, initial_amount=1e6, auto_reset=auto_reset) for _ in range(2)], "packed"


def _twowave_pair(cls_name):
    def make(E, auto_reset=True):
        import finrl_amd.vec_cashpenalty as m
        rng = np.random.default_rng(5)
        T, N, Cc = 6, 4, 3
        close = 50 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
        panel = m.CashPenaltyPanel(close, rng.normal(0, 10, (T, N, Cc)))
        kw = dict(hmax=5_000, initial_amount=1e5, random_start=False, auto_reset=auto_reset)
        return [getattr(m, cls_name)(panel, E, **kw) for _ in range(2)], "packed"
    return make


@pytest.mark.parametrize("make", [_stock_pair, _crypto_pair, _btc_pair, _stocknp_pair, _portfolio_pair,
                                  _twowave_pair("VecCashPenaltyEnv"), _twowave_pair("VecStopLossEnv")],
                         ids=["stock", "crypto", "btc", "stocknp", "portfolio", "cashpenalty", "stoploss"])
def test_filling_through_the_env(make):
    """buf.step against a twin env stepped with the same actions: after every one of 9 steps into a
    4-slot ring every valid slot holds the twin's record of its step (rows of finished episodes, whose
    next observation is the next episode's first, included), sample(257) is a look-up in that record,
    and the host mirror and the device head agree."""
    need_gpu()
    from finrl_amd import ReplayBuffer
    E, S, n_steps = 70, 4, 9
    (env, twin), pitch = make(E)
    D, A = env.obs.shape[1], env.action_dim
    buf = ReplayBuffer(S, E, D, A, obs_pitch=pitch, seed=3)
    assert buf.obs_pitch == (D if pitch == "packed" else (D + 15) // 16 * 16)
    rng = np.random.default_rng(7)
    seen = twin.reset().clone()
    buf.start(env, env.reset())
    assert torch.equal(buf.obs[0], seen) and len(buf) == 0
    record, saw_done = [], False                    # per step: obs before, action, reward, done, obs after
    for n in range(1, n_steps + 1):
        a = torch.from_numpy(rng.uniform(-1, 1, (E, A)).astype(np.float32)).cuda()
        o, r, d, _ = twin.step(a)
        record.append(tuple(x.cpu().numpy() for x in (seen, a, r, d, o)))
        seen = o.clone()
        ret = buf.step(env, a)
        assert torch.equal(ret[0], o) and torch.equal(ret[1], r) and torch.equal(ret[2], d)
        pos, n_valid = rm.head_after(n, S)
        assert (buf.pos, len(buf)) == (pos, n_valid) and buf.head.tolist() == [pos, n_valid]
        ring = [x.cpu().numpy() for x in (buf.obs, buf.actions, buf.rewards, buf.dones)]
        for j, s in enumerate(rm.valid_slots(pos, n_valid, S)):
            ob, ac, rw, dn, nx = record[n - 1 - j]
            for got, want, what in ((ring[0][s], ob, "obs"), (ring[1][s], ac, "action"),
                                    (ring[2][s], rw, "reward"), (ring[3][s], dn, "done"),
                                    (ring[0][(s + 1) % S], nx, "next_obs")):
                np.testing.assert_array_equal(got, want, err_msg=f"step {n} slot {s} {what}")
            saw_done = saw_done or bool(dn.any())
        smp = buf.sample(257)
        idx = buf.last_indices.cpu().numpy()
        np.testing.assert_array_equal(idx, rm.draw_pairs(3, n - 1, 257, pos, n_valid, S, E))
        step_of = {s: n - 1 - j for j, s in enumerate(rm.valid_slots(pos, n_valid, S))}
        rows = [record[step_of[s]] for s in idx[0]]
        e = idx[1]
        want = (np.stack([rw_[0][k] for rw_, k in zip(rows, e)]), np.stack([rw_[1][k] for rw_, k in zip(rows, e)]),
                np.stack([rw_[4][k] for rw_, k in zip(rows, e)]),
                np.array([rw_[3][k] for rw_, k in zip(rows, e)], dtype=np.float32)[:, None],
                np.array([rw_[2][k] for rw_, k in zip(rows, e)], dtype=np.float32)[:, None])
        assert_batch(smp, want, f"sample after step {n}")
    assert saw_done                                  # an episode ended inside a valid slot
    (manual, _), _ = make(E, auto_reset=False)
    manual.reset()
    with pytest.raises(ValueError):
        buf.step(manual, a)


def test_packed_env_needs_a_packed_ring():
    need_gpu()
    from finrl_amd import ReplayBuffer
    (env, _), _ = _crypto_pair(8)
    D = env.obs.shape[1]
    buf = ReplayBuffer(3, 8, D, env.action_dim)             # the aligned default: rows 16 floats apart
    assert buf.obs_pitch != D
    buf.start(env, env.reset())
    with pytest.raises(ValueError):
        buf.step(env, torch.zeros(8, env.action_dim, device="cuda"))


# ------------------------------------------------------------------------------------------------
# 5. inside a captured graph
# ------------------------------------------------------------------------------------------------
def test_captured_sample_follows_the_ring_and_the_draw_word():
    need_gpu()
    from finrl_amd import ReplayBuffer
    E, S, B, seed = 70, 8, 257, 5
    (env, _), pitch = _crypto_pair(E)
    D, A = env.obs.shape[1], env.action_dim
    buf = ReplayBuffer(S, E, D, A, obs_pitch=pitch, seed=seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    acts = [torch.rand(E, A, generator=gen, device="cuda") * 2 - 1 for _ in range(4)]
    buf.start(env, env.reset())
    for a in acts[:2]:
        buf.step(env, a)
    buf.sample(B)                                            # first call outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pass
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        smp = buf.sample(B)
    idx = buf.last_indices
    new_slots = set()
    for n_steps in (2, 4):
        draw = int(buf.draw.item())
        g.replay()
        torch.cuda.synchronize()
        assert int(buf.draw.item()) == draw + 1              # the bump is part of the capture
        pos, n_valid = rm.head_after(n_steps, S)
        want_idx = rm.draw_pairs(seed, draw, B, pos, n_valid, S, E)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_idx, err_msg=f"after {n_steps} steps")
        assert_batch(smp, rm.lookup(*host_ring(buf), want_idx), f"after {n_steps} steps")
        if n_steps == 2:
            assert set(want_idx[0].tolist()) <= {0, 1}
            for a in acts[2:]:
                buf.step(env, a)
        else:
            new_slots = set(want_idx[0].tolist()) & {2, 3}
    assert new_slots                                         # the second replay drew from the new slots


def test_captured_step_segment_publishes_its_own_head():
    """Three buf.step calls captured once: replayed twice from the same restored state they write
    the same slots and the same head, and what they write is what three eager steps write."""
    need_gpu()
    from finrl_amd import ReplayBuffer
    E, S = 70, 4
    (env, _), pitch = _crypto_pair(E)
    D, A = env.obs.shape[1], env.action_dim
    buf = ReplayBuffer(S, E, D, A, obs_pitch=pitch)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    acts = [torch.rand(E, A, generator=gen, device="cuda") * 2 - 1 for _ in range(5)]
    buf.start(env, env.reset())
    for a in acts[:2]:
        buf.step(env, a)
    state = [t for t in (env._f64, env._i32, env._f32) if t is not None]
    ring = [buf._obs_buf, buf.actions, buf.rewards, buf.dones]
    snap = [t.clone() for t in state + ring]
    before = (buf.pos, len(buf))

    def restore():
        for t, s in zip(state + ring, snap):
            t.copy_(s)
        buf.head.fill_(-1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pass
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for a in acts[2:]:
            buf.step(env, a)
    assert (buf.pos, len(buf)) == rm.head_after(5, S) == (1, 3)
    results = []
    for _ in range(2):
        restore()
        g.replay()
        torch.cuda.synchronize()
        results.append([t.clone() for t in ring + state] + [buf.head.clone()])
        assert buf.head.tolist() == [1, 3]
    restore()
    buf.pos, buf._n_valid = before
    for a in acts[2:]:
        buf.step(env, a)
    results.append([t.clone() for t in ring + state] + [buf.head.clone()])
    for other in results[1:]:
        for x, y in zip(results[0], other):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------
# 6. a ring past 4 GiB
# ------------------------------------------------------------------------------------------------
def test_ring_past_4_gib():
    """obs of 870 slots x 4,096 envs x 304 floats (4.33 GB): marker rows in slots 0, 868 and 869 only;
    the next observation of slot 869 wraps to slot 0.  A 32-bit row offset would land elsewhere in
    the (unwritten) tensor."""
    need_gpu()
    from finrl_amd import _native as nat
    S, E, D, P, A, B = 870, 4096, 301, 304, 1, 6
    assert S * E * P * 4 > 2 ** 32
    obs = torch.empty(S, E, P, dtype=torch.float32, device="cuda")
    act = torch.zeros(S, E, A, dtype=torch.float32, device="cuda")
    rew = torch.zeros(S, E, dtype=torch.float32, device="cuda")
    done = torch.zeros(S, E, dtype=torch.uint8, device="cuda")
    cols = torch.arange(P, dtype=torch.float32, device="cuda")
    envs = torch.arange(E, dtype=torch.float32, device="cuda")
    for k, s in enumerate((0, 868, 869)):
        obs[s] = (k + 1) * 1e6 + envs[:, None] * 512 + cols[None, :]
        act[s] = -(k + 1) * 1e4 - envs[:, None]
        rew[s] = (k + 1) * 1e4 + envs
        done[s] = k % 2
    pairs = np.array([[868, 868, 869, 869, 869, 868], [0, E - 1, 0, E - 1, 2049, 77]], dtype=np.int32)
    view = nat.ReplayViewPtrs(obs.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(),
                              S, E, D, P, A, 0)
    kw = dict(dtype=torch.float32, device="cuda")
    o, n = torch.full((B, P), POISON, **kw), torch.full((B, P), POISON, **kw)
    a_o, r_o, d_o = torch.zeros(B, A, **kw), torch.zeros(B, **kw), torch.zeros(B, **kw)
    batch = nat.ReplayBatchPtrs(o.data_ptr(), n.data_ptr(), a_o.data_ptr(), r_o.data_ptr(),
                                d_o.data_ptr(), B, P)
    idx = torch.from_numpy(pairs).cuda()
    rc = nat.lib().finenv_replay_gather(C.byref(view), C.c_void_p(idx.data_ptr()), C.byref(batch),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    k_of = {0: 1, 868: 2, 869: 3}
    s, e = pairs.astype(np.int64)
    c = np.arange(D, dtype=np.float64)
    want_o = np.stack([k_of[si] * 1e6 + ei * 512 + c for si, ei in zip(s, e)]).astype(np.float32)
    want_n = np.stack([k_of[(si + 1) % S] * 1e6 + ei * 512 + c for si, ei in zip(s, e)]).astype(np.float32)
    np.testing.assert_array_equal(o.cpu().numpy()[:, :D], want_o)
    np.testing.assert_array_equal(n.cpu().numpy()[:, :D], want_n)
    assert (o[:, D:] == POISON).all() and (n[:, D:] == POISON).all()
    np.testing.assert_array_equal(a_o.cpu().numpy()[:, 0], [-k_of[si] * 1e4 - ei for si, ei in zip(s, e)])
    np.testing.assert_array_equal(r_o.cpu().numpy(), [k_of[si] * 1e4 + ei for si, ei in zip(s, e)])
    np.testing.assert_array_equal(d_o.cpu().numpy(), [(k_of[si] - 1) % 2 for si, ei in zip(s, e)])
