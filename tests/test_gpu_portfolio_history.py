"""Episode history of the batched portfolio env (VecStockPortfolioEnv.enable_history(),
finenv_portfolio_set_history) on the MI355X.  The record is made of the very values the step computes,
so wherever the comparison is with this build's own step it is exact (tolerance 0): value against
state["value"], ret against the step's own return (read through a zeroed run_sum of the last-episode
block), weights against env.weights, row against state["day"].  mean / std / Sharpe of metrics() against
pandas keep the bound the project uses for that quantity across summation orders (rtol 1e-9,
atol 1e-12)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

COMPLETE, OVERFLOW = 1, 2
KEYS = ("value", "ret", "row", "weights", "length", "flags")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _random_panel(seed, T, N, K):
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    cov = rng.normal(0, 1e-4, (T, N, N))
    tech = rng.normal(0, 1, (T, K, N))
    return close, cov, tech


def _env(close, cov, tech, E, **kw):
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    return VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, **kw)


def _host(hist):
    return {k: (None if getattr(hist, k) is None else getattr(hist, k).cpu().numpy()) for k in KEYS}


def _clone(hist):
    return {k: getattr(hist, k).clone() for k in KEYS if getattr(hist, k) is not None}


class _Tracker:
    """The recording rule of include/finenv.h restated on the host, per env: fed with each step's
    `done` and the values the step left behind (state, weights, the step's return), it holds what the
    record must contain."""

    def __init__(self, E, cap):
        self.E, self.cap = E, cap
        self.rec = [None] * E                      # per env: list of (value, ret, row, weights) or None
        self.flags = np.zeros(E, np.int32)

    def arm(self, ids, value, day, N):
        w0 = np.full(N, np.float32(1 / N), np.float32)
        for e in ids:
            self.rec[e] = [(value[e], 0.0, int(day[e]), w0)]
            self.flags[e] = 0

    def step(self, done, value, ret, day, weights):
        for e in range(self.E):
            if self.rec[e] is None or self.flags[e] & COMPLETE:
                continue
            if done[e]:
                self.flags[e] |= COMPLETE
            elif len(self.rec[e]) >= self.cap:
                self.flags[e] |= OVERFLOW
            else:
                self.rec[e].append((value[e], ret[e], int(day[e]), weights[e].copy()))

    def check(self, hist, what=""):
        h = _host(hist)
        for e in range(self.E):
            msg = f"{what} env {e}"
            if self.rec[e] is None:
                assert h["length"][e] == 0, msg
                continue
            n = len(self.rec[e])
            assert h["length"][e] == n, (msg, h["length"][e], n)
            assert h["flags"][e] == self.flags[e], (msg, h["flags"][e], self.flags[e])
            np.testing.assert_array_equal(h["value"][:n, e], [r[0] for r in self.rec[e]], err_msg=msg)
            np.testing.assert_array_equal(h["ret"][:n, e], [r[1] for r in self.rec[e]], err_msg=msg)
            np.testing.assert_array_equal(h["row"][:n, e], [r[2] for r in self.rec[e]], err_msg=msg)
            np.testing.assert_array_equal(h["weights"][:n, e], np.stack([r[3] for r in self.rec[e]]),
                                          err_msg=msg)
            v, r = h["value"][:n, e], h["ret"][:n, e]
            np.testing.assert_array_equal(v[1:], v[:-1] * (1 + r[1:]), err_msg=msg)   # :187-188, fp64


# ------------------------------------------------------------------------------------------------
# 1. + 2. the record equals the step, every step; lifecycle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("windows", [False, True])
@pytest.mark.parametrize("desync", [False, True])
@pytest.mark.parametrize("N", [1, 2, 7, 8, 30, 33, 64])
def test_record_equals_the_step_every_step(N, desync, windows):
    """Random panel, E not a multiple of 64, distinct actions per env, weights output and last-episode
    block attached.  run_sum is zeroed before each step, so after it the row holds exactly this step's
    portfolio_return (0 + ret).  Lock-step, and desynchronised by masked resets (which re-arm) so that the
    entry index differs inside a block; without and with per-env windows (WIN x HIST).  done / day are
    checked against the CPU oracle where the batch is the oracle's (no windows, no masked resets)."""
    _need_gpu()
    from oracle.portfolio import PortfolioOracle
    E, T, K = 150 + N, 12, 2
    close, cov, tech = _random_panel(N, T, N, K)
    rng = np.random.default_rng(100 + N)
    kw = {}
    s = np.zeros(E, np.int64)
    if windows:
        length = rng.integers(2, T + 1, E)
        s = (rng.random(E) * (T - length + 1)).astype(np.int64)
        kw["windows"] = (s, s + length)
    env = _env(close, cov, tech, E, initial_amount=250_000, auto_reset=True, **kw)
    env.enable_weights()
    env.enable_last_episode()
    hist = env.enable_history()
    assert env.enable_history() is hist and hist.capacity == env.max_step + 1
    tr = _Tracker(E, hist.capacity)
    st = env.state_numpy()
    tr.arm(range(E), st["value"], st["day"], N)
    tr.check(hist, "armed by enable_history")
    env.reset()
    st = env.state_numpy()
    np.testing.assert_array_equal(st["day"], s)
    tr.arm(range(E), st["value"], st["day"], N)
    orc = None
    if not windows and not desync:
        orc = PortfolioOracle(close, cov, tech, n_envs=E, initial_amount=250_000)
        orc.reset()
    for step in range(2 * T + 4):
        a = rng.uniform(0, 1, (E, N)).astype(np.float32)
        env.last_episode["run_sum"].zero_()
        _, _, done, _ = env.step(torch.from_numpy(a).cuda())
        done = done.cpu().numpy().astype(bool)
        ret = env.last_episode["run_sum"].cpu().numpy()
        st = env.state_numpy()
        if orc is not None:
            o_done = orc.vec_step(a, want_obs=False)[2]
            np.testing.assert_array_equal(done, o_done)
            np.testing.assert_array_equal(st["day"], orc.state()["day"])
        # a non-terminal step moved the env to st["day"] and left st["value"]; a terminal one recorded nothing
        tr.step(done, st["value"], ret, st["day"], env.weights.cpu().numpy())
        if desync and step in (2, 5, 9, 16):
            m = rng.random(E) < 0.3
            env.reset(torch.from_numpy(m.astype(np.uint8)).cuda())
            st = env.state_numpy()
            tr.arm(np.nonzero(m)[0], st["value"], st["day"], N)
            assert (st["value"][m] == 250_000).all() and (st["day"][m] == s[m]).all()
        if step in (3, T + 1):
            tr.check(hist, f"step {step}")
    tr.check(hist, "end")
    assert (tr.flags & COMPLETE).astype(bool).sum() > E // 2
    assert not bool(hist.overflow.any())


def test_first_episode_survives_auto_reset_and_reset_rearms():
    """The tracker's `done` and `day` come from oracle/portfolio.py throughout (the oracle has no return;
    value, return and weights are the step's own, compared through test 1): a step kernel with a wrong
    terminal test cannot mislead the tracker the way it would corrupt the record."""
    _need_gpu()
    from oracle.portfolio import PortfolioOracle
    from oracle.stock import lib
    E, T, N, K = 200, 10, 30, 3
    close, cov, tech = _random_panel(11, T, N, K)
    env = _env(close, cov, tech, E, initial_amount=1e6, auto_reset=True)
    env.enable_weights()
    env.enable_last_episode()
    with pytest.raises(Exception, match="enable_history"):
        env.save_asset_memory()
    hist = env.enable_history()
    rng = np.random.default_rng(5)
    tr = _Tracker(E, hist.capacity)
    orc = PortfolioOracle(close, cov, tech, n_envs=E, initial_amount=1e6)
    env.reset()
    orc.reset()
    st = env.state_numpy()
    tr.arm(range(E), st["value"], orc.state()["day"], N)

    def run(n):
        for _ in range(n):
            a = rng.uniform(0, 1, (E, N)).astype(np.float32)
            env.last_episode["run_sum"].zero_()
            _, _, done, _ = env.step(torch.from_numpy(a).cuda())
            o_done = orc.vec_step(a, want_obs=False)[2]
            o_day = orc.state()["day"]
            st = env.state_numpy()
            np.testing.assert_array_equal(done.cpu().numpy().astype(bool), o_done)
            np.testing.assert_array_equal(st["day"], o_day)
            tr.step(o_done, st["value"], env.last_episode["run_sum"].cpu().numpy(), o_day,
                    env.weights.cpu().numpy())

    run(T + 3)                                   # past the first episode end (lock-step: step T)
    assert bool(hist.complete.all()) and int(hist.length.min()) == T
    tr.check(hist, "first episode")
    snap = _clone(hist)
    run(5)
    assert all(torch.equal(getattr(hist, k), v) for k, v in snap.items()), \
        "a finished record changed under later steps"
    # reset(mask) re-arms exactly the masked envs
    mask = rng.random(E) < 0.4
    env.reset(torch.from_numpy(mask.astype(np.uint8)).cuda())
    for j in np.nonzero(mask)[0]:
        lib().pf_oracle_reset_env(orc._h, C.c_int(int(j)), None)
    st = env.state_numpy()
    np.testing.assert_array_equal(st["day"], orc.state()["day"])
    tr.arm(np.nonzero(mask)[0], st["value"], orc.state()["day"], N)
    h = _host(hist)
    np.testing.assert_array_equal(h["length"][mask], 1)
    np.testing.assert_array_equal(h["flags"][mask], 0)
    np.testing.assert_array_equal(h["row"][0][mask], 0)
    np.testing.assert_array_equal(h["value"][0][mask], 1e6)
    np.testing.assert_array_equal(h["ret"][0][mask], 0.0)
    np.testing.assert_array_equal(h["weights"][0][mask], np.float32(1 / N))
    keep = torch.nonzero(torch.from_numpy(~mask).cuda())[:, 0]
    for k, v in snap.items():                    # the others keep their finished record
        dim = 0 if v.dim() == 1 else 1
        assert torch.equal(getattr(hist, k).index_select(dim, keep), v.index_select(dim, keep)), k
    run(T + 2)
    tr.check(hist, "episode after reset(mask)")
    assert bool(hist.complete.all())
    # arm(mask) mid-episode starts at the current value and row
    run(2)
    mask2 = rng.random(E) < 0.5
    st = env.state_numpy()
    assert (st["day"][mask2] != 0).sum() > 10
    hist.arm(torch.from_numpy(mask2).cuda())
    tr.arm(np.nonzero(mask2)[0], st["value"], st["day"], N)
    h = _host(hist)
    np.testing.assert_array_equal(h["value"][0][mask2], st["value"][mask2])
    np.testing.assert_array_equal(h["row"][0][mask2], st["day"][mask2])
    run(3)
    tr.check(hist, "after arm(mask)")
    # frames: a single index gives a frame, a list a list
    acct, acts = env.save_asset_memory(3), env.save_action_memory([3, 70])
    assert acct[0].columns.tolist() == ["date", "daily_return"] and len(acts) == 2
    n = int(hist.length[3])
    np.testing.assert_array_equal(acct[0]["daily_return"].to_numpy(), hist.ret[:n, 3].cpu().numpy())
    assert hist.save_action_memory(70).equals(acts[1]) and acts[1].index.name == "date"


# ------------------------------------------------------------------------------------------------
# 3. capacity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_weights", [True, False])
def test_capacity_shorter_than_the_episode(with_weights):
    """A caller-owned history (through the C ABI, as a foreign binding would attach it) whose capacity is
    shorter than the episode, each tensor followed by sentinel rows: the entries below the capacity equal
    those of a full-size history, COMPLETE | OVERFLOW at the end, the sentinels are intact; attached but
    unarmed records nothing."""
    _need_gpu()
    from finrl_amd import _native as nat
    E, T, N, K, cap, pad = 130, 14, 30, 2, 6, 3
    close, cov, tech = _random_panel(8, T, N, K)
    full_env = _env(close, cov, tech, E, auto_reset=False)
    full = full_env.enable_history(weights=with_weights)
    env = _env(close, cov, tech, E, auto_reset=False)
    SENT_F, SENT_I = -12345.5, -777
    value = torch.full((cap + pad, E), SENT_F, dtype=torch.float64, device="cuda")
    ret = torch.full((cap + pad, E), SENT_F, dtype=torch.float64, device="cuda")
    row = torch.full((cap + pad, E), SENT_I, dtype=torch.int32, device="cuda")
    weights = torch.full((cap + pad, E, N), SENT_F, dtype=torch.float32, device="cuda")
    length = torch.zeros(E + 64, dtype=torch.int32, device="cuda")
    flags = torch.zeros(E + 64, dtype=torch.int32, device="cuda")
    length[E:] = SENT_I
    flags[E:] = SENT_I
    ptrs = nat.PortfolioHistoryPtrs(value.data_ptr(), ret.data_ptr(), row.data_ptr(),
                                    weights.data_ptr() if with_weights else None,
                                    length.data_ptr(), flags.data_ptr(), cap)
    env._call("set_history", C.byref(ptrs))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    a0 = torch.rand(E, N, generator=gen, device="cuda")
    env.step(a0)                                  # attached, not armed: nothing is recorded
    full_env.step(a0)
    assert int(length[:E].abs().sum()) == 0 and bool((value == SENT_F).all()) and bool((row == SENT_I).all())
    assert bool((ret == SENT_F).all()) and bool((weights == SENT_F).all())
    env.reset()                                   # arms
    full_env.reset()
    for s in range(T - 1):
        a = torch.rand(E, N, generator=gen, device="cuda")
        env.step(a)
        full_env.step(a)
        want = OVERFLOW if s + 1 >= cap else 0
        if s in (cap - 2, cap - 1, cap):
            assert bool((flags[:E] == want).all()), s
    _, _, done, _ = env.step(a0)
    full_env.step(a0)
    assert bool(done.all())
    assert bool((full.length == T).all()) and bool((full.flags == COMPLETE).all())
    assert bool((length[:E] == cap).all()) and bool((flags[:E] == (COMPLETE | OVERFLOW)).all())
    for mine, theirs, sent in ((value, full.value, SENT_F), (ret, full.ret, SENT_F), (row, full.row, SENT_I)):
        assert torch.equal(mine[:cap], theirs[:cap]) and bool((mine[cap:] == sent).all())
    assert bool((length[E:] == SENT_I).all()) and bool((flags[E:] == SENT_I).all())
    if with_weights:
        assert torch.equal(weights[:cap], full.weights[:cap]) and bool((weights[cap:] == SENT_F).all())
    else:
        assert bool((weights == SENT_F).all()) and full.weights is None
    env._call("set_history", None)                # detach before the tensors go away


# ------------------------------------------------------------------------------------------------
# 4. a weights tensor past 4 GiB
# ------------------------------------------------------------------------------------------------
def test_weights_tensor_larger_than_4_gib():
    """65,536 envs x 30 tickers x 601 entries of f32 weights = 4.7 GB: the entries of the last recorded
    steps (offsets past 2^32 bytes), sampled over envs including block borders, equal env.weights /
    state["value"] cloned at those steps."""
    _need_gpu()
    E, N, K, cap = 65536, 30, 1, 600
    need = cap * E * (N * 4 + 20) + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, the device reports {free / 2**30:.1f}")
    close, cov, tech = _random_panel(4, cap + 1, N, K)
    env = _env(close, cov, tech, E)
    env.enable_weights()
    hist = env.enable_history()
    assert hist.capacity == cap + 1 and hist.weights.numel() * 4 > 2 ** 32
    env.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    pool = [torch.rand(E, N, generator=gen, device="cuda") for _ in range(5)]
    sample = torch.tensor([0, 1, 63, 64, 65, 127, 128, 4095, 4096, E // 2 - 1, E // 2, E - 65, E - 64, E - 1],
                          device="cuda")
    kept = {}
    for s in range(cap):
        env.step(pool[s % 5])
        if s >= cap - 4:
            kept[s + 1] = (env.weights[sample].clone(), env.state["value"][sample].clone())
    assert bool((hist.length == cap + 1).all()) and not bool(hist.flags.any())
    for k, (w, v) in kept.items():
        assert k * E * N * 4 > 2 ** 32
        assert torch.equal(hist.weights[k][sample], w), k
        assert torch.equal(hist.value[k][sample], v), k
    assert bool((hist.row[cap] == cap).all())


# ------------------------------------------------------------------------------------------------
# 5. inside a captured graph
# ------------------------------------------------------------------------------------------------
def test_history_in_a_captured_graph_equals_eager():
    _need_gpu()
    E, T, N, K, n_steps = 2048 + 70, 20, 30, 8, 8
    close, cov, tech = _random_panel(3, T, N, K)
    envs = [_env(close, cov, tech, E) for _ in range(2)]
    hists = [e.enable_history() for e in envs]            # attached before the capture
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    acts = [torch.rand(E, N, generator=gen, device="cuda") for _ in range(n_steps)]
    for e in envs:
        e.reset()
    eager, graphed = envs
    state0 = {k: v.clone() for k, v in graphed.state.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm up on a side stream
        for a in acts[:2]:
            graphed.step(a)
    torch.cuda.current_stream().wait_stream(side)
    for k, v in graphed.state.items():
        v.copy_(state0[k])
    hists[1].arm()
    hists[1].weights[1:].zero_()                          # entries past the length: make them comparable
    for k in ("value", "ret", "row"):
        getattr(hists[1], k)[1:].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for a in acts:
            graphed.step(a)
    for rep in range(3):                                  # 24 steps: across the episode end at 19
        for a in acts:
            eager.step(a)
        g.replay()
        for k in KEYS:
            assert torch.equal(getattr(hists[0], k), getattr(hists[1], k)), (rep, k)
        for k in eager.state:
            assert torch.equal(eager.state[k], graphed.state[k]), (rep, k)
        assert torch.equal(eager.obs, graphed.obs)
        assert int(hists[0].length[0]) == min(1 + n_steps * (rep + 1), T)
    assert bool(hists[1].complete.all())


# ------------------------------------------------------------------------------------------------
# 6. non-interference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("windows", [False, True])
@pytest.mark.parametrize("N", [30, 64])
def test_history_does_not_change_the_env(N, windows):
    """The same seeded run with and without a history: bit-identical obs, reward, done, weights, state,
    last-episode block and last_episode_stats(), masked reset included."""
    _need_gpu()
    E, T, K = 333, 11, 3
    close, cov, tech = _random_panel(2, T, N, K)
    kw = {}
    if windows:
        rng = np.random.default_rng(N)
        length = rng.integers(1, T + 1, E)
        s = (rng.random(E) * (T - length + 1)).astype(np.int64)
        kw["windows"] = (s, s + length)
    envs = [_env(close, cov, tech, E, initial_amount=250_000, **kw) for _ in range(2)]
    for e in envs:
        e.enable_last_episode()
        e.enable_weights()
        e.enable_terminal_obs()
    envs[1].enable_history()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(N)
    assert torch.equal(envs[0].reset(), envs[1].reset())
    for s_ in range(3 * T):
        a = torch.rand(E, N, generator=gen, device="cuda")
        outs = [e.step(a) for e in envs]
        for x, y in zip(outs[0][:3], outs[1][:3]):
            assert torch.equal(x, y), s_
        assert torch.equal(envs[0].weights, envs[1].weights)
        assert torch.equal(envs[0].term_obs, envs[1].term_obs)
        if s_ == T + 2:
            m = (torch.rand(E, generator=gen, device="cuda") < 0.3).to(torch.uint8)
            assert torch.equal(envs[0].reset(m), envs[1].reset(m))
    for k in envs[0].state:
        assert torch.equal(envs[0].state[k], envs[1].state[k]), k
    assert torch.equal(torch.nan_to_num(envs[0]._last, nan=-1.0), torch.nan_to_num(envs[1]._last, nan=-1.0))
    assert torch.equal(torch.nan_to_num(envs[0].last_episode_stats(), nan=-1.0),
                       torch.nan_to_num(envs[1].last_episode_stats(), nan=-1.0))
    assert int(envs[1].history.length.min()) >= 1


# ------------------------------------------------------------------------------------------------
# 7. metrics
# ------------------------------------------------------------------------------------------------
def test_metrics_against_pandas_and_the_last_episode_block():
    """metrics() against pandas on the recorded series copied to the host: n_returns, cumulative_return
    and max_drawdown exactly; mean / std / Sharpe within rtol 1e-9, atol 1e-12.  Windows of 2 .. 30 rows;
    rows [40, 60) of the panel have constant closes, and envs 0 .. 19 run windows inside them (every
    return exactly 0: std == 0); envs 20 .. 29 are armed right before their terminal step (length 1: NaN
    std and Sharpe); some envs are unarmed.  metrics(252 ** 0.5)'s Sharpe against
    last_episode_stats()."""
    _need_gpu()
    import pandas as pd
    E, T, N, K = 300, 60, 30, 2
    close, cov, tech = _random_panel(21, T, N, K)
    close[40:] = close[40]
    rng = np.random.default_rng(3)
    length = rng.integers(2, 31, E)
    length[30:34] = (2, 3, 30, 30)
    s = (rng.random(E) * (40 - length + 1)).astype(np.int64)
    length[:20] = 3 + np.arange(20) % 15
    s[:20] = 40 + np.arange(20) % 3
    env = _env(close, cov, tech, E, windows=(s, s + length), initial_amount=500_000, auto_reset=False)
    env.enable_last_episode()
    hist = env.enable_history(weights=False)
    assert hist.weights is None and hist.capacity == 30
    env.reset()
    late = np.zeros(E, bool)
    late[20:30] = True
    for i in range(33):
        # arm right before the terminal step: the env stands on its window's last row
        at_end = late & (env.state["day"].cpu().numpy() == s + length - 1) & ~hist.complete.cpu().numpy()
        if at_end.any():
            hist.arm(at_end)
        env.step(torch.from_numpy(rng.uniform(0, 1, (E, N)).astype(np.float32)).cuda())
    assert bool(hist.complete.all())
    unarmed = np.arange(E) % 50 == 37
    hist.length[torch.from_numpy(unarmed).cuda()] = 0
    h = _host(hist)
    assert (h["length"][20:30] == 1).all()
    from finrl_amd.history import PORTFOLIO_METRIC_KEYS
    assert PORTFOLIO_METRIC_KEYS == ("n_returns", "cumulative_return", "mean", "std", "sharpe", "max_drawdown")
    for ann in (252 ** 0.5, 4 ** 0.5):
        m = hist.metrics(ann).cpu().numpy()
        assert m.shape == (E, 6)
        worst = 0.0
        for e in range(E):
            n = h["length"][e]
            if n == 0:
                assert np.isnan(m[e]).all(), e
                continue
            val, r = pd.Series(h["value"][:n, e]), pd.Series(h["ret"][:n, e])
            assert m[e, 0] == n
            assert m[e, 1] == val.iloc[-1] / val.iloc[0] - 1, e
            assert m[e, 5] == (val / val.cummax() - 1).min(), e
            np.testing.assert_allclose(m[e, 2], r.mean(), rtol=1e-9, atol=1e-12, err_msg=f"mean {e}")
            std = r.std()
            np.testing.assert_allclose(m[e, 3], std, rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=f"std {e}")
            if n < 2 or std == 0:
                assert np.isnan(m[e, 4]), e
            else:
                ref = ann * r.mean() / std
                np.testing.assert_allclose(m[e, 4], ref, rtol=1e-9, atol=1e-12, err_msg=f"sharpe {e}")
                worst = max(worst, abs(m[e, 4] - ref) / abs(ref))
        print(f"annualization {ann:.4f}: worst relative Sharpe difference to pandas {worst:.3g}")
    assert np.isnan(m[20:30, 3]).all() and np.isnan(m[20:30, 4]).all() and (m[20:30, 0] == 1).all()
    flat = np.zeros(E, bool)
    flat[:20] = True
    assert flat.sum() >= 10 and (h["ret"][:3, flat] == 0).all()
    assert (m[flat, 3] == 0).all() and np.isnan(m[flat, 4]).all()
    # the terminal printout's Sharpe, by two routes (records that hold the whole episode)
    m = hist.metrics(252 ** 0.5).cpu().numpy()
    last = env.last_episode_stats().cpu().numpy()
    ok = ~unarmed & ~late
    np.testing.assert_allclose(m[ok, 4], last[ok, 2], rtol=1e-9, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(m[ok, 0], env.last_episode["ret_n"].cpu().numpy()[ok])
    end = h["value"][h["length"][ok] - 1, np.nonzero(ok)[0]]
    np.testing.assert_array_equal(end, env.last_episode["end_value"].cpu().numpy()[ok])


# ------------------------------------------------------------------------------------------------
# 8. the unmodified reference: DRL_prediction's loop on 130 replicas
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dow30", "n5", "n2k1", "const"])
def test_drl_prediction_loop_equals_the_reference(name):
    """tests/golden/harness_portfolio_<name>.npz: the reference env's four memories on the second-to-last
    day of DRL_prediction, the two frames it returned and the terminal printout.  The same loop on 130
    replicas (two waves and a partial one): lengths, flags, rows and dates exactly; weights and value
    rtol 1e-6 (the bounds of test_gpu_portfolio_parity.py: the softmax is f32 expf against NumPy's);
    ret[0] == 0 and the frame's first action row == 1 / N exactly; ret[k] within
    1e-6 * max_i |gross_ret[row-1, i]| (a relative weight error of 1e-6 on weights that sum to one moves
    sum(g_i w_i) by at most that).  The terminal Sharpe against the reference's printed figure is
    printed, not asserted."""
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    z = np.load(os.path.join(HERE, "golden", f"harness_portfolio_{name}.npz"), allow_pickle=False)
    T, N, K = z["cfg_int"].tolist()
    panel = PortfolioPanel(z["close"], z["cov"], z["tech"], dates=z["dates"].tolist(),
                           tickers=z["tickers"].tolist())
    E = 130
    env = VecStockPortfolioEnv(panel, E, initial_amount=z["cfg_float"][0], auto_reset=False)
    hist = env.enable_history()
    assert hist.capacity == T
    env.reset()                              # get_sb_env()
    env.reset()                              # DRL_prediction's own reset
    for i in range(T):
        a = torch.from_numpy(np.broadcast_to(z["actions"][i], (E, N)).copy()).cuda()
        _, _, done, _ = env.step(a)
    assert bool(done.all()) and bool(hist.complete.all())
    h = _host(hist)
    np.testing.assert_array_equal(h["length"], np.full(E, T))
    np.testing.assert_array_equal(h["flags"], np.full(E, COMPLETE))
    np.testing.assert_array_equal(h["row"], np.broadcast_to(np.arange(T)[:, None], (T, E)))
    assert [panel.dates[r] for r in h["row"][:, E - 1]] == z["date_memory"].tolist()
    ref_w, ref_v, ref_r = z["actions_memory"], z["asset_memory"], z["portfolio_return_memory"]
    np.testing.assert_array_equal(h["ret"][0], 0.0)
    np.testing.assert_array_equal(h["value"][0], ref_v[0])
    np.testing.assert_array_equal(h["weights"][0], np.float32(1 / N))
    np.testing.assert_allclose(h["weights"][1:], np.broadcast_to(ref_w[1:, None, :], (T - 1, E, N)), rtol=1e-6)
    np.testing.assert_allclose(h["value"], np.broadcast_to(ref_v[:, None], (T, E)), rtol=1e-6)
    gross = panel.gross_returns()
    worst_w = np.abs(h["weights"][1:] / ref_w[1:, None, :] - 1).max()
    worst_v = np.abs(h["value"] / ref_v[:, None] - 1).max()
    worst_r = 0.0
    for k in range(1, T):
        bound = 1e-6 * np.abs(gross[k - 1]).max()
        np.testing.assert_allclose(h["ret"][k], ref_r[k], rtol=0, atol=bound, err_msg=f"ret[{k}]")
        if bound > 0:
            worst_r = max(worst_r, np.abs(h["ret"][k] - ref_r[k]).max() / bound)
    print(f"{name}: worst relative difference weights {worst_w:.3g}, value {worst_v:.3g}; "
          f"worst |ret - ref| / bound {worst_r:.3g}")
    accts, acts = env.save_asset_memory(), env.save_action_memory()
    assert len(accts) == len(acts) == E
    for e in (0, 63, 64, 127, 128, E - 1):
        acct, act = accts[e], acts[e]
        assert acct.columns.tolist() == z["account_columns"].tolist()
        assert acct["date"].tolist() == z["account_date"].tolist()
        assert [str(t) for t in acct.dtypes] == z["account_dtypes"].tolist()
        np.testing.assert_array_equal(acct["daily_return"].to_numpy(), h["ret"][:, e])
        assert act.columns.tolist() == z["action_columns"].tolist()
        assert act.index.tolist() == z["action_index"].tolist()
        assert str(act.index.name) == str(z["action_index_name"])
        assert [str(t) for t in act.dtypes] == z["action_dtypes"].tolist()
        assert (act.to_numpy()[0] == 1 / N).all() and (z["action_values"][0] == 1 / N).all()
        np.testing.assert_allclose(act.to_numpy(), z["action_values"], rtol=1e-6)
    one = hist.save_asset_memory(E - 1)                  # a single index: a frame, not a list
    assert one.equals(accts[E - 1]) and env.save_asset_memory(3)[0].equals(accts[3])
    assert hist.save_action_memory(64).equals(acts[64])
    # the terminal Sharpe
    sharpe = hist.metrics(252 ** 0.5)[:, 4].cpu().numpy()
    printed = [ln for ln in z["printout"].tolist() if "Sharpe" in ln]
    if name == "const":
        assert (h["ret"] == 0).all() and np.isnan(sharpe).all() and not printed
    else:
        ref = float(printed[0].split(":")[1])
        print(f"{name}: terminal Sharpe {sharpe[0]!r}, reference prints {ref!r}, "
              f"relative difference {np.abs(sharpe / ref - 1).max():.3g}")
