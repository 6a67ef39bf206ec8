"""Per-env episode windows of the batched portfolio env (VecStockPortfolioEnv(windows=...),
finenv_portfolio_set_windows) on the MI355X: env e on panel rows [s_e, t_e) must equal the reference
env built on data_split(df, dates[s_e], dates[t_e]).  Checked against the committed reference fixtures
embedded twice in a NaN-padded panel, against an unwindowed env on each window's slice of the panel
(bit for bit), and against the CPU oracle on each slice (the tolerances of
test_gpu_portfolio_parity.py)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[len("portfolio_"):-4]
               for p in glob.glob(os.path.join(GOLDEN, "portfolio_*.npz")))
NAMES.remove("domain")      # NaN / inf values: checked with derived bounds by the *_portfolio_domain tests


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _random_panel(seed, T, N, K):
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    cov = rng.normal(0, 1e-4, (T, N, N))
    tech = rng.normal(0, 1, (T, K, N))
    return close, cov, tech


def _draw_windows(rng, E, T):
    length = rng.integers(1, T + 1, E)
    start = (rng.random(E) * (T - length + 1)).astype(np.int64)
    # the edges: lengths 1, 2 and T, windows touching row 0 and row T
    fixed = [(0, 1), (T - 2, T), (0, T), (T - 1, T), (0, 2), (T // 2, T // 2 + 1), (1, T)]
    for e, (a, b) in enumerate(fixed[:E]):
        start[e], length[e] = a, b - a
    return start, start + length


def _act(rng, E, N):
    return torch.from_numpy(rng.uniform(0, 1, (E, N)).astype(np.float32)).cuda()


# ------------------------------------------------------------------------------------------------
# 1. the reference fixtures as windows of a longer panel
# ------------------------------------------------------------------------------------------------
def _embed_twice(z, pre=3, gap=2, post=3):
    """The fixture's panel twice, with NaN days before, between and after: a kernel that reads a row
    outside an env's window carries a NaN into its value, reward or observation."""
    T, N, K, _ = z["cfg_int"].tolist()
    TT = pre + T + gap + T + post
    close = np.full((TT, N), np.nan)
    cov = np.full((TT, N, N), np.nan)
    tech = np.full((TT, K, N), np.nan)
    starts = (pre, pre + T + gap)
    for s in starts:
        close[s:s + T], cov[s:s + T], tech[s:s + T] = z["close"], z["cov"], z["tech"].reshape(T, K, N)
    return close, cov, tech, starts


@pytest.mark.parametrize("auto", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_fixture_as_embedded_windows(name, auto):
    """70 envs alternating between the fixture's two copies; the fixture's actions and reset schedule
    (gym semantics), or the same run with the resets done by the step kernel (auto_reset)."""
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    z = np.load(os.path.join(GOLDEN, f"portfolio_{name}.npz"), allow_pickle=False)
    T, N, K, S = z["cfg_int"].tolist()
    E = 70
    close, cov, tech, starts = _embed_twice(z)
    s = np.array([starts[e % 2] for e in range(E)])
    env = VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, initial_amount=z["cfg_float"][0],
                               auto_reset=auto, windows=(s, s + T))
    env.enable_weights()
    env.enable_terminal_obs()
    env.enable_last_episode()
    assert env.max_step == T - 1
    resets = dict(zip(z["reset_step"].tolist(), z["reset_obs"]))
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(obs, np.broadcast_to(resets[-1].astype(np.float32), obs.shape))
    nd = 0
    for k in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][k], (E, N)).copy()).cuda()
        obs, rew, done, _ = env.step(a)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        st = env.state_numpy()
        msg = f"{name} auto={auto} step {k}"
        d = bool(z["done"][k])
        np.testing.assert_array_equal(done.astype(bool), np.full(E, d), err_msg=msg)
        np.testing.assert_allclose(rew, np.float32(z["reward"][k]), rtol=1e-6, err_msg=msg)
        assert np.isfinite(obs).all() and np.isfinite(rew).all() and np.isfinite(st["value"]).all(), msg
        assert np.isfinite(env.weights.cpu().numpy()).all(), msg
        if d and auto:          # the step kernel already reset: day 0 of the window, the reset row
            np.testing.assert_array_equal(st["window_day"], 0, err_msg=msg)
            np.testing.assert_array_equal(st["day"], s, err_msg=msg)
            assert (st["value"] == z["cfg_float"][0]).all(), msg
            np.testing.assert_array_equal(obs, np.broadcast_to(resets[k].astype(np.float32), obs.shape),
                                          err_msg=msg)
            np.testing.assert_array_equal(env.term_obs.cpu().numpy(),
                                          np.broadcast_to(z["obs"][k].astype(np.float32), obs.shape),
                                          err_msg=msg)
        else:
            np.testing.assert_array_equal(st["window_day"], z["day"][k], err_msg=msg)
            np.testing.assert_array_equal(st["day"], s + z["day"][k], err_msg=msg)
            np.testing.assert_allclose(st["value"], z["value"][k], rtol=1e-6, err_msg=msg)
            np.testing.assert_array_equal(obs, np.broadcast_to(z["obs"][k].astype(np.float32), obs.shape),
                                          err_msg=msg)
        if not d:
            np.testing.assert_allclose(env.weights.cpu().numpy(),
                                       np.broadcast_to(z["weights"][k], (E, N)), rtol=1e-6, err_msg=msg)
        if d:
            nd += 1
            le = env.last_episode
            np.testing.assert_array_equal(le["count"].cpu().numpy(), nd, err_msg=msg)
            np.testing.assert_array_equal(le["ret_n"].cpu().numpy(), z["day"][k] + 1, err_msg=msg)
            np.testing.assert_allclose(le["end_value"].cpu().numpy(), z["value"][k], rtol=1e-6, err_msg=msg)
            if not auto:
                obs = env.reset().cpu().numpy()
                np.testing.assert_array_equal(obs, np.broadcast_to(resets[k].astype(np.float32), obs.shape),
                                              err_msg=msg)
                np.testing.assert_array_equal(env.state_numpy()["day"], s)
    assert nd == 2


# ------------------------------------------------------------------------------------------------
# 2. random windows against an unwindowed env on each window's slice (bit for bit) and the oracle
# ------------------------------------------------------------------------------------------------
class _SliceTwins:
    """One unwindowed VecStockPortfolioEnv per distinct window (s, t), on PortfolioPanel(close[s:t],
    cov[s:t], tech[s:t]), holding every env of the batch on that window."""

    def __init__(self, close, cov, tech, s, t, initial_amount, auto):
        from finrl_amd.panel import PortfolioPanel
        from finrl_amd.vec_portfolio import VecStockPortfolioEnv
        self.E = len(s)
        self.groups = []
        for a, b in sorted(set(zip(s.tolist(), t.tolist()))):
            idx = np.nonzero((s == a) & (t == b))[0]
            env = VecStockPortfolioEnv(PortfolioPanel(close[a:b], cov[a:b], tech[a:b]), len(idx),
                                       initial_amount=initial_amount, auto_reset=auto)
            env.enable_terminal_obs()
            env.enable_weights()
            env.enable_last_episode()
            self.groups.append((torch.from_numpy(idx).cuda(), env))

    def _gather(self, fn, like):
        out = torch.empty((self.E,) + tuple(like.shape[1:]), dtype=like.dtype, device="cuda")
        for idx, env in self.groups:
            out[idx] = fn(env)
        return out

    def reset(self, mask=None):
        for idx, env in self.groups:
            env.reset(None if mask is None else mask[idx])

    def step(self, actions):
        for idx, env in self.groups:
            env.step(actions[idx].contiguous())

    def outputs(self, ref):
        """The same tensors as `outputs(ref)` of the windowed env, gathered into batch order."""
        like = _outputs(ref)
        g = lambda name, fn: self._gather(fn, like[name])  # noqa: E731
        return dict(obs=g("obs", lambda e: e.obs), reward=g("reward", lambda e: e.reward),
                    done=g("done", lambda e: e.done), value=g("value", lambda e: e.state["value"]),
                    last_reward=g("last_reward", lambda e: e.state["last_reward"]),
                    window_day=g("window_day", lambda e: e.state["day"]),
                    term_obs=g("term_obs", lambda e: e.term_obs), weights=g("weights", lambda e: e.weights),
                    last=g("last", lambda e: e.enable_last_episode().T.contiguous()),
                    last_stats=g("last_stats", lambda e: e.last_episode_stats()))


def _outputs(env):
    return dict(obs=env.obs, reward=env.reward, done=env.done, value=env.state["value"],
                last_reward=env.state["last_reward"], window_day=env.window_day(), term_obs=env.term_obs,
                weights=env.weights, last=env.enable_last_episode().T.contiguous(),
                last_stats=env.last_episode_stats())


def _assert_same(got, ref, msg):
    for k in ref:
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg=f"{k} {msg}")


@pytest.mark.parametrize("N,K,E,T,auto", [(1, 1, 70, 9, True), (7, 3, 130, 12, False),
                                          (30, 8, 70, 14, True), (30, 8, 100, 11, False),
                                          (64, 2, 65, 9, True)])
def test_random_windows_equal_slice_twins_and_oracle(N, K, E, T, auto):
    """Random windows (lengths 1, 2 and T, windows on row 0 and row T), two or more episode ends per
    env: obs, reward, done, value, term_obs, weights and the last-episode block equal an unwindowed env
    on each slice bit for bit; the CPU oracle on each slice agrees within the parity tolerances."""
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    from oracle.portfolio import PortfolioOracle
    rng = np.random.default_rng(100 * N + E + T)
    close, cov, tech = _random_panel(N + 3 * E, T, N, K)
    s, t = _draw_windows(rng, E, T)
    env = VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, initial_amount=1e6, auto_reset=auto,
                               windows=(s, t))
    env.enable_terminal_obs()
    env.enable_weights()
    env.enable_last_episode()
    assert env.max_step == int((t - s).max()) - 1
    twins = _SliceTwins(close, cov, tech, s, t, 1e6, auto)
    orc = [PortfolioOracle(close[a:b], cov[a:b], tech[a:b], n_envs=1, initial_amount=1e6)
           for a, b in zip(s, t)]
    o0 = np.concatenate([o.reset() for o in orc])
    twins.reset()
    np.testing.assert_array_equal(env.reset().cpu().numpy(), o0.astype(np.float32))
    _assert_same(_outputs(env), twins.outputs(env), "reset")
    ends = np.zeros(E, dtype=np.int64)
    pending = np.zeros(E, dtype=bool)
    for k in range(2 * T + 2):
        msg = f"step {k}"
        if not auto and pending.any():          # the caller resets the envs that reported done
            m = torch.from_numpy(pending.astype(np.uint8)).cuda()
            env.reset(m)
            twins.reset(m)
            for e in np.nonzero(pending)[0]:
                orc[e].reset()
            pending[:] = False
            _assert_same(_outputs(env), twins.outputs(env), f"reset {msg}")
        a = _act(rng, E, N)
        env.step(a)
        twins.step(a)
        _assert_same(_outputs(env), twins.outputs(env), msg)
        a_np = a.cpu().numpy()
        o = [x.vec_step(a_np[e:e + 1], auto_reset=auto) for e, x in enumerate(orc)]
        o_done = np.array([r[2][0] for r in o])
        np.testing.assert_array_equal(env.done.cpu().numpy().astype(bool), o_done, err_msg=msg)
        np.testing.assert_array_equal(env.obs.cpu().numpy(),
                                      np.concatenate([r[0] for r in o]).astype(np.float32), err_msg=msg)
        np.testing.assert_allclose(env.reward.cpu().numpy(), np.concatenate([r[1] for r in o]), rtol=1e-6,
                                   err_msg=msg)
        st = env.state_numpy()
        np.testing.assert_array_equal(st["window_day"], [x.state()["day"][0] for x in orc], err_msg=msg)
        np.testing.assert_allclose(st["value"], [x.state()["value"][0] for x in orc], rtol=1e-6, err_msg=msg)
        assert ((st["day"] >= s) & (st["day"] < t)).all(), msg
        if auto and o_done.any():
            np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done],
                                          np.concatenate([r[3] for r in o])[o_done].astype(np.float32))
        ends += o_done
        pending |= o_done
    assert (ends >= 2).all(), ends.min()


# ------------------------------------------------------------------------------------------------
# 3. windows [0, T) change nothing; detaching restores the no-window kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,auto", [(30, 8, True), (7, 2, False), (5, 0, True)])
def test_full_panel_windows_equal_the_unwindowed_env(N, K, auto):
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    E, T = 200, 9
    close, cov, tech = _random_panel(N * 3 + K, T, N, K)
    rng = np.random.default_rng(N)
    panel = PortfolioPanel(close, cov, tech)
    ref = VecStockPortfolioEnv(panel, E, auto_reset=auto)
    win = VecStockPortfolioEnv(panel, E, auto_reset=auto, windows=(0, T))
    for env in (ref, win):
        env.enable_terminal_obs()
        env.enable_weights()
        env.enable_last_episode()
        env.reset()
    assert win.max_step == ref.max_step == T - 1
    for k in range(3 * T):
        if k == 2 * T:
            win.set_windows(None)
            assert win.windows is None
        if k in (4, 11) or (not auto and k % T == 0):
            m = torch.from_numpy((rng.random(E) < 0.4).astype(np.uint8)).cuda()
            if not auto:
                m |= ref.done
            np.testing.assert_array_equal(win.reset(m).cpu().numpy(), ref.reset(m).cpu().numpy())
        a = _act(rng, E, N)
        ref.step(a)
        win.step(a)
        _assert_same(_outputs(win), _outputs(ref), f"step {k}")
        np.testing.assert_array_equal(win.state_numpy()["day"], ref.state_numpy()["day"])


# ------------------------------------------------------------------------------------------------
# 4. edits of the window block, eagerly and between graph replays
# ------------------------------------------------------------------------------------------------
def test_window_edits_apply_at_the_documented_points():
    """An edited end applies from the next step; an edited start only at the env's next reset."""
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    E, T, N, K = 70, 24, 30, 4
    close, cov, tech = _random_panel(5, T, N, K)
    rng = np.random.default_rng(5)
    env = VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, windows=(2, 20))
    env.enable_last_episode()
    env.reset()
    for _ in range(3):
        env.step(_act(rng, E, N))
    assert (env.state_numpy()["day"] == 5).all()
    s_new, t_new = np.full(E, 2), np.full(E, 20)
    t_new[::2] = 8                       # new end: terminal at day 7
    env.set_windows(torch.from_numpy(s_new).cuda(), torch.from_numpy(t_new).cuda())
    assert env.max_step == 17
    env.step(_act(rng, E, N))
    env.step(_act(rng, E, N))
    assert (env.state_numpy()["day"] == 7).all()
    _, _, done, _ = env.step(_act(rng, E, N))
    done = done.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(done, t_new == 8)
    st = env.state_numpy()
    np.testing.assert_array_equal(st["day"][done], 2)           # auto-reset to the start
    np.testing.assert_array_equal(st["day"][~done], 8)
    np.testing.assert_array_equal(env.last_episode["ret_n"].cpu().numpy()[done], 6)   # days 2..7 + the 0
    # a new start, set for the envs that just finished, applies at their next reset
    s_new[done] = 10
    t_new[done] = 14
    env.set_windows(s_new, t_new, mask=done)
    np.testing.assert_array_equal(env.state_numpy()["day"][done], 2)       # nobody moved
    env.reset(torch.from_numpy(done.astype(np.uint8)).cuda())
    st = env.state_numpy()
    np.testing.assert_array_equal(st["day"][done], 10)
    np.testing.assert_array_equal(st["window_day"][done], 0)
    np.testing.assert_array_equal(st["day"][~done], 8)
    for _ in range(4):
        _, _, d, _ = env.step(_act(rng, E, N))
    np.testing.assert_array_equal(d.cpu().numpy().astype(bool), done)      # rows 10..13: terminal at 13
    np.testing.assert_array_equal(env.last_episode["ret_n"].cpu().numpy()[done], 4)
    np.testing.assert_array_equal(env.last_episode["count"].cpu().numpy()[done], 2)


@pytest.mark.parametrize("auto", [True, False])
def test_masked_set_windows_then_reset_recipe(auto):
    """set_windows(s, t, mask=done) + reset(done) after every step: each episode equals an unwindowed
    env on its slice, and the latch holds that episode's summary (count, ret_n, sums, Sharpe)."""
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    E, T, N, K = 67, 20, 7, 2
    close, cov, tech = _random_panel(9, T, N, K)
    rng = np.random.default_rng(9)
    s, t = _draw_windows(rng, E, T)
    env = VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, auto_reset=auto, windows=(s, t))
    env.enable_last_episode()
    env.reset()
    cur = [(int(a), int(b)) for a, b in zip(s, t)]
    hist = [[] for _ in range(E)]        # actions of each env's episode in progress
    checked = 0
    for k in range(3 * T):
        a = _act(rng, E, N)
        _, _, done, _ = env.step(a)
        a_np = a.cpu().numpy()
        d = done.cpu().numpy().astype(bool)
        for e in range(E):
            hist[e].append(a_np[e])
        last = env.enable_last_episode().cpu().numpy()
        stats = env.last_episode_stats().cpu().numpy()
        for e in np.nonzero(d)[0]:       # replay the finished episode on a slice twin
            a0, b0 = cur[e]
            tw = VecStockPortfolioEnv(PortfolioPanel(close[a0:b0], cov[a0:b0], tech[a0:b0]), 1,
                                      auto_reset=False)
            tw.enable_last_episode()
            tw.reset()
            for x in hist[e]:
                tw.step(torch.from_numpy(x[None]).cuda())
            assert bool(tw.done[0]), (k, e)
            # begin / end value, ret_n and the return sums (COUNT counts this env's episodes)
            np.testing.assert_array_equal(tw.enable_last_episode().cpu().numpy()[1:6, 0], last[1:6, e])
            np.testing.assert_array_equal(tw.last_episode_stats().cpu().numpy()[0], stats[e])
            hist[e] = []
            checked += 1
        ns, nt = _draw_windows(rng, E, T)
        ns, nt = ns[rng.permutation(E)], nt[rng.permutation(E)]
        ok = nt > ns
        ns, nt = np.where(ok, ns, 0), np.where(ok, nt, T)
        env.set_windows(ns, nt, mask=d)
        env.reset(done)
        for e in np.nonzero(d)[0]:
            cur[e] = (int(ns[e]), int(nt[e]))
        st = env.state_numpy()
        np.testing.assert_array_equal(st["day"][d], ns[d])
        np.testing.assert_array_equal(st["window_day"][d], 0)
    assert checked >= E


def test_graph_replay_sees_edited_windows():
    """A captured step + masked set_windows + reset(done), replayed with the window pool and the
    window block edited between replays, equals the same calls run eagerly."""
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    E, T, N, K = 130, 16, 30, 8
    close, cov, tech = _random_panel(11, T, N, K)
    panel = PortfolioPanel(close, cov, tech)
    rng = np.random.default_rng(3)
    s0, t0 = _draw_windows(rng, E, T)
    mk = lambda: VecStockPortfolioEnv(panel, E, windows=(s0, t0))  # noqa: E731
    cap, eager = mk(), mk()
    for env in (cap, eager):
        env.enable_terminal_obs()
        env.enable_weights()
        env.enable_last_episode()
        env.reset()
    act = torch.zeros(E, N, dtype=torch.float32, device="cuda")
    pool_s = torch.zeros(E, dtype=torch.int32, device="cuda")
    pool_t = torch.full((E,), T, dtype=torch.int32, device="cuda")

    def segment(env):
        env.step(act)
        env.set_windows(pool_s, pool_t, mask=env.done)
        env.reset(env.done)

    act.copy_(_act(rng, E, N))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up on a side stream (both envs take it)
        segment(cap)
    torch.cuda.current_stream().wait_stream(side)
    segment(eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        segment(cap)
    redrawn = 0
    for rep in range(3 * T):
        act.copy_(_act(rng, E, N))
        ns, nt = _draw_windows(rng, E, T)
        pool_s.copy_(torch.from_numpy(ns[rng.permutation(E)]))
        pool_t.copy_(torch.from_numpy(nt[rng.permutation(E)]))
        bad = pool_t <= pool_s
        pool_s[bad], pool_t[bad] = 0, T
        if rep % 7 == 3:                    # an eager edit of the block itself, between replays
            m = rng.random(E) < 0.2
            e_s, e_t = np.where(m, 1, s0), np.where(m, T - 1, t0)
            for env in (cap, eager):
                env.set_windows(torch.from_numpy(e_s).cuda(), torch.from_numpy(e_t).cuda(),
                                mask=torch.from_numpy(m).cuda())
        graph.replay()
        segment(eager)
        torch.cuda.synchronize()
        _assert_same(_outputs(cap), _outputs(eager), f"replay {rep}")
        np.testing.assert_array_equal(cap.windows.cpu().numpy(), eager.windows.cpu().numpy())
        np.testing.assert_array_equal(cap.state["day"].cpu().numpy(), eager.state["day"].cpu().numpy())
        redrawn += int(cap.done.sum())
    assert redrawn > E


# ------------------------------------------------------------------------------------------------
# 5. the tutorial's train and trade slices in one batch
# ------------------------------------------------------------------------------------------------
def test_tutorial_train_and_trade_windows_in_one_batch():
    """FinRL_PortfolioAllocation_Explainable_DRL: train = data_split(df, '2009-01-01', '2020-06-30'),
    trade = data_split(df, '2020-07-01', '2021-09-02'), cov_list computed over the whole frame.  Both
    as windows of one panel equal two unwindowed envs built on the two data_split frames."""
    _need_gpu()
    import pandas as pd
    from finrl_amd.data import data_split, windows_from_dates
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    dates = list(pd.bdate_range("2020-05-01", "2020-08-14").strftime("%Y-%m-%d"))
    tics, N, tech_names = [f"T{i}" for i in range(6)], 6, ["macd", "rsi_30"]
    rng = np.random.default_rng(21)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (len(dates), N)), axis=0))
    rows = []
    for r, d in enumerate(dates):
        cov = rng.normal(0, 1e-4, (N, N))
        for i, tic in enumerate(tics):
            rows.append(dict(date=d, tic=tic, close=close[r, i], macd=rng.normal(), rsi_30=rng.normal(),
                             cov_list=cov))
    df = pd.DataFrame(rows)
    panel = PortfolioPanel.from_dataframe(data_split(df, dates[0], "9999"), tech_names)
    (s_tr, s_td), (t_tr, t_td) = windows_from_dates(panel.dates, ["2009-01-01", "2020-07-01"],
                                                    ["2020-06-30", "2021-09-02"])
    E = 130
    s = np.where(np.arange(E) % 2 == 0, s_tr, s_td)
    t = np.where(np.arange(E) % 2 == 0, t_tr, t_td)
    env = VecStockPortfolioEnv(panel, E, auto_reset=False, windows=(s, t))
    parts = [VecStockPortfolioEnv(PortfolioPanel.from_dataframe(data_split(df, a, b), tech_names), E // 2,
                                  auto_reset=False)
             for a, b in (("2009-01-01", "2020-06-30"), ("2020-07-01", "2021-09-02"))]
    assert [p.panel.T for p in parts] == [t_tr - s_tr, t_td - s_td]
    for x in [env] + parts:
        x.enable_weights()
        x.enable_last_episode()
    obs = env.reset()
    for j, p in enumerate(parts):
        np.testing.assert_array_equal(obs[j::2].cpu().numpy(), p.reset().cpu().numpy())
    for k in range(max(p.panel.T for p in parts) + 3):
        a = _act(rng, E, N)
        env.step(a)
        for j, p in enumerate(parts):
            p.step(a[j::2].contiguous())
            for key in ("obs", "reward", "done", "weights"):
                np.testing.assert_array_equal(getattr(env, key)[j::2].cpu().numpy(),
                                              getattr(p, key).cpu().numpy(), err_msg=f"{key} {j} {k}")
            np.testing.assert_array_equal(env.state["value"][j::2].cpu().numpy(), p.state["value"].cpu().numpy())
            np.testing.assert_array_equal(env.window_day()[j::2].cpu().numpy(), p.state["day"].cpu().numpy())
            np.testing.assert_array_equal(env.last_episode_stats()[j::2].cpu().numpy(),
                                          p.last_episode_stats().cpu().numpy())
    assert env.done.cpu().numpy().all()


# ------------------------------------------------------------------------------------------------
# 6. full size: bench.py --env portfolio's shape with random 63-day windows
# ------------------------------------------------------------------------------------------------
def test_full_size_random_63_day_windows():
    """65,536 envs at DOW30 x 8, random 63-day windows redrawn for the envs that finish
    (set_windows(mask=done) + reset(done)), past two episode ends per env; a sample of envs against
    slice twins bit for bit."""
    _need_gpu()
    from finrl_amd.data import random_windows
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    E, T, N, K, L = 65_536, 252, 30, 8, 63
    close, cov, tech = _random_panel(63, T, N, K)
    g = torch.Generator(device="cuda").manual_seed(63)
    s, t = random_windows(T, E, L, generator=g)
    env = VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, windows=(s, t))
    env.enable_last_episode()
    assert env.max_step == L - 1
    rng = np.random.default_rng(63)
    sample = np.unique(np.concatenate([[0, 1, 63, 64, E // 2, E - 65, E - 1], rng.integers(0, E, 25)]))
    sidx = torch.from_numpy(sample).cuda()
    win = env.windows[:, sidx].cpu().numpy()
    twins = [None] * len(sample)

    def twin(j):
        a, b = win[:, j]
        tw = VecStockPortfolioEnv(PortfolioPanel(close[a:b], cov[a:b], tech[a:b]), 1, auto_reset=False)
        tw.enable_last_episode()
        tw.reset()
        return tw

    obs = env.reset()
    for j in range(len(sample)):
        twins[j] = twin(j)
        np.testing.assert_array_equal(obs[sample[j]].cpu().numpy(), twins[j].obs[0].cpu().numpy())
    pool = [torch.from_numpy(np.random.default_rng(i).uniform(0, 1, (E, N)).astype(np.float32)).cuda()
            for i in range(4)]
    ends = torch.zeros(E, dtype=torch.int32, device="cuda")
    for k in range(2 * L + 5):
        a = pool[k % 4]
        env.step(a)
        done = env.done.bool()
        ends += done.to(torch.int32)
        o, r, d = env.obs[sidx].cpu().numpy(), env.reward[sidx].cpu().numpy(), env.done[sidx].cpu().numpy()
        v = env.state["value"][sidx].cpu().numpy()
        last = env.enable_last_episode()[:, sidx].cpu().numpy()
        a_s = a[sidx]
        for j in range(len(sample)):
            tw = twins[j]
            if bool(tw.done[0]):
                continue
            tw.step(a_s[j:j + 1].contiguous())
            assert bool(tw.done[0]) == bool(d[j]), (k, sample[j])
            assert r[j] == tw.reward[0].item(), (k, sample[j])
            if bool(d[j]):      # auto-reset: the finished episode's value is in the latch
                np.testing.assert_array_equal(last[1:6, j], tw.enable_last_episode()[1:6, 0].cpu().numpy())
            else:
                assert v[j] == tw.state["value"][0].item(), (k, sample[j])
                np.testing.assert_array_equal(o[j], tw.obs[0].cpu().numpy(), err_msg=f"step {k} env {sample[j]}")
        # new 63-day windows for the envs that finished, then their reset
        ns, nt = random_windows(T, E, L, generator=g)
        env.set_windows(ns, nt, mask=done)
        env.reset(done)
        if bool(d.any()):
            win[:, d.astype(bool)] = env.windows[:, sidx].cpu().numpy()[:, d.astype(bool)]
            for j in np.nonzero(d)[0]:
                twins[j] = twin(j)
                np.testing.assert_array_equal(env.obs[sample[j]].cpu().numpy(), twins[j].obs[0].cpu().numpy())
    st = env.state_numpy()
    w = env.windows.cpu().numpy()
    assert ((st["day"] >= w[0]) & (st["day"] < w[1])).all()
    assert int(ends.min()) >= 2
    assert torch.isfinite(env.obs).all() and torch.isfinite(env.state["value"]).all()
