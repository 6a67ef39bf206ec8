"""Per-env episode windows of the batched stock env (VecStockTradingEnv(windows=...),
finenv_stock_set_windows) on the MI355X: env e on panel rows [s_e, t_e) must equal the reference env
built on data_split(df, dates[s_e], dates[t_e]) -- the committed reference fixtures embedded twice in
a longer panel, and the CPU oracle run on each env's slice of the panel.  Every output is compared
exactly; the Sharpe column against the oracle keeps the bar of test_gpu_stock_parity.py (the oracle
evaluates it with a different summation), and exactly wherever two GPU paths are compared."""
import numpy as np
import pytest

from _golden import StockFixture, stock_fixture_names

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _random_panel(seed, T, N, K, flag_frac=0.03):
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    tech = rng.normal(0, 1, (T, K, N))
    if K:
        tech[:, 0, :][rng.random((T, N)) < flag_frac] = 1.0
    risk = np.abs(rng.normal(0, 30, T))
    return close, tech, risk


def _stats_equal(g, o, what):
    np.testing.assert_array_equal(g[..., :5], o[..., :5], err_msg=what)
    np.testing.assert_allclose(g[..., 5], o[..., 5], rtol=1e-9, atol=1e-12, equal_nan=True,
                               err_msg=what)


# ------------------------------------------------------------------------------------------------
# 1. the reference fixtures as windows of a longer panel
# ------------------------------------------------------------------------------------------------
def _embed_twice(fx, pre=3, gap=2, post=3):
    """The fixture's panel twice, with NaN days before, between and after: a kernel that reads a
    row outside an env's window carries a NaN into its cash, asset or observation."""
    T, N, K = fx.T, fx.N, fx.K
    TT = pre + T + gap + T + post
    close = np.full((TT, N), np.nan)
    tech = np.full((TT, K, N), np.nan)
    risk = np.full(TT, np.nan)
    starts = (pre, pre + T + gap)
    for s in starts:
        close[s:s + T], tech[s:s + T], risk[s:s + T] = fx.close, fx.tech.reshape(T, K, N), fx.risk
    return close, tech, risk, starts


@pytest.mark.parametrize("name", stock_fixture_names())
def test_fixture_as_embedded_windows(name):
    """130 envs alternating between the fixture's two copies (a desynchronised batch: two 64-env
    blocks and a 2-lane tail), gym semantics, the fixture's actions and reset schedule; every env
    equals the fixture at every step."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    fx = StockFixture(name)
    z = fx.z
    E = 130
    close, tech, risk, starts = _embed_twice(fx)
    s = np.array([starts[e % 2] for e in range(E)])
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, auto_reset=False,
                             windows=(s, s + fx.T), **fx.env_kwargs())
    env.enable_realised()
    env.enable_last_episode()
    resets = dict(zip(z["reset_step"].tolist(), z["reset_obs"]))
    if -1 in resets:
        obs = env.reset().cpu().numpy()
        np.testing.assert_array_equal(obs, np.broadcast_to(resets[-1].astype(np.float32), obs.shape))
    else:
        obs = env.observe().cpu().numpy()
        np.testing.assert_array_equal(obs, np.broadcast_to(z["ctor_obs"].astype(np.float32), obs.shape))
    tj = 0
    for k in range(fx.S):
        a = torch.from_numpy(np.broadcast_to(fx.actions[k], (E, fx.N)).copy()).cuda()
        obs, rew, done, _ = env.step(a)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        st = env.state_numpy()
        msg = f"{name} step {k}"
        np.testing.assert_array_equal(done.astype(bool), np.full(E, bool(z["done"][k])), err_msg=msg)
        np.testing.assert_array_equal(st["window_day"], np.full(E, z["day"][k]), err_msg=msg)
        np.testing.assert_array_equal(st["day"], s + z["day"][k], err_msg=msg)
        np.testing.assert_array_equal(st["shares"], np.broadcast_to(z["shares"][k], (E, fx.N)), err_msg=msg)
        np.testing.assert_array_equal(st["trades"], np.full(E, z["trades"][k]), err_msg=msg)
        np.testing.assert_array_equal(st["cash"], np.full(E, z["cash"][k]), err_msg=msg)
        np.testing.assert_array_equal(st["cost"], np.full(E, z["cost"][k]), err_msg=msg)
        np.testing.assert_array_equal(st["last_reward"], np.full(E, z["reward"][k]), err_msg=msg)
        np.testing.assert_array_equal(st["turbulence"], np.full(E, z["turbulence"][k]), err_msg=msg)
        np.testing.assert_array_equal(rew, np.full(E, np.float32(z["reward"][k])), err_msg=msg)
        np.testing.assert_array_equal(env.realised.cpu().numpy(),
                                      np.broadcast_to(z["realised"][k], (E, fx.N)), err_msg=msg)
        if "obs" in z.files:
            np.testing.assert_array_equal(obs, np.broadcast_to(z["obs"][k].astype(np.float32), obs.shape),
                                          err_msg=msg)
        if z["done"][k]:
            stats = env.episode_stats().cpu().numpy()
            last = env.last_episode_stats().cpu().numpy()
            np.testing.assert_array_equal(last, stats, err_msg=msg)
            am = z[f"asset_memory_{tj}"]
            assert (stats[:, 0] == am[0]).all(), msg
            assert (stats[:, 3] == z["cost"][k]).all() and (stats[:, 4] == z["trades"][k]).all(), msg
            sh = fx.sharpe(tj)
            if np.isnan(sh):
                assert np.isnan(stats[:, 5]).all(), msg
            else:
                np.testing.assert_allclose(stats[:, 5], sh, rtol=1e-9, atol=1e-12, err_msg=msg)
            tj += 1
            obs = env.reset().cpu().numpy()
            np.testing.assert_array_equal(obs, np.broadcast_to(resets[k].astype(np.float32), obs.shape),
                                          err_msg=msg)
            st = env.state_numpy()
            np.testing.assert_array_equal(st["day"], s)
            np.testing.assert_array_equal(st["start_day"], s)
    assert tj >= 2


# ------------------------------------------------------------------------------------------------
# 2. random windows against the oracle on each env's slice
# ------------------------------------------------------------------------------------------------
def _draw_windows(rng, E, T):
    length = rng.integers(1, T + 1, E)
    start = (rng.random(E) * (T - length + 1)).astype(np.int64)
    # the edges: lengths 1 and 2, windows touching day 0 and day T, the whole panel
    fixed = [(0, 1), (T - 2, T), (0, T), (T - 1, T), (0, 2), (T // 2, T // 2 + 1)]
    for e, (a, b) in enumerate(fixed[:E]):
        start[e], length[e] = a, b - a
    return start, start + length


class _SliceOracles:
    """One oracle.stock.StockOracle per env, on close[s:t], tech[s:t], risk[s:t]."""

    def __init__(self, close, tech, risk, s, t, cash0, sh0, **kw):
        from oracle.stock import StockOracle
        self.o = [StockOracle(close[a:b], tech[a:b], risk[a:b], n_envs=1, initial_amount=cash0[e],
                              num_stock_shares=sh0[e], **kw) for e, (a, b) in enumerate(zip(s, t))]

    def reset(self, idx=None):
        idx = range(len(self.o)) if idx is None else idx
        return {int(e): self.o[e].reset()[0] for e in idx}

    def stats(self):
        return np.concatenate([o.episode_stats() for o in self.o])

    def state(self):
        st = [o.state() for o in self.o]
        return {k: np.concatenate([x[k] for x in st]) for k in st[0]}


def _compare_state(env, orc, s, msg):
    st, os_ = env.state_numpy(), orc.state()
    for k in ("cash", "cost", "trades", "episode", "last_reward", "turbulence"):
        np.testing.assert_array_equal(st[k], os_[k], err_msg=f"{k} {msg}")
    np.testing.assert_array_equal(st["shares"], os_["shares"], err_msg=f"shares {msg}")
    np.testing.assert_array_equal(st["window_day"], os_["day"], err_msg=f"day {msg}")
    np.testing.assert_array_equal(st["day"], s + os_["day"], err_msg=f"day {msg}")
    np.testing.assert_array_equal(st["price_day"], s + os_["price_day"], err_msg=f"price_day {msg}")


SWEEP = [
    # N, K, E, T, auto_reset, reset_quirk, turbulence, initial, desync hint
    (1, 2, 65, 12, True, True, True, True, False),
    (7, 3, 130, 15, False, False, False, False, True),
    (30, 8, 130, 18, True, False, True, True, False),
    (30, 8, 70, 14, False, True, False, True, True),
    (33, 1, 70, 12, True, True, False, False, False),
    (64, 2, 65, 12, False, False, True, True, False),
    (65, 1, 70, 12, True, False, True, True, False),
    (100, 3, 130, 12, True, True, True, True, False),
    (100, 2, 70, 11, False, False, False, False, True),
    (128, 1, 64, 10, True, False, False, True, False),
]


@pytest.mark.parametrize("N,K,E,T,auto,quirk,turb,initial,hint", SWEEP)
def test_random_windows_match_oracle(N, K, E, T, auto, quirk, turb, initial, hint):
    """Every kernel width (32, 64, 128, the N = 100 one), random windows, per-env cash / shares,
    two or more episode ends per env, with and without auto-reset; the last-episode latch equals
    the oracle's episode_stats() just before the terminal step."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    rng = np.random.default_rng(1000 * N + E + T)
    close, tech, risk = _random_panel(N + 7 * E, T, N, K)
    s, t = _draw_windows(rng, E, T)
    cash0 = 100_000 * rng.uniform(0.5, 1.5, E)
    sh0 = rng.integers(0, 15, (E, N))
    kw = dict(hmax=100, turbulence_threshold=(40.0 if turb else None), reset_quirk=quirk,
              initial=initial)
    orc = _SliceOracles(close, tech, risk, s, t, cash0, sh0, **kw)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, windows=(s, t), initial_amount=cash0,
                             num_stock_shares=sh0, auto_reset=auto, **kw)
    env.hint_desynchronised(hint)
    env.enable_terminal_obs()
    env.enable_last_episode()
    assert env.max_step == int((t - s).max()) - 1
    o0 = orc.reset()
    g0 = env.reset().cpu().numpy()
    np.testing.assert_array_equal(g0, np.stack([o0[e] for e in range(E)]).astype(np.float32))
    ends = np.zeros(E, dtype=np.int64)
    pending = np.zeros(E, dtype=bool)          # gym semantics: envs that reported done
    for k in range(2 * T + 2):
        msg = f"step {k}"
        if not auto and pending.any():        # the caller resets the finished envs
            idx = np.nonzero(pending)[0]
            exp = env.obs.cpu().numpy().copy()
            for e, row in orc.reset(idx).items():
                exp[e] = row.astype(np.float32)
            g = env.reset(torch.from_numpy(pending.astype(np.uint8)).cuda()).cpu().numpy()
            np.testing.assert_array_equal(g, exp, err_msg=f"reset {msg}")
            pending[:] = False
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        a[rng.random((E, N)) < 0.05] = 0.0
        before = orc.stats()
        o_obs = np.empty((E, env.state_dim))
        o_rew, o_done = np.empty(E), np.zeros(E, dtype=bool)
        o_term = np.zeros_like(o_obs)
        for e, o in enumerate(orc.o):
            if auto:
                ob, r, d, tm = o.vec_step(a[e:e + 1])
                o_term[e] = tm[0]
            else:
                ob, r, d = o.step(a[e:e + 1])
            o_obs[e], o_rew[e], o_done[e] = ob[0], r[0], d[0]
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(a).cuda())
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done, err_msg=msg)
        np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32), err_msg=msg)
        np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32), err_msg=msg)
        _compare_state(env, orc, s, msg)
        _stats_equal(env.episode_stats().cpu().numpy(), orc.stats(), f"stats {msg}")
        if o_done.any():
            d = o_done
            if auto:
                np.testing.assert_array_equal(env.term_obs.cpu().numpy()[d], o_term[d].astype(np.float32),
                                              err_msg=msg)
            _stats_equal(env.last_episode_stats().cpu().numpy()[d], before[d], f"latch {msg}")
            ends += d
            pending |= d
    assert (ends >= 2).all(), ends.min()


# ------------------------------------------------------------------------------------------------
# 3. batches larger than one resident round of blocks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E", [(30, 69_700), (100, 66_000), (50, 40_000)])
def test_windows_in_multi_round_batches(N, E):
    """Random windows over several launches of one step (launch_rounds), the desynchronised hint on,
    auto-reset and masked resets: sampled envs from every round against their slice oracles."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    T, K = 12, 2
    rng = np.random.default_rng(N + E)
    close, tech, risk = _random_panel(N + E, T, N, K)
    s, t = _draw_windows(rng, E, T)
    kw = dict(hmax=100, initial_amount=500_000, turbulence_threshold=45.0)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, windows=(s, t), **kw)
    env.hint_desynchronised(True)
    sample = np.unique(np.concatenate([np.arange(6), rng.integers(0, E, 40), [E // 2, E - 65, E - 1]]))
    orc = _SliceOracles(close, tech, risk, s[sample], t[sample], np.full(len(sample), 500_000.0),
                        np.zeros((len(sample), N), dtype=np.int64), hmax=100, turbulence_threshold=45.0)
    o0 = orc.reset()
    g0 = env.reset().cpu().numpy()[sample]
    np.testing.assert_array_equal(g0, np.stack([o0[j] for j in range(len(sample))]).astype(np.float32))
    for k in range(2 * T):
        if k in (3, 9, 16):          # masked resets of a random subset
            m = rng.random(E) < 0.3
            g = env.reset(torch.from_numpy(m.astype(np.uint8)).cuda()).cpu().numpy()
            idx = np.nonzero(m[sample])[0]
            rows = orc.reset(idx)
            for j in idx:
                np.testing.assert_array_equal(g[sample[j]], rows[j].astype(np.float32))
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(a).cuda())
        g_obs, g_rew, g_done = g_obs.cpu().numpy(), g_rew.cpu().numpy(), g_done.cpu().numpy()
        for j, e in enumerate(sample):
            ob, r, d, _ = orc.o[j].vec_step(a[e:e + 1])
            assert bool(g_done[e]) == bool(d[0]), (k, e)
            assert g_rew[e] == np.float32(r[0]), (k, e)
            np.testing.assert_array_equal(g_obs[e], ob[0].astype(np.float32), err_msg=f"step {k} env {e}")
        st = env.state_numpy()
        os_ = orc.state()
        np.testing.assert_array_equal(st["cash"][sample], os_["cash"])
        np.testing.assert_array_equal(st["shares"][sample], os_["shares"])
        np.testing.assert_array_equal(st["window_day"][sample], os_["day"])
        # every env of the batch stays inside its window
        assert ((st["day"] >= s) & (st["day"] < t)).all()
        assert np.isfinite(g_obs).all() and np.isfinite(st["cash"]).all()


# ------------------------------------------------------------------------------------------------
# 4. windows [0, T) change nothing; detaching restores today's path
# ------------------------------------------------------------------------------------------------
def _outputs(env):
    st = env.state_numpy()
    out = {k: v for k, v in st.items()}
    out.update(obs=env.obs.cpu().numpy(), reward=env.reward.cpu().numpy(), done=env.done.cpu().numpy(),
               term_obs=env.term_obs.cpu().numpy(), realised=env.realised.cpu().numpy(),
               stats=env.episode_stats().cpu().numpy(), last=env.last_episode_stats().cpu().numpy(),
               block=env.enable_last_episode().cpu().numpy())
    return out


@pytest.mark.parametrize("N,K,hint", [(30, 8, False), (30, 8, True), (50, 2, False), (100, 3, False),
                                      (7, 2, False)])
def test_full_panel_windows_equal_the_unwindowed_env(N, K, hint):
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T = 200, 9
    close, tech, risk = _random_panel(N * 3 + K, T, N, K)
    rng = np.random.default_rng(N)
    kw = dict(hmax=100, initial_amount=200_000 * rng.uniform(0.5, 1.5, E),
              num_stock_shares=rng.integers(0, 9, (E, N)), turbulence_threshold=40.0, day=2)
    panel = StockPanel(close, tech, risk)
    ref = VecStockTradingEnv(panel, E, **kw)
    win = VecStockTradingEnv(panel, E, windows=(0, T), **kw)
    for env in (ref, win):
        env.hint_desynchronised(hint)
        env.enable_terminal_obs()
        env.enable_realised()
        env.enable_last_episode()
    assert win.max_step == ref.max_step == T - 1
    np.testing.assert_array_equal(win.observe().cpu().numpy(), ref.observe().cpu().numpy())
    for k in range(3 * T):
        if k == 2 * T:
            win.set_windows(None)                 # detached: the no-window kernels again
            assert win.windows is None
        if k in (4, 11):
            m = torch.from_numpy((rng.random(E) < 0.4).astype(np.uint8)).cuda()
            np.testing.assert_array_equal(win.reset(m).cpu().numpy(), ref.reset(m).cpu().numpy())
        a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
        ref.step(a)
        win.step(a)
        go, ro = _outputs(win), _outputs(ref)
        for key in ro:
            np.testing.assert_array_equal(go[key], ro[key], err_msg=f"{key} step {k}")


# ------------------------------------------------------------------------------------------------
# 5. edits of the window block, eagerly and between graph replays
# ------------------------------------------------------------------------------------------------
def test_window_edits_apply_at_the_documented_points():
    """An edited end applies from the next step; an edited start at the env's next reset -- the
    env mid-episode keeps its day; with the start edited and the episode finished, the auto-reset
    lands on the new start and the env then equals an oracle on the new window."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T, N, K = 70, 24, 30, 4
    close, tech, risk = _random_panel(5, T, N, K)
    rng = np.random.default_rng(5)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, windows=(2, 20), hmax=100,
                             initial_amount=100_000)
    env.enable_last_episode()
    env.reset()
    act = lambda: torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()  # noqa: E731
    for _ in range(3):
        env.step(act())
    day = env.state_numpy()["day"]
    assert (day == 5).all()
    s_new = np.full(E, 2)
    t_new = np.full(E, 20)
    s_new[:35] = 1                       # new start: applies at the next reset only
    t_new[::2] = 8                       # new end: day 5 -> done when day >= 7
    env.set_windows(torch.from_numpy(s_new).cuda(), torch.from_numpy(t_new).cuda())
    assert env.max_step == 18
    env.step(act())
    assert (env.state_numpy()["day"] == 6).all()            # nobody moved
    _, _, done, _ = env.step(act())
    assert (env.state_numpy()["day"][1::2] == 7).all()
    _, _, done, _ = env.step(act())                          # day 7 = the new end - 1: terminal
    done = done.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(done, t_new == 8)
    st = env.state_numpy()
    np.testing.assert_array_equal(st["day"][done], s_new[done])              # reset to the NEW start
    np.testing.assert_array_equal(st["start_day"][done], s_new[done])
    np.testing.assert_array_equal(st["price_day"][done], 7)          # reset_quirk: the row held
    np.testing.assert_array_equal(st["window_day"][done], 0)
    assert (st["day"][~done] == 8).all()
    last = env.last_episode["ret_n"].cpu().numpy()
    np.testing.assert_array_equal(last[done], 5)          # days 2 .. 7 of the old start


def test_graph_replay_sees_edited_windows():
    """A captured 4-step segment, replayed three times with the window block redrawn between replays
    (torch ops, masked to the envs that just finished) equals the same steps run eagerly."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.data import random_windows
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T, N, K, S = 130, 16, 30, 8, 4
    close, tech, risk = _random_panel(11, T, N, K)
    panel = StockPanel(close, tech, risk)
    g = torch.Generator(device="cuda").manual_seed(3)
    s0, t0 = random_windows(T, E, 5, generator=g)
    mk = lambda: VecStockTradingEnv(panel, E, windows=(s0, t0), hmax=100,  # noqa: E731
                                    initial_amount=100_000, turbulence_threshold=40.0)
    cap, eager = mk(), mk()
    for env in (cap, eager):
        env.hint_desynchronised(True)
        env.enable_terminal_obs()
        env.enable_last_episode()
        env.reset()
    pool = [torch.from_numpy(np.random.default_rng(i).uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
            for i in range(S)]
    hist = {k: torch.zeros((S,) + tuple(v.shape), dtype=v.dtype, device="cuda")
            for k, v in (("obs", cap.obs), ("reward", cap.reward), ("done", cap.done))}
    # warm-up step on a side stream (both envs take it), then capture S steps of `cap`
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.step(pool[0])
    torch.cuda.current_stream().wait_stream(side)
    eager.step(pool[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(S):
            o, r, d, _ = cap.step(pool[i])
            hist["obs"][i].copy_(o)
            hist["reward"][i].copy_(r)
            hist["done"][i].copy_(d)
    redrawn = 0
    for rep in range(3):
        graph.replay()
        ref = {k: [] for k in hist}
        for i in range(S):
            o, r, d, _ = eager.step(pool[i])
            ref["obs"].append(o.clone())
            ref["reward"].append(r.clone())
            ref["done"].append(d.clone())
        torch.cuda.synchronize()
        for k in hist:
            np.testing.assert_array_equal(hist[k].cpu().numpy(), torch.stack(ref[k]).cpu().numpy(),
                                          err_msg=f"{k} replay {rep}")
        for key in ("cash", "day", "price_day", "start_day", "trades"):
            np.testing.assert_array_equal(cap.state[key].cpu().numpy(), eager.state[key].cpu().numpy())
        np.testing.assert_array_equal(cap.last_episode_stats().cpu().numpy(),
                                      eager.last_episode_stats().cpu().numpy())
        # redraw the windows of the envs that just finished (and shorten some ends), on the device
        done = cap.done.bool()
        length = 3 + rep
        ns, nt = random_windows(T, E, length, generator=g)
        for env in (cap, eager):
            env.set_windows(ns, nt, mask=done)
        assert bool((cap.windows == eager.windows).all())
        redrawn += int(done.sum())
    assert redrawn > 0


# ------------------------------------------------------------------------------------------------
# 6. the ensemble's validation and trade windows as windows of one panel
# ------------------------------------------------------------------------------------------------
def _scripted_actions(models, obs):
    return np.concatenate([m.predict(obs[e:e + 1])[0] for e, m in enumerate(models)])


def _run_windows(panel, windows, offsets, base, n_envs, **kw):
    """One batch over `panel` whose env e runs window windows[e % W] (gym semantics, the ensemble's
    DummyVecEnv loop) driven by the scripted model with step offset offsets[e % W] -> per env the
    account values per day, and render() on the second-to-last day (the hand-over state)."""
    from finrl_amd.vec_env import VecStockTradingEnv
    import harness_loops as hl
    W = len(windows)
    s = np.array([windows[e % W][0] for e in range(n_envs)])
    t = np.array([windows[e % W][1] for e in range(n_envs)])
    env = VecStockTradingEnv(panel, n_envs, windows=(s, t), auto_reset=False, **kw)
    N = panel.N
    models = []
    for e in range(n_envs):
        m = hl.ScriptedModel(base, 1 + np.arange(N))
        m.step = offsets[e % W]
        models.append(m)
    obs = env.reset().cpu().numpy()

    def state_list(st, e):          # the facade's render(): [cash] + close + shares + tech (:453-478)
        row = st["price_day"][e]
        return ([float(st["cash"][e])] + panel.close[row].tolist() + st["shares"][e].astype(np.int64).tolist()
                + panel.tech[row].reshape(-1).tolist())

    st = env.state_numpy()
    values = [[float(st["asset0"][e])] for e in range(n_envs)]
    last = [None] * n_envs
    n = t - s
    for i in range(int(n.max())):
        a = _scripted_actions(models, obs)
        o, _, done, _ = env.step(torch.from_numpy(a).cuda())
        obs, done = o.cpu().numpy(), done.cpu().numpy().astype(bool)
        st = env.state_numpy()
        for e in range(n_envs):
            if i >= n[e]:
                continue
            assert bool(done[e]) == (i == n[e] - 1), (e, i)
            if i == n[e] - 2:
                last[e] = state_list(st, e)
            if not done[e]:
                sl = state_list(st, e)
                p, h = np.asarray(sl[1:N + 1]), np.asarray(sl[N + 1:2 * N + 1])
                values[e].append(sl[0] + sum(p * h))              # end_total_asset, :344-347
    return values, last


@pytest.mark.parametrize("name", ["ensemble", "ensemble_dow30"])
def test_ensemble_windows_in_one_batch(name):
    """tests/test_gpu_harness.py::test_ensemble_caller_surface runs the ensemble's validation window and
    its two trade windows as three envs, one after another.  Here the validation window and the first
    trade window (initial=True) share ONE batch over the full panel, 65 replicas each; the second trade
    window (initial=False, seeded with the first one's hand-over state) is a second batch.  Hand-over
    states and the per-day account values equal the reference's."""
    _need_gpu()
    import os
    import pandas as pd
    from finrl_amd import StockPanel
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"harness_{name}.npz"),
                allow_pickle=False)
    T, N, K, Tv, Tr, hmax, use_t = z["cfg_int"].tolist()
    cash0, bc, sc, rs, thr = z["cfg_float"].tolist()
    dates = z["dates"].tolist()
    panel = StockPanel(z["close"], z["tech"], z["risk"], dates=dates)
    kw = dict(hmax=hmax, buy_cost_pct=bc, sell_cost_pct=sc, reward_scaling=rs,
              turbulence_threshold=(thr if use_t else None))
    E = 130
    vals1, last1 = _run_windows(panel, [(0, Tv), (Tv, Tv + Tr)], [0, Tv], z["base"], E,
                                initial_amount=cash0, num_stock_shares=[0] * N, initial=True, **kw)
    for e in range(1, E, 2):
        np.testing.assert_array_equal(np.asarray(last1[e], np.float64), z["last_state_1"])
    ls1 = z["last_state_1"]
    vals2, last2 = _run_windows(panel, [(Tv + Tr, T)], [Tv + Tr], z["base"], E,
                                initial_amount=ls1[0],
                                num_stock_shares=[int(x) for x in ls1[N + 1:2 * N + 1]], initial=False, **kw)
    for e in range(E):
        np.testing.assert_array_equal(np.asarray(last2[e], np.float64), z["last_state_2"])
    csv = dict(zip(z["csv_names"].tolist(), z["csv_texts"].tolist()))
    for fn, vals, lo, env_ids in (("account_value_validation_A2C_63.csv", vals1, 0, range(0, E, 2)),
                                  ("account_value_trade_ensemble_126.csv", vals1, Tv, range(1, E, 2)),
                                  ("account_value_trade_ensemble_189.csv", vals2, Tv + Tr, range(E))):
        n = len(vals[env_ids[0]])
        for e in env_ids:           # the file the reference's terminal branch writes (:266-292)
            df = pd.DataFrame({"account_value": vals[e]})
            df["date"] = dates[lo:lo + n]
            df["daily_return"] = df["account_value"].pct_change(1)
            assert df.to_csv(index=False) == csv[fn], (fn, e)
