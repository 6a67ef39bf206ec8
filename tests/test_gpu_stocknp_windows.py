"""Per-env episode windows of the batched array-state stock env (VecStockTradingEnvNP(windows=...),
finenv_stocknp_set_windows) on the MI355X: env e on panel rows [s_e, t_e) must equal the reference
env built on {'price_array': price[s_e:t_e], 'tech_array': tech[s_e:t_e], 'turbulence_array':
turb[s_e:t_e]} -- the reference fixtures embedded in a longer panel, and one CPU oracle per env on
its slice -- bit for bit, NumPy dtype tags included."""
import glob
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import harness_loops as hl  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
NAMES = sorted(os.path.basename(p)[len("stocknp_"):-4]
               for p in glob.glob(os.path.join(GOLDEN, "stocknp_*.npz")))
STATE_KEYS = ("amount", "amount_tag", "total_asset", "ta_tag", "gamma_reward", "g_tag",
              "episode_return", "stocks", "cool_down")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(rng, T, N, K):
    price = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    return price, rng.normal(0, 50, (T, N * K)), np.abs(rng.normal(0, 70, T))


def _config(price, tech, turb, if_train=False):
    return {"price_array": price, "tech_array": tech, "turbulence_array": turb, "if_train": if_train}


def _windows(rng, T, E, lo=2):
    """Random windows, lengths uniform in [lo, T]."""
    length = rng.integers(lo, T + 1, E)
    start = (rng.random(E) * (T - length + 1)).astype(np.int64)
    return start, start + length


def _start_states(rng, E, N, cap):
    """Per-env start states, a mix of Python-float and float32 amounts (eval / train style)."""
    st0 = rng.integers(0, 20, (E, N)).astype(np.float32)
    tag0 = rng.integers(0, 2, E).astype(np.int32)
    am0 = np.where(tag0 == 1, (cap * rng.uniform(0.9, 1.1, E)).astype(np.float32),
                   cap * rng.uniform(0.9, 1.1, E))
    return st0, am0, tag0


def _padded(arrays, T, offs, P):
    """The fixture's arrays at row offsets `offs` of a P-row panel that is NaN everywhere else."""
    out = []
    for a in arrays:
        big = np.full((P,) + a.shape[1:], np.nan, dtype=a.dtype)
        for o in offs:
            big[o:o + T] = a
        out.append(big)
    return out


class _Twins:
    """The reference envs a windowed batch must equal: for the envs `idx`, one
    StockNpOracle(price[s:t], tech[s:t], turb[s:t]) per distinct window (envs that share a window
    share an oracle, each from its own start state).  restart(k, s, t) gives env k a fresh
    oracle of its own on a new slice."""

    def __init__(self, arrays, s, t, idx, starts, **kw):
        self.arrays, self.kw, self.starts = arrays, kw, starts
        self.idx = np.asarray(idx)
        self.s = np.array(s, dtype=np.int64)[self.idx]
        self.t = np.array(t, dtype=np.int64)[self.idx]
        groups = {}
        for k, w in enumerate(zip(self.s.tolist(), self.t.tolist())):
            groups.setdefault(w, []).append(k)
        self.groups = [[np.array(ks), self._make(np.array(ks), *w)] for w, ks in groups.items()]
        self.where = np.empty((len(self.idx), 2), dtype=np.int64)     # env k -> (group, row)
        for g, (ks, _) in enumerate(self.groups):
            self.where[ks] = np.stack([np.full(len(ks), g), np.arange(len(ks))], axis=1)

    def _make(self, ks, s, t):
        from oracle.stocknp import StockNpOracle
        o = StockNpOracle(*(a[s:t] for a in self.arrays), n_envs=len(ks), **self.kw)
        if self.starts is not None:
            o.set_initial(*(x[self.idx[ks]] for x in self.starts))
        return o

    def restart(self, k, s, t):
        """Env k leaves its oracle (whose row goes on unobserved) for a fresh one on [s, t)."""
        self.s[k], self.t[k] = s, t
        self.groups.append([np.array([k]), self._make(np.array([k]), s, t)])
        self.where[k] = len(self.groups) - 1, 0
        return self.groups[-1][1].reset()[0]

    def _gather(self, parts):
        """Per-group arrays (rows in group order) -> one array in env order."""
        sizes = np.array([len(ks) for ks, _ in self.groups])
        first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        return np.concatenate(parts)[first[self.where[:, 0]] + self.where[:, 1]]

    def reset(self, ks=None):
        """Reset obs of every env, or of the envs `ks` (whole groups reset together: callers pass
        envs that ended their episodes, and envs that share a window end together)."""
        if ks is None:
            return self._gather([o.reset() for _, o in self.groups])
        ks = np.asarray(ks)
        out = np.empty((len(ks), self.groups[0][1].D), dtype=np.float32)
        for g in np.unique(self.where[ks, 0]):
            gk, o = self.groups[g]
            live = gk[self.where[gk, 0] == g]
            assert np.isin(live, ks).all()
            obs = o.reset()
            for j, k in enumerate(ks):
                if self.where[k, 0] == g:
                    out[j] = obs[self.where[k, 1]]
        return out

    def step(self, actions, auto_reset):
        outs = [o.vec_step(actions[self.idx[ks]], auto_reset=auto_reset) for ks, o in self.groups]
        return tuple(self._gather([o[j] for o in outs]) for j in range(4))

    def state(self):
        sts = [o.state() for _, o in self.groups]
        return {k: self._gather([s[k] for s in sts]) for k in sts[0]}


def _assert_state(env, twins, tag, keys=STATE_KEYS):
    st, os_ = env.state_numpy(), twins.state()
    for k in keys:
        np.testing.assert_array_equal(st[k][twins.idx], os_[k], err_msg=f"{k} {tag}")
    # state["day"] is the panel row, window_day() the reference's self.day
    np.testing.assert_array_equal(st["day"][twins.idx] - twins.s, os_["day"], err_msg=f"day {tag}")
    np.testing.assert_array_equal(env.window_day().cpu().numpy()[twins.idx], os_["day"])


def _assert_step(env, twins, out, a, auto, tag, moves=None):
    """Compare one step's outputs and state with the twins.  moves(e) -> the (start, end) an env that
    reported done and was auto-reset now runs on, or None if it stays on its slice."""
    g_obs, g_rew, g_done = (x.cpu().numpy() for x in out)
    o_obs, o_rew, o_done, o_term = twins.step(a, auto)
    i = twins.idx
    np.testing.assert_array_equal(g_done[i].astype(bool), o_done, err_msg=f"done {tag}")
    np.testing.assert_array_equal(g_rew[i], o_rew.astype(np.float32), err_msg=f"reward {tag}")
    if auto and env.term_obs is not None and o_done.any():
        np.testing.assert_array_equal(env.term_obs.cpu().numpy()[i][o_done], o_term[o_done])
    if auto and moves is not None:
        # (episode_return is latched by the terminal step: the fresh twin has none yet)
        st, os_ = env.state_numpy(), twins.state()
        np.testing.assert_array_equal(st["episode_return"][i][o_done], os_["episode_return"][o_done])
        for k in np.flatnonzero(o_done):
            new = moves(int(i[k]))
            if new is not None:
                o_obs[k] = twins.restart(k, *new)
        np.testing.assert_array_equal(g_obs[i], o_obs, err_msg=f"obs {tag}")
        _assert_state(env, twins, tag, tuple(k for k in STATE_KEYS if k != "episode_return"))
    else:
        np.testing.assert_array_equal(g_obs[i], o_obs, err_msg=f"obs {tag}")
        _assert_state(env, twins, tag)
    return g_done.astype(bool)


# ------------------------------------------------------------------------------------------
# 1. the reference fixtures, each embedded twice in a longer NaN-padded panel
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_windows_in_a_nan_padded_panel(name):
    """E = 70 envs (a full wave and a 6-lane tail), even envs on the first copy of the fixture's
    arrays and odd envs on the second, in a panel that is NaN everywhere else: every output and
    state field equals the fixture through its episodes and no NaN ever appears -- nothing outside
    a window is read."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    assert len(NAMES) == 10
    z = np.load(os.path.join(GOLDEN, f"stocknp_{name}.npz"), allow_pickle=False)
    T, N, K, S, if_train = z["cfg_int"].tolist()
    cap, ms, bc, sc, g = z["cfg_float"].tolist()
    E = 70
    offs = np.array([5, 5 + T + 3])
    P = int(offs[1]) + T + 4
    price, tech, turb = _padded((z["price_array"], z["tech_array"], z["turbulence_array"]), T, offs, P)
    extra = {}
    if "obs_amount_floor" in z.files:            # StockEnvNAS100 fixtures (env_nas100_wrds.py)
        extra = dict(obs_amount_floor=float(z["obs_amount_floor"]),
                     turbulence_thresh=float(z["turbulence_thresh"]))
    s_e = offs[np.arange(E) % 2]
    with np.errstate(invalid="ignore"):
        env = VecStockTradingEnvNP(_config(price, tech, turb), E, gamma=g, max_stock=ms,
                                   initial_capital=cap, buy_cost_pct=bc, sell_cost_pct=sc,
                                   auto_reset=False, windows=(s_e, s_e + T), **extra)
    assert env.max_step == T - 1
    np.testing.assert_array_equal(env.active_windows.cpu().numpy(), np.stack([s_e, s_e + T]))
    ri = 0

    def do_reset():
        nonlocal ri
        env.set_start_state(z["reset_stocks0"][ri], z["reset_amount0"][ri],
                            z["reset_amount0_tag"][ri])
        obs = env.reset().cpu().numpy()
        np.testing.assert_array_equal(obs, np.broadcast_to(z["reset_obs"][ri], obs.shape))
        np.testing.assert_array_equal(env.state_numpy()["day"], s_e)
        ri += 1

    do_reset()
    nd = 0
    for s in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][s], (E, N)).copy()).cuda()
        obs, rew, done, _ = env.step(a)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        assert not np.isnan(obs).any() and not np.isnan(rew).any(), s
        st = env.state_numpy()
        wd = env.window_day().cpu().numpy()
        for e in (0, 1, 63, 64, 69):
            assert bool(done[e]) == bool(z["done"][s]), (s, e)
            assert wd[e] == z["day"][s] and st["day"][e] == s_e[e] + z["day"][s], (s, e)
            np.testing.assert_array_equal(st["stocks"][e], z["stocks"][s], err_msg=f"step {s}")
            np.testing.assert_array_equal(st["cool_down"][e], z["cool_down"][s])
            assert (st["amount"][e], st["amount_tag"][e]) == (z["amount"][s], z["amount_tag"][s]), s
            assert (st["total_asset"][e], st["ta_tag"][e]) == (z["total_asset"][s], z["ta_tag"][s]), s
            assert (st["gamma_reward"][e], st["g_tag"][e]) == (z["gamma_reward"][s], z["g_tag"][s]), s
            assert (st["last_reward"][e], st["reward_tag"][e]) == (z["reward"][s], z["reward_tag"][s]), s
            assert st["episode_return"][e] == z["episode_return"][s], s
            assert rew[e] == np.float32(z["reward"][s])
            np.testing.assert_array_equal(obs[e], z["obs"][s], err_msg=f"obs step {s}")
        if z["done"][s]:
            nd += 1
            do_reset()
    assert nd == 2


# ------------------------------------------------------------------------------------------
# 2. random windows against one oracle per env on its slice
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("cfg", [dict(E=1000, T=30, N=30, K=8, cap=1e6),
                                 dict(E=130, T=20, N=5, K=2, cap=4e3),
                                 dict(E=65, T=12, N=32, K=1, cap=2e5),
                                 dict(E=64, T=10, N=1, K=0, cap=1e3)])
def test_random_windows_match_one_oracle_per_env(cfg, auto):
    """A partial wave, a block seam at 256, N at the 32 limit and N = 1 without indicators; window
    lengths uniform in [2, T]; mixed Python-float / float32 start amounts; auto-reset inside the
    step, or a masked host reset of the envs that reported done."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K = cfg["E"], cfg["T"], cfg["N"], cfg["K"]
    rng = np.random.default_rng(E + N)
    arrays = _panel(rng, T, N, K)
    s, t = _windows(rng, T, E)
    s[0], t[0] = 0, T                                   # the longest window is in the batch
    kw = dict(gamma=0.98, initial_capital=cfg["cap"], buy_cost_pct=0.0012, sell_cost_pct=0.0008)
    starts = _start_states(rng, E, N, cfg["cap"])
    twins = _Twins(arrays, s, t, np.arange(E), starts, **kw)
    env = VecStockTradingEnvNP(_config(*arrays), E, auto_reset=auto, windows=(s, t), **kw)
    env.enable_terminal_obs()
    env.set_start_state(*starts)
    assert env.max_step == T - 1
    np.testing.assert_array_equal(env.reset().cpu().numpy(), twins.reset())
    _assert_state(env, twins, "reset", tuple(k for k in STATE_KEYS if k != "episode_return"))
    ends = np.zeros(E, dtype=np.int64)
    mixed = False
    for step in range(2 * T + 2):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        out = env.step(torch.from_numpy(a).cuda())[:3]
        done = _assert_step(env, twins, out, a, auto, f"step {step}")
        ends += done
        mixed |= bool(done.any() and not done.all())
        if not auto and done.any():
            before = env.obs.clone()
            obs = env.reset(torch.from_numpy(done).cuda()).cpu().numpy()
            ks = np.flatnonzero(done)
            np.testing.assert_array_equal(obs[ks], twins.reset(ks))
            np.testing.assert_array_equal(obs[~done], before.cpu().numpy()[~done])
            _assert_state(env, twins, f"host reset {step}")
    # (properties of the oracle's done flags alone: the run covers what it is meant to cover)
    assert ends.min() >= 2 and mixed


# ------------------------------------------------------------------------------------------
# 3. whole-panel windows equal no windows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,K", [(200, 30, 8), (70, 3, 2)])
def test_whole_panel_windows_equal_no_windows(E, N, K):
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    T = 9
    rng = np.random.default_rng(E)
    arrays = _panel(rng, T, N, K)
    starts = _start_states(rng, E, N, 1e5)
    kw = dict(initial_capital=1e5, gamma=0.97)
    plain = VecStockTradingEnvNP(_config(*arrays), E, **kw)
    win = VecStockTradingEnvNP(_config(*arrays), E, windows=(0, T), **kw)
    assert plain.windows is None and plain.active_windows is None
    assert torch.equal(plain.window_day(), plain.state["day"])
    for env in (plain, win):
        env.enable_terminal_obs()
        env.set_start_state(*starts)
    assert torch.equal(plain.reset(), win.reset())
    nd = 0
    for step in range(2 * T + 1):
        a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
        plain.step(a)
        win.step(a)
        for k in ("obs", "reward", "done"):
            assert torch.equal(getattr(plain, k), getattr(win, k)), (step, k)
        for k in plain.state:
            assert torch.equal(plain.state[k], win.state[k]), (step, k)
        assert torch.equal(win.window_day(), win.state["day"])
        if bool(plain.done.any()):
            nd += 1
            assert torch.equal(plain.term_obs, win.term_obs)
    assert nd >= 2
    # detached: the no-window kernels again, and the same results
    assert win.set_windows(None) is None and win.windows is None and win.active_windows is None
    assert win.max_step == T - 1
    a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
    plain.step(a)
    win.step(a)
    assert torch.equal(plain.obs, win.obs) and torch.equal(plain.reward, win.reward)


# ------------------------------------------------------------------------------------------
# 4. edits of the pending rows wait for each env's own reset
# ------------------------------------------------------------------------------------------
def test_pending_edits_wait_for_each_envs_own_reset():
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K = 130, 24, 5, 2
    rng = np.random.default_rng(4)
    arrays = _panel(rng, T, N, K)
    s0, t0 = _windows(rng, T, E, lo=4)
    s1, t1 = _windows(rng, T, E, lo=3)
    starts = _start_states(rng, E, N, 5e4)
    kw = dict(initial_capital=5e4)
    twins = _Twins(arrays, s0, t0, np.arange(E), starts, **kw)
    env = VecStockTradingEnvNP(_config(*arrays), E, windows=(s0, t0), **kw)
    env.set_start_state(*starts)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), twins.reset())
    moved = np.zeros(E, dtype=bool)

    def moves(e):
        if moved[e]:
            return None
        moved[e] = True
        return int(s1[e]), int(t1[e])

    for step in range(2 * T):
        if step == 2:                                   # mid-episode for every env (lengths >= 4)
            env.set_windows(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda())
            np.testing.assert_array_equal(env.windows.cpu().numpy(), np.stack([s1, t1]))
            np.testing.assert_array_equal(env.active_windows.cpu().numpy(), np.stack([s0, t0]))
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        out = env.step(torch.from_numpy(a).cuda())[:3]
        # done on the step the OLD window ends (the twins), the new pair taken at that reset only
        _assert_step(env, twins, out, a, True, f"step {step}", moves=moves if step >= 2 else None)
        want = np.where(moved, np.stack([s1, t1]), np.stack([s0, t0]))
        np.testing.assert_array_equal(env.active_windows.cpu().numpy(), want, err_msg=f"step {step}")
    assert moved.all()


# ------------------------------------------------------------------------------------------
# 5. a masked reset moves exactly the selected envs
# ------------------------------------------------------------------------------------------
def test_masked_reset_moves_exactly_the_selected_envs():
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K = 200, 20, 30, 2
    rng = np.random.default_rng(5)
    arrays = _panel(rng, T, N, K)
    s0, t0 = _windows(rng, T, E, lo=6)
    s1, t1 = _windows(rng, T, E)
    starts = _start_states(rng, E, N, 1e5)
    kw = dict(initial_capital=1e5)
    twins = _Twins(arrays, s0, t0, np.arange(E), starts, **kw)
    env = VecStockTradingEnvNP(_config(*arrays), E, windows=(s0, t0), **kw)
    env.set_start_state(*starts)
    env.reset()
    twins.reset()
    for step in range(3):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        _assert_step(env, twins, env.step(torch.from_numpy(a).cuda())[:3], a, True, f"step {step}")
    env.set_windows(s1, t1)
    sel = rng.random(E) < 0.4
    sel[[0, 63, 64]] = True, False, True
    obs_before = env.obs.clone().cpu().numpy()
    st_before = env.state_numpy()
    obs = env.reset(torch.from_numpy(sel).cuda()).cpu().numpy()
    st = env.state_numpy()
    want = np.where(sel, np.stack([s1, t1]), np.stack([s0, t0]))
    np.testing.assert_array_equal(env.active_windows.cpu().numpy(), want)
    np.testing.assert_array_equal(env.windows.cpu().numpy(), np.stack([s1, t1]))
    np.testing.assert_array_equal(obs[~sel], obs_before[~sel])
    for k in st:
        np.testing.assert_array_equal(st[k][~sel], st_before[k][~sel], err_msg=k)
    np.testing.assert_array_equal(st["day"][sel], s1[sel])
    for k in np.flatnonzero(sel):
        np.testing.assert_array_equal(obs[k], twins.restart(k, int(s1[k]), int(t1[k])))
    # and the batch goes on, every env on the window it is now running
    for step in range(T):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        out = env.step(torch.from_numpy(a).cuda())[:3]
        _assert_step(env, twins, out, a, True, f"after {step}",
                     moves=lambda e: None if sel[e] else (int(s1[e]), int(t1[e])))
        sel |= out[2].cpu().numpy().astype(bool)


# ------------------------------------------------------------------------------------------
# 6. redraw on done inside a captured graph
# ------------------------------------------------------------------------------------------
def test_redraw_on_done_inside_a_captured_graph():
    """step + set_windows(device tensors, mask=done) + draw_train_start(mask=done) captured on one
    stream and replayed equals the same sequence run eagerly with the same generator seeds."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K, L = 130, 40, 5, 2, 8
    rng = np.random.default_rng(6)
    arrays = _panel(rng, T, N, K)
    length = rng.integers(3, L + 1, E)
    s0 = (rng.random(E) * (T - length + 1)).astype(np.int64)
    envs = [VecStockTradingEnvNP(_config(*arrays, if_train=True), E, seed=3, windows=(s0, s0 + length),
                                 initial_capital=2e5) for _ in range(2)]
    eager, graphed = envs
    act = torch.zeros(E, N, device="cuda")
    ns = torch.zeros(E, dtype=torch.int32, device="cuda")
    nt = torch.zeros(E, dtype=torch.int32, device="cuda")

    def feed():
        ln = rng.integers(3, L + 1, E)
        st = (rng.random(E) * (T - ln + 1)).astype(np.int64)
        act.copy_(torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)))
        ns.copy_(torch.from_numpy(st.astype(np.int32)))
        nt.copy_(torch.from_numpy((st + ln).astype(np.int32)))

    def body(env):
        env.step(act)
        env.set_windows(ns, nt, mask=env.done)
        env.draw_train_start(mask=env.done)

    def same(tag):
        torch.cuda.synchronize()
        for k in ("obs", "reward", "done", "windows", "active_windows"):
            assert torch.equal(getattr(eager, k), getattr(graphed, k)), (tag, k)
        for k in eager.state:
            assert torch.equal(eager.state[k], graphed.state[k]), (tag, k)

    for env in envs:
        env.reset()
    feed()
    for env in envs:                                    # one eager step first (caches, allocations)
        body(env)
    same("warm-up")
    g = torch.cuda.CUDAGraph()
    g.register_generator_state(graphed.generator)
    with torch.cuda.graph(g):
        body(graphed)
    for env in envs:
        env.generator.manual_seed(17)
    n_done = 0
    first_active = eager.active_windows.clone()
    for rep in range(3 * L + 2):
        feed()
        body(eager)
        g.replay()
        same(rep)
        n_done += int(eager.done.sum())
    assert n_done >= 3 * E                              # every env ended episodes and was redrawn
    assert not torch.equal(first_active, eager.active_windows)
    # the redrawn start states were priced on the redrawn windows' first rows
    st = eager.state_numpy()
    first = eager.price_ary[eager.windows[0].cpu().numpy()]
    total = st["amount0"] + (st["stocks0"].astype(np.float64) * first).sum(1)
    # (initial_capital * [0.95, 1.05) of :88; the float32 roundings of the draw are ~1e-7 of it)
    assert (total > 2e5 * 0.949).all() and (total < 2e5 * 1.051).all()


# ------------------------------------------------------------------------------------------
# 7. train-mode start states on windows
# ------------------------------------------------------------------------------------------
def test_train_mode_start_is_priced_on_the_window_start():
    _need_gpu()
    from finrl_amd.vec_stocknp import TAG_F32, VecStockTradingEnvNP
    from oracle.stocknp import StockNpOracle
    E, T, N, K = 130, 30, 30, 2
    cap = 1e6
    rng = np.random.default_rng(7)
    price, tech, turb = _panel(rng, T, N, K)
    price = price * np.linspace(1.0, 6.0, T)[:, None]    # the first row of a slice matters
    s, t = _windows(rng, T, E)
    init = rng.integers(0, 5, N).astype(np.float32)
    env = VecStockTradingEnvNP(_config(price, tech, turb, if_train=True), E, seed=11, windows=(s, t),
                               initial_capital=cap, initial_stocks=init)
    obs = env.reset().cpu().numpy()
    st = env.state_numpy()
    extra = st["stocks0"] - init
    assert (extra == np.round(extra)).all() and (extra >= 0).all() and (extra < 64).all()
    assert len(np.unique(extra)) > 32
    assert (st["amount0_tag"] == TAG_F32).all()
    assert (st["amount0"] == st["amount0"].astype(np.float32)).all()
    total = st["amount0"] + (st["stocks0"] * env.price_ary[s]).sum(1)
    assert (total >= cap * 0.95).all() and (total <= cap * 1.05).all()
    np.testing.assert_array_equal(st["day"], s)
    for e in range(E):
        orc = StockNpOracle(price[s[e]:t[e]], tech[s[e]:t[e]], turb[s[e]:t[e]], n_envs=1,
                            initial_capital=cap)
        orc.set_initial(st["stocks0"][e:e + 1], st["amount0"][e:e + 1], st["amount0_tag"][e:e + 1])
        np.testing.assert_array_equal(obs[e], orc.reset()[0], err_msg=f"env {e}")
        os_ = orc.state()
        assert (st["total_asset"][e], st["ta_tag"][e]) == (os_["total_asset"][0], os_["ta_tag"][0])
    # a masked draw leaves the other envs' start states alone
    keep = rng.random(E) < 0.5
    env.draw_train_start(mask=torch.from_numpy(~keep).cuda())
    st2 = env.state_numpy()
    for k in ("stocks0", "amount0", "amount0_tag"):
        np.testing.assert_array_equal(st2[k][keep], st[k][keep])
    assert (st2["stocks0"][~keep] != st["stocks0"][~keep]).any(axis=1).all()


# ------------------------------------------------------------------------------------------
# 8. more 64-env groups than one resident round
# ------------------------------------------------------------------------------------------
def test_windows_in_a_batch_larger_than_one_round():
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K = 70_100, 10, 30, 2
    rng = np.random.default_rng(8)
    arrays = _panel(rng, T, N, K)
    s, t = _windows(rng, T, E)
    sample = np.unique(np.concatenate([[0, 255, 256, E - 1, E - 70, 35_071, 35_072, 35_327, 35_328],
                                       rng.choice(E, 200, replace=False)]))
    s[sample[0]], t[sample[0]] = 0, T
    twins = _Twins(arrays, s, t, sample, None)
    env = VecStockTradingEnvNP(_config(*arrays), E, windows=(s, t))
    np.testing.assert_array_equal(env.reset()[sample].cpu().numpy(), twins.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    ends = np.zeros(len(sample), dtype=np.int64)
    for step in range(2 * T + 2):
        a = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
        out = env.step(a)[:3]
        ends += _assert_step(env, twins, out, a.cpu().numpy(), True, f"step {step}")[sample]
    assert ends.min() >= 2
    length = (t - s).astype(np.int64)
    # every env of the batch, not only the sample: where it stands after 2T + 2 steps of its cycle
    np.testing.assert_array_equal(env.window_day().cpu().numpy(), (2 * T + 2) % (length - 1))


# ------------------------------------------------------------------------------------------
# 9. the ElegantRL prediction loop on windows
# ------------------------------------------------------------------------------------------
def test_elegantrl_prediction_loop_on_three_windows():
    """The harness_erl_stocknp panel at three offsets of one NaN-padded panel, E = 3: each env's
    total_asset after every step is the reference loop's episode_total_assets."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    z = np.load(os.path.join(GOLDEN, "harness_erl_stocknp.npz"), allow_pickle=False)
    T, N, K = z["cfg_int"].tolist()
    offs = np.array([2, 2 + T + 1, 2 + 2 * T + 6])
    P = int(offs[2]) + T + 3
    arrays = _padded((z["price_array"], z["tech_array"], z["turbulence_array"]), T, offs, P)
    with np.errstate(invalid="ignore"):
        env = VecStockTradingEnvNP(_config(*arrays), 3, auto_reset=False, windows=(offs, offs + T))
    assert env.max_step == T - 1
    acts = [hl.scripted_act(z["base"], 3 + np.arange(N)) for _ in range(3)]
    obs = env.reset().cpu().numpy()
    want = z["episode_total_assets"]
    np.testing.assert_array_equal(env.state_numpy()["initial_total_asset"], np.repeat(want[0], 3))
    for i in range(env.max_step):
        a = np.concatenate([act(obs[e:e + 1]) for e, act in enumerate(acts)])
        o, _, done, _ = env.step(torch.from_numpy(a).cuda())
        obs = o.cpu().numpy()
        assert not np.isnan(obs).any()
        np.testing.assert_array_equal(env.state_numpy()["total_asset"], np.repeat(want[i + 1], 3),
                                      err_msg=f"step {i}")
        assert bool(done.all()) == (i == env.max_step - 1) and bool(done.any()) == bool(done.all())
    np.testing.assert_array_equal(env.state_numpy()["episode_return"],
                                  np.repeat(z["episode_returns"][-1], 3))
