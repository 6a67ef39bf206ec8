"""Per-env episode windows of the batched crypto env (VecCryptoEnv(windows=...),
finenv_crypto_set_windows) on the MI355X: env e on panel rows [s_e, t_e) must equal the reference
CryptoEnv built on {'price_array': price[s_e:t_e], 'tech_array': tech[s_e:t_e]} -- the reference
fixtures embedded in a longer panel, and one CPU oracle per env on its slice -- bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATE_KEYS = ("cash", "total_asset", "gamma_return", "stocks")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(rng, T, N, W, decades=3.0):
    """Prices that drift over `decades` orders of magnitude along the panel, up or down per asset:
    the action normaliser of a window depends on where the window starts, so that a normaliser
    taken from the wrong row changes the trades."""
    drift = np.linspace(0.0, decades, T)[:, None] * rng.choice([-1.0, 1.0], N)
    price = 10.0 ** (rng.uniform(0.0, 3.0, N) + drift) * np.exp(
        np.cumsum(rng.normal(0, 0.004, (T, N)), axis=0))
    return price, rng.normal(0, 3000, (T, W))


def _windows(rng, T, E, L, spread=10):
    """Random windows of mixed lengths, each with at least one step per episode."""
    length = rng.integers(2 * L + 1, 2 * L + 1 + spread, E)
    start = (rng.random(E) * (T - length + 1)).astype(np.int64)
    return start, start + length


class _Twins:
    """One CryptoOracle(price[s:t], tech[s:t], n_envs=1) per env of `idx`: the reference env a
    windowed env must equal.  restart(k, s, t) replaces env k's twin by a fresh one on a new slice."""

    def __init__(self, price, tech, s, t, idx, **kw):
        self.price, self.tech, self.kw = price, tech, kw
        self.idx = np.asarray(idx)
        self.s = np.array(s, dtype=np.int64)[self.idx]
        self.t = np.array(t, dtype=np.int64)[self.idx]
        self.orc = [self._make(a, b) for a, b in zip(self.s, self.t)]

    def _make(self, s, t):
        from oracle.crypto import CryptoOracle
        return CryptoOracle(self.price[s:t], self.tech[s:t], n_envs=1, **self.kw)

    def restart(self, k, s, t):
        self.s[k], self.t[k] = s, t
        self.orc[k] = self._make(s, t)
        return self.orc[k].reset()[0]

    def reset(self, ks=None):
        ks = range(len(self.orc)) if ks is None else ks
        return np.stack([self.orc[k].reset()[0] for k in ks])

    def step(self, actions, auto_reset):
        outs = [o.vec_step(actions[i:i + 1], auto_reset=auto_reset) for o, i in zip(self.orc, self.idx)]
        return (np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]),
                np.concatenate([o[2] for o in outs]), np.concatenate([o[3] for o in outs]))

    def state(self):
        sts = [o.state() for o in self.orc]
        return {k: np.concatenate([s[k] for s in sts]) for k in sts[0]}


def _assert_state(env, twins, tag, keys=STATE_KEYS + ("episode_return",)):
    st, os_ = env.state_numpy(), twins.state()
    for k in keys:
        np.testing.assert_array_equal(st[k][twins.idx], os_[k], err_msg=f"{k} {tag}")
    # state["time"] is the panel row, window_time() the reference's self.time
    np.testing.assert_array_equal(st["time"][twins.idx] - twins.s, os_["time"], err_msg=f"time {tag}")
    np.testing.assert_array_equal(env.window_time().cpu().numpy()[twins.idx], os_["time"])


def _assert_step(env, twins, out, a, auto, tag, state_keys=STATE_KEYS + ("episode_return",),
                 moves=None):
    """Compare one step's outputs and state with the twins.  moves(e) -> the (start, end) an env that
    reported done and was auto-reset now runs on, or None if it stays on its slice: such an env is
    from here on a fresh reference env on the new slice (its gamma_return zeroed, as documented)."""
    g_obs, g_rew, g_done = (x.cpu().numpy() for x in out)
    o_obs, o_rew, o_done, o_term = twins.step(a, auto)
    i = twins.idx
    np.testing.assert_array_equal(g_done[i].astype(bool), o_done, err_msg=f"done {tag}")
    np.testing.assert_array_equal(g_rew[i], o_rew.astype(np.float32), err_msg=f"reward {tag}")
    if auto and moves is not None:
        for k in np.flatnonzero(o_done):
            new = moves(int(i[k]))
            if new is not None:
                o_obs[k] = twins.restart(k, *new)
                env.state["gamma_return"][int(i[k])] = 0.0
    np.testing.assert_array_equal(g_obs[i], o_obs, err_msg=f"obs {tag}")
    if auto and env.term_obs is not None and o_done.any():
        np.testing.assert_array_equal(env.term_obs.cpu().numpy()[i][o_done], o_term[o_done])
    _assert_state(env, twins, tag, state_keys)
    return g_done.astype(bool)


# ------------------------------------------------------------------------------------------
# 1. the reference fixtures, each embedded twice in a longer NaN-padded panel
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n1", "n9_poor", "pairs10", "lookback3"])
def test_fixture_windows_in_a_nan_padded_panel(name):
    """E = 70 envs (a full wave and a 6-lane tail) spread over two copies of the fixture's arrays at
    different offsets of a panel that is NaN everywhere else: every output and state field equals
    the fixture through its episodes, and no NaN ever appears -- nothing outside a window is read."""
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    z = np.load(os.path.join(GOLDEN, f"crypto_{name}.npz"), allow_pickle=False)
    T, N, W, S, L = z["cfg_int"].tolist()
    cap, bc, sc, g = z["cfg_float"].tolist()
    E = 70
    offs = np.array([3, 3 + T + 5])
    P = int(offs[1]) + T + 4
    price, tech = np.full((P, N), np.nan), np.full((P, W), np.nan)
    for o in offs:
        price[o:o + T], tech[o:o + T] = z["price"], z["tech"]
    s = offs[(np.arange(E) * 7 // 3) % 2]                      # both copies inside each wave
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, lookback=L,
                       initial_capital=cap, buy_cost_pct=bc, sell_cost_pct=sc, gamma=g,
                       auto_reset=False, windows=(s, s + T))
    assert env.max_step == T - L - 1
    np.testing.assert_array_equal(env.norm_table()[offs[0]], z["norm"])
    np.testing.assert_array_equal(env.window_time().cpu().numpy(), L - 1)   # the constructor's episode
    resets = dict(zip(z["reset_step"].tolist(), z["reset_obs"]))
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(obs, np.broadcast_to(resets[-1], obs.shape))
    nd = 0
    for k in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][k], (E, N)).copy()).cuda()
        obs, rew, done, _ = env.step(a)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        st = env.state_numpy()
        assert not np.isnan(obs).any() and not np.isnan(rew).any()
        for key in ("cash", "total_asset", "gamma_return", "last_reward", "stocks"):
            assert not np.isnan(st[key]).any(), key
        np.testing.assert_array_equal(done.astype(bool), bool(z["done"][k]))
        np.testing.assert_array_equal(st["time"] - s, z["time"][k])
        np.testing.assert_array_equal(env.window_time().cpu().numpy(), z["time"][k])
        np.testing.assert_array_equal(st["stocks"], np.broadcast_to(z["stocks"][k], (E, N)))
        np.testing.assert_array_equal(st["cash"], z["cash"][k])
        np.testing.assert_array_equal(st["total_asset"], z["total_asset"][k])
        np.testing.assert_array_equal(st["gamma_return"], z["gamma_return"][k])
        np.testing.assert_array_equal(st["last_reward"], z["reward"][k])
        np.testing.assert_array_equal(rew, np.float32(z["reward"][k]))
        np.testing.assert_array_equal(obs, np.broadcast_to(z["obs"][k], obs.shape), err_msg=f"obs step {k}")
        if z["done"][k]:
            nd += 1
            obs = env.reset().cpu().numpy()
            np.testing.assert_array_equal(obs, np.broadcast_to(resets[k], obs.shape))
    assert nd == 2


# ------------------------------------------------------------------------------------------
# 2. random windows of mixed lengths against one oracle per env, every launch shape
# ------------------------------------------------------------------------------------------
SHAPES = [
    dict(E=200, T=40, N=10, W=40, L=1),       # trader + streamer, column split (12-wide build)
    dict(E=130, T=40, N=1, W=0, L=1),         # one asset, no indicators
    dict(E=70, T=40, N=8, W=56, L=1),         # 8-wide build, D = 65
    dict(E=136, T=50, N=12, W=5, L=3),        # 12-wide build at its full width, lookback 3
    dict(E=128, T=40, N=16, W=47, L=1),       # 16-wide build, D = 64
    dict(E=68, T=40, N=32, W=1, L=2),         # 32-wide build
    dict(E=192, T=50, N=10, W=40, L=3),       # 120 indicator columns: no column split
]


@pytest.mark.parametrize("auto,record", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("cfg", SHAPES, ids=lambda c: "E{E}-N{N}-W{W}-L{L}".format(**c))
def test_random_windows_match_per_env_oracles(cfg, auto, record):
    _need_gpu()
    from finrl_amd.rollout import RolloutBuffer
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = cfg["E"], cfg["T"], cfg["N"], cfg["W"], cfg["L"]
    rng = np.random.default_rng(E + 3 * N + L)
    price, tech = _panel(rng, T, N, W)
    s, t = _windows(rng, T, E, L)
    kw = dict(lookback=L, initial_capital=3e4, buy_cost_pct=0.0012, sell_cost_pct=0.0008, gamma=0.98)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, auto_reset=auto,
                       windows=(s, t), **kw)
    env.enable_terminal_obs()
    twins = _Twins(price, tech, s, t, np.arange(E), **kw)
    assert env.max_step == int((t - s).max()) - L - 1
    assert len(np.unique(env.norm_table()[s], axis=0)) > 1 or N == 1     # normalisers do differ
    np.testing.assert_array_equal(env.reset().cpu().numpy(), twins.reset())
    steps = 2 * int((t - s).max() - 2 * L) + 2
    buf = RolloutBuffer(steps, E, env.obs_dim, N) if record else None
    ends = np.zeros(E, dtype=int)
    for k in range(steps):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        a[rng.random((E, N)) < 0.1] = 0.0
        at = torch.from_numpy(a).cuda()
        if record:
            v, lp = torch.randn(E, device="cuda"), torch.randn(E, device="cuda")
            buf.step(env, k, at, v, lp)
            out = (buf.obs[k + 1], buf.rewards[k], buf.dones[k])
            assert torch.equal(buf.actions[k], at) and torch.equal(buf.values[k], v)
            assert torch.equal(buf.log_probs[k], lp)
        else:
            out = env.step(at)[:3]
        done = _assert_step(env, twins, out, a, auto, f"step {k}")
        ends += done
        if not auto and done.any():               # the caller's reset of the finished envs
            rows = env.reset(torch.from_numpy(done.astype(np.uint8))).cpu().numpy()
            np.testing.assert_array_equal(rows[done], twins.reset(np.flatnonzero(done)))
            _assert_state(env, twins, f"reset after step {k}")
    assert (ends >= 2).all()
    np.testing.assert_array_equal(env.active_windows.cpu().numpy(), np.stack([s, t]))


@pytest.mark.parametrize("record", [False, True])
def test_random_windows_large_batch_regime(record):
    """E = 140,000: the four-wave launch shape.  A sample of envs (whole first and last waves and
    others) against their oracles, and the done flag of EVERY env against the window arithmetic."""
    _need_gpu()
    from finrl_amd.rollout import RolloutBuffer
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = 140_000, 60, 10, 40, 1
    rng = np.random.default_rng(91)
    price, tech = _panel(rng, T, N, W)
    s, t = _windows(rng, T, E, L, spread=6)
    kw = dict(initial_capital=2e5, buy_cost_pct=0.0012, sell_cost_pct=0.0008, gamma=0.97)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, windows=(s, t), **kw)
    env.enable_terminal_obs()
    idx = np.unique(np.concatenate([np.arange(64), np.arange(E - 96, E), rng.integers(0, E, 140)]))
    twins = _Twins(price, tech, s, t, idx, **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy()[idx], twins.reset())
    steps = 2 * int((t - s).max() - 2 * L) + 2
    buf = RolloutBuffer(steps, E, env.obs_dim, N) if record else None
    time, ends = s + L - 1, np.zeros(E, dtype=int)
    for k in range(steps):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        at = torch.from_numpy(a).cuda()
        if record:
            v, lp = torch.randn(E, device="cuda"), torch.randn(E, device="cuda")
            buf.step(env, k, at, v, lp)
            out = (buf.obs[k + 1], buf.rewards[k], buf.dones[k])
            assert torch.equal(buf.actions[k], at) and torch.equal(buf.values[k], v)
        else:
            out = env.step(at)[:3]
        done = _assert_step(env, twins, out, a, True, f"step {k}")
        want = time + 1 == t - L - 1
        np.testing.assert_array_equal(done, want, err_msg=f"done of every env, step {k}")
        time = np.where(want, s + L - 1, time + 1)
        np.testing.assert_array_equal(env.state["time"].cpu().numpy(), time)
        ends += done
    assert (ends >= 2).all()


# ------------------------------------------------------------------------------------------
# 3. pending and active windows
# ------------------------------------------------------------------------------------------
def test_edited_windows_wait_for_each_envs_own_reset():
    """Windows edited in mid-episode: every running episode goes on against the OLD slice's oracle,
    step by step, and each env moves to its new window -- start, end and normaliser -- at its own
    auto-reset.  The new starts lie where prices are orders of magnitude away from the old ones."""
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = 128, 80, 10, 40, 1
    rng = np.random.default_rng(17)
    price, tech = _panel(rng, T, N, W, decades=5.0)
    s0, t0 = _windows(rng, T // 4, E, L)                                  # first quarter of the panel
    s1, t1 = _windows(rng, T // 4, E, L)
    s1, t1 = s1 + 3 * T // 4, t1 + 3 * T // 4                             # last quarter: decades away
    kw = dict(initial_capital=5e4, gamma=0.95)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, windows=(s0, t0), **kw)
    nt = env.norm_table()
    assert (nt[s0] != nt[s1]).any(axis=1).all()                           # every env's normaliser changes
    twins = _Twins(price, tech, s0, t0, np.arange(E), **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), twins.reset())
    moved = np.zeros(E, dtype=bool)
    act = np.stack([s0, t0])
    edited = False

    def moves(e):
        """The first auto-reset after the edit takes the pending window."""
        if not edited or moved[e]:
            return None
        moved[e] = True
        act[:, e] = s1[e], t1[e]
        return s1[e], t1[e]

    for k in range(3 + 2 * 12 + 2):
        if k == 3:                                                        # everybody is mid-episode
            env.set_windows(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda())
            edited = True
            np.testing.assert_array_equal(env.windows.cpu().numpy(), np.stack([s1, t1]))
            np.testing.assert_array_equal(env.active_windows.cpu().numpy(), act)
            assert not (env.state["time"].cpu().numpy() == s0 + L - 1).all()
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        before = moved.copy()
        _assert_step(env, twins, env.step(torch.from_numpy(a).cuda())[:3], a, True, f"step {k}",
                     STATE_KEYS, moves)
        if k == 3:
            assert not moved.all()            # most envs go on inside their old window
        assert (moved >= before).all()
        np.testing.assert_array_equal(env.active_windows.cpu().numpy(), act, err_msg=f"step {k}")
    assert moved.all()


# ------------------------------------------------------------------------------------------
# 4. redraw on done inside a captured graph
# ------------------------------------------------------------------------------------------
def test_redraw_on_done_inside_a_captured_graph():
    """step + set_windows(*random_windows(...), mask=done) captured in one graph, no reset launch:
    every replay equals the eager run fed the same draws, and every episode its slice's oracle."""
    _need_gpu()
    from finrl_amd.data import random_windows
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L, LEN, steps = 256, 90, 10, 40, 1, 8, 30
    rng = np.random.default_rng(29)
    price, tech = _panel(rng, T, N, W, decades=4.0)
    kw = dict(initial_capital=1e5, gamma=0.96)
    gen = torch.Generator(device="cuda").manual_seed(5)
    s0, t0 = random_windows(T, E, torch.randint(3, LEN + 1, (E,)), generator=gen)
    s0n, t0n = s0.cpu().numpy().astype(np.int64), t0.cpu().numpy().astype(np.int64)

    def make():
        env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, windows=(s0n, t0n), **kw)
        env.reset()
        return env

    env, eager = make(), make()
    a_in = torch.zeros(E, N, device="cuda")
    drawn = torch.zeros(2, E, dtype=torch.int32, device="cuda")
    outs = {}

    def body():
        obs, rew, done, _ = env.step(a_in)
        ns, nt = random_windows(T, E, LEN, device="cuda")
        env.set_windows(ns, nt, mask=done)
        # "a fresh env object on a new slice": the redrawn envs' discounted return starts over
        env.state["gamma_return"].masked_fill_(done.bool(), 0.0)
        drawn[0].copy_(ns)
        drawn[1].copy_(nt)
        outs.update(obs=obs.clone(), rew=rew.clone(), done=done.clone())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                          # warm-up step 0 (eager, on the side stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    acts = rng.uniform(-1, 1, (steps, E, N)).astype(np.float32)
    # the warm-up ran one step with zero actions: mirror it everywhere
    twins = _Twins(price, tech, s0n, t0n, np.arange(E), **kw)
    twins.reset()
    pend, act = np.stack([s0n, t0n]), np.stack([s0n, t0n])

    def follow(a, tag):
        """The eager env and the oracles take the step the graph env just took."""
        d = drawn.cpu().numpy().astype(np.int64)
        e_obs, e_rew, e_done, _ = eager.step(torch.from_numpy(a).cuda())
        eager.set_windows(drawn[0], drawn[1], mask=e_done)
        eager.state["gamma_return"].masked_fill_(e_done.bool(), 0.0)
        assert torch.equal(outs["obs"], e_obs) and torch.equal(outs["rew"], e_rew), tag
        assert torch.equal(outs["done"], e_done), tag
        for key in env.state:
            assert torch.equal(env.state[key], eager.state[key]), (key, tag)
        assert torch.equal(env.windows, eager.windows), tag
        assert torch.equal(env.active_windows, eager.active_windows), tag
        o_obs, o_rew, o_done, _ = twins.step(a, True)
        done = outs["done"].cpu().numpy().astype(bool)
        np.testing.assert_array_equal(done, o_done, err_msg=tag)
        np.testing.assert_array_equal(outs["rew"].cpu().numpy(), o_rew.astype(np.float32), err_msg=tag)
        g_obs = outs["obs"].cpu().numpy()
        for e in np.flatnonzero(done):                  # auto-reset: onto the window that was pending
            act[:, e] = pend[:, e]
            o_obs[e] = twins.restart(e, *pend[:, e])
            pend[:, e] = d[:, e]
        np.testing.assert_array_equal(g_obs, o_obs, err_msg=tag)
        np.testing.assert_array_equal(env.active_windows.cpu().numpy(), act, err_msg=tag)
        np.testing.assert_array_equal(env.windows.cpu().numpy(), pend, err_msg=tag)
        st, os_ = env.state_numpy(), twins.state()
        for key in STATE_KEYS:
            np.testing.assert_array_equal(st[key], os_[key], err_msg=f"{key} {tag}")
        np.testing.assert_array_equal(st["time"] - act[0], os_["time"], err_msg=tag)
        return done

    ends = follow(np.zeros((E, N), dtype=np.float32), "warm-up").astype(int)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    # (the capture itself runs nothing: state and windows are as the warm-up left them)
    for k in range(steps):
        a_in.copy_(torch.from_numpy(acts[k]))
        graph.replay()
        torch.cuda.synchronize()
        ends += follow(acts[k], f"replay {k}")
    assert (ends >= 2).all()
    assert len(np.unique(act[0])) > 20                  # the envs really sit on redrawn windows


# ------------------------------------------------------------------------------------------
# 5. whole-panel windows equal no windows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(E=200, T=20, N=10, W=40, L=1), dict(E=70, T=20, N=3, W=7, L=3),
                                 dict(E=140_000, T=12, N=10, W=40, L=1)],
                         ids=lambda c: "E{E}-N{N}-L{L}".format(**c))
def test_whole_panel_windows_equal_no_windows(cfg):
    """Windows [0, T) for every env: every output and state field equals a no-window env's over an
    episode end; detached, the env is back on the no-window kernel and still equal."""
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = cfg["E"], cfg["T"], cfg["N"], cfg["W"], cfg["L"]
    rng = np.random.default_rng(E + L)
    price, tech = _panel(rng, T, N, W, decades=1.0)
    kw = dict(lookback=L, initial_capital=7e4, gamma=0.97)
    plain = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, **kw)
    win = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, windows=(0, T), **kw)
    assert win.max_step == plain.max_step
    np.testing.assert_array_equal(win.action_norm_vector, plain.action_norm_vector)
    plain.enable_terminal_obs()
    win.enable_terminal_obs()
    assert torch.equal(win.reset(), plain.reset())
    nd = 0
    for k in range(2 * T):
        if k == T + 3:
            assert win.set_windows(None) is None and win.windows is None
            assert win.max_step == plain.max_step
        a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
        p_out, w_out = plain.step(a), win.step(a)
        for x, y, what in zip(p_out[:3], w_out[:3], ("obs", "reward", "done")):
            assert torch.equal(x, y), (what, k)
        for key in plain.state:
            assert torch.equal(plain.state[key], win.state[key]), (key, k)
        if bool(p_out[2].any()):
            nd += 1
            assert torch.equal(plain.term_obs, win.term_obs)
    assert nd >= 2


# ------------------------------------------------------------------------------------------
# 6. masked reset onto pending windows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto", [True, False])
def test_masked_reset_moves_a_subset_to_its_pending_windows(auto):
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = 200, 70, 10, 40, 2
    rng = np.random.default_rng(41 + auto)
    price, tech = _panel(rng, T, N, W, decades=4.0)
    s0, t0 = _windows(rng, T, E, L)
    s1, t1 = _windows(rng, T, E, L)
    kw = dict(lookback=L, initial_capital=5e4, gamma=0.95)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, auto_reset=auto,
                       windows=(s0, t0), **kw)
    twins = _Twins(price, tech, s0, t0, np.arange(E), **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), twins.reset())
    act, pend = np.stack([s0, t0]), np.stack([s0, t0])

    def moves(e):
        """An env that ends takes its pending window, if that is another one."""
        if (pend[:, e] == act[:, e]).all():
            return None
        act[:, e] = pend[:, e]
        return pend[:, e]

    n_moved_at_end = 0
    for k in range(30):
        if k in (2, 9):                                     # in mid-episode: move 40 % of the envs
            m = rng.random(E) < 0.4
            env.set_windows(s1, t1, mask=m)                 # host values, validated
            pend[:, m] = np.stack([s1, t1])[:, m]
            if k == 2:                                      # ... at once, with a masked reset
                rows = env.reset(torch.from_numpy(m.astype(np.uint8))).cpu().numpy()
                for e in np.flatnonzero(m):
                    act[:, e] = pend[:, e]
                    np.testing.assert_array_equal(rows[e], twins.restart(e, *pend[:, e]))
                env.state["gamma_return"][torch.from_numpy(m).cuda()] = 0.0
                _assert_state(env, twins, f"reset at {k}", STATE_KEYS)
            # (k == 9: no reset -- those envs move when their episodes end)
            np.testing.assert_array_equal(env.windows.cpu().numpy(), pend)
            np.testing.assert_array_equal(env.active_windows.cpu().numpy(), act)
            s1, t1 = _windows(rng, T, E, L)
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        before = act.copy()
        done = _assert_step(env, twins, env.step(torch.from_numpy(a).cuda())[:3], a, auto,
                            f"step {k}", STATE_KEYS, moves)
        if not auto and done.any():                         # the caller's reset of the finished envs
            rows = env.reset(torch.from_numpy(done.astype(np.uint8))).cpu().numpy()
            for e in np.flatnonzero(done):
                new = moves(e)
                if new is not None:
                    env.state["gamma_return"][int(e)] = 0.0
                np.testing.assert_array_equal(
                    rows[e], twins.reset([e])[0] if new is None else twins.restart(e, *new))
            _assert_state(env, twins, f"reset after step {k}", STATE_KEYS)
        n_moved_at_end += int((act != before).any(axis=0).sum())
        np.testing.assert_array_equal(env.active_windows.cpu().numpy(), act, err_msg=f"step {k}")
    assert n_moved_at_end > 0 and (act == pend).all()
    with pytest.raises(ValueError):
        env.set_windows(0, L + 1)                           # shorter than lookback + 2 rows
    with pytest.raises(ValueError):
        env.set_windows(5, T + 1)


def test_start_row_with_a_non_positive_price_is_refused_on_the_host():
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    rng = np.random.default_rng(2)
    price, tech = _panel(rng, 30, 4, 3)
    price[7, 2] = 0.0
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, 8)
    with pytest.raises(ValueError, match="price"):
        env.set_windows(7, 20)
    assert env.set_windows(8, 20) is env.windows


# ------------------------------------------------------------------------------------------
# 7. sharding
# ------------------------------------------------------------------------------------------
def test_sharded_windows_equal_the_single_batch():
    """make_sharded_env(kind="crypto", windows=(start [E], end [E])): two ranks' shards, each on its
    slice of the windows, equal the single batch (both shards live on the box's one GPU; envs are
    independent, so no collective is part of the data path)."""
    _need_gpu()
    from finrl_amd.distributed import make_sharded_env, shard_range
    E, T, N, W, L = 141, 40, 10, 40, 1
    rng = np.random.default_rng(42)
    price, tech = _panel(rng, T, N, W)
    cfg = {"price_array": price, "tech_array": tech}
    s, t = _windows(rng, T, E, L)
    kw = dict(initial_capital=2e5, gamma=0.97)
    whole = make_sharded_env(cfg, E, kind="crypto", rank=0, world=1, device="cuda:0",
                             windows=(s, t), **kw)
    shards = [make_sharded_env(cfg, E, kind="crypto", rank=r, world=2, device="cuda:0",
                               windows=(torch.from_numpy(s).cuda(), t), **kw) for r in (0, 1)]
    rngs = [shard_range(E, r, 2) for r in (0, 1)]
    assert [sh.num_envs for sh in shards] == [hi - lo for lo, hi in rngs]
    ref = whole.reset()
    for sh, (lo, hi) in zip(shards, rngs):
        np.testing.assert_array_equal(sh.windows.cpu().numpy(), np.stack([s, t])[:, lo:hi])
        assert torch.equal(sh.reset(), ref[lo:hi])
    nd = 0
    for k in range(2 * 12 + 2):
        a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
        obs, rew, done, _ = whole.step(a)
        nd += int(done.sum())
        for sh, (lo, hi) in zip(shards, rngs):
            o, r, d, _ = sh.step(a[lo:hi].contiguous())
            assert torch.equal(o, obs[lo:hi]) and torch.equal(r, rew[lo:hi]) and torch.equal(d, done[lo:hi])
            for key in whole.state:
                assert torch.equal(sh.state[key], whole.state[key][..., lo:hi]), (key, k)
            assert torch.equal(sh.episode_return(), whole.episode_return()[lo:hi])
    assert nd >= 2 * E


def test_graphed_segment_on_a_windowed_env():
    """finrl_amd.graph.GraphedSegment over a windowed env, unchanged: replays equal eager collection."""
    _need_gpu()
    from finrl_amd.graph import GraphedSegment
    from finrl_amd.rollout import RolloutBuffer
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L, n_steps = 256, 40, 10, 40, 1, 8
    rng = np.random.default_rng(6)
    price, tech = _panel(rng, T, N, W)
    s, t = _windows(rng, T, E, L)
    wgt = torch.from_numpy(rng.normal(0, 0.3, (1 + N + W, N)).astype(np.float32)).cuda()

    def policy(obs):
        a = torch.tanh(obs @ wgt)
        return a, a.sum(1), -a.abs().sum(1)

    envs = [VecCryptoEnv({"price_array": price, "tech_array": tech}, E, windows=(s, t)) for _ in range(2)]
    bufs = [RolloutBuffer(n_steps, E, envs[0].obs_dim, N) for _ in range(2)]
    first = [env.reset().clone() for env in envs]
    seg = GraphedSegment(envs[0], policy, bufs[0])
    obs_g, obs_e = first
    for r in range(4):                                   # 32 steps: past two episode ends per env
        seg.replay(obs_g)
        obs_e = bufs[1].collect(envs[1], policy, obs_e).clone()
        obs_g = bufs[0].obs[n_steps].clone()
        for k in ("obs", "actions", "values", "log_probs", "rewards", "dones"):
            assert torch.equal(getattr(bufs[0], k), getattr(bufs[1], k)), (k, r)
        for key in envs[0].state:
            assert torch.equal(envs[0].state[key], envs[1].state[key]), (key, r)
    assert bool(bufs[0].dones.any())
    # the window blocks survived the segment's warm-up
    assert torch.equal(envs[0].active_windows, envs[1].active_windows)
    np.testing.assert_array_equal(envs[0].active_windows.cpu().numpy(), np.stack([s, t]))
