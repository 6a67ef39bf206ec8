"""Degenerate panel sizes for the stock env: a one-day panel (every step is terminal, :221),
two- and three-day panels (episodes of 1-2 trading steps), with 1, 5 and 32 tickers, auto-reset
on; and one small batch through every instantiation the step launchers choose between.  HIP
(through the C ABI) vs the oracle, exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 5, 32])
def test_tiny_panels_match_oracle(T, N):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import bench
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E = 70
    rng = np.random.default_rng(T * 10 + N)
    close = (50 + rng.uniform(0, 10, (T, N))).astype(np.float32).astype(np.float64)
    tech = rng.normal(0, 1, (T, 2, N)).astype(np.float32).astype(np.float64)
    risk = np.abs(rng.normal(0, 30, T))
    kw = dict(bench.ENV_KW)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    env.enable_terminal_obs()
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    n_done = 0
    for s in range(9):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, o_done, o_term = orc.vec_step(a)
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done, err_msg=f"step {s}")
        np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32))
        np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32))
        if o_done.any():
            n_done += 1
            np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done],
                                          o_term[o_done].astype(np.float32))
    assert n_done >= 3
    st, os_ = env.state_numpy(), orc.state()
    np.testing.assert_array_equal(st["cash"], os_["cash"])
    np.testing.assert_array_equal(st["shares"], os_["shares"])


# (N, hmax, desync_hint, windows): one case per leaf of the step launcher's choice of instantiation
_LEAVES = [
    (30, 100, False, False),    # np32 plain
    (30, 100, True, False),     # np32 desync-hint (DES)
    (30, 100, False, True),     # np32 windows (DES + WIN)
    (50, 100, False, False),    # np64 plain
    (50, 100, False, True),     # np64 WIN
    (100, 100, False, False),   # np128 wide N = 100
    (100, 100, False, True),    # np128 wide N = 100, WIN
    (100, 300, False, False),   # np128 generic at N = 100 (hmax > 255 does not fit the wide kernel's keys)
    (100, 300, False, True),    # np128 generic at N = 100, WIN
    (128, 100, False, False),   # np128 generic, full width
]


@pytest.mark.parametrize("track_stats", [False, True])
@pytest.mark.parametrize("use_turbulence", [False, True])
@pytest.mark.parametrize("N,hmax,desync_hint,windows", _LEAVES)
def test_every_step_launch_leaf_matches_the_oracle(N, hmax, desync_hint, windows, use_turbulence, track_stats):
    """Every instantiation the step launchers can select (width x TURB x STATS x the leaves above) steps
    a batch of two full 64-env blocks and a partial one exactly like the oracle.  `windows` gives every
    env the window [0, T): the WIN kernels run while one whole-panel oracle stays the exact reference."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, T, K = 130, 6, 2
    rng = np.random.default_rng(1000 * N + hmax)
    close = (50 + rng.uniform(0, 10, (T, N))).astype(np.float32).astype(np.float64)
    tech = rng.normal(0, 1, (T, K, N)).astype(np.float32).astype(np.float64)
    risk = np.abs(rng.normal(0, 30, T))
    kw = dict(hmax=hmax, initial_amount=1_000_000, num_stock_shares=rng.integers(0, 40, N),
              turbulence_threshold=(float(np.median(risk)) if use_turbulence else None))
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, track_stats=track_stats, **kw)
    env.enable_terminal_obs()
    if desync_hint:
        env.hint_desynchronised()
    if windows:
        env.set_windows(0, T)
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    n_done = 0
    for s in range(2 * T + 2):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, o_done, o_term = orc.vec_step(a)
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done, err_msg=f"step {s}")
        np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32), err_msg=f"step {s}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32), err_msg=f"step {s}")
        if o_done.any():
            n_done += 1
            np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done],
                                          o_term[o_done].astype(np.float32))
    assert n_done == 2
    st, os_ = env.state_numpy(), orc.state()
    np.testing.assert_array_equal(st["cash"], os_["cash"])
    np.testing.assert_array_equal(st["shares"], os_["shares"])


# (N, hmax, E): one shape per width path -- np32 (three blocks), np64, WideGeom<100>, generic np128
@pytest.mark.parametrize("N,hmax,E", [(5, 100, 130), (40, 100, 70), (100, 100, 70), (100, 300, 70)])
def test_results_do_not_depend_on_the_chosen_step_kernel(N, hmax, E):
    """The step kernel is chosen when the handle is bound and again when the desync hint flips or
    windows are attached -- here in the middle of an episode, after steps have run.  Env B goes
    lock-step -> hinted -> whole-panel windows (0, T) -> hint off and on through an episode end
    with its auto-reset; its twin A stays lock-step throughout.  Every output and every state tensor
    of the two are the same bits after every step."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    T, K = 12, 2
    rng = np.random.default_rng(77 * N + hmax)
    close = (50 + rng.uniform(0, 10, (T, N))).astype(np.float32).astype(np.float64)
    tech = rng.normal(0, 1, (T, K, N)).astype(np.float32).astype(np.float64)
    risk = np.abs(rng.normal(0, 30, T))
    panel = StockPanel(close, tech, risk)
    kw = dict(hmax=hmax, initial_amount=1_000_000, num_stock_shares=rng.integers(0, 40, N),
              turbulence_threshold=float(np.median(risk)), auto_reset=True)
    a_env, b_env = VecStockTradingEnv(panel, E, **kw), VecStockTradingEnv(panel, E, **kw)
    for env in (a_env, b_env):
        env.enable_terminal_obs()
        env.enable_realised()
    assert torch.equal(a_env.reset(), b_env.reset())
    changes = {3: lambda: b_env.hint_desynchronised(True), 6: lambda: b_env.set_windows(0, T),
               9: lambda: b_env.hint_desynchronised(False)}
    n_done = 0
    for s in range(T + 3):                       # the episode ends on step T, after the last change
        if s in changes:
            changes[s]()
        act = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
        a_out, b_out = a_env.step(act), b_env.step(act)
        for name, x, y in zip(("obs", "reward", "done"), a_out, b_out):
            assert torch.equal(x, y), f"{name}, step {s}"
        for name in ("term_obs", "realised"):
            assert torch.equal(getattr(a_env, name), getattr(b_env, name)), f"{name}, step {s}"
        for name in a_env.state:
            assert torch.equal(a_env.state[name], b_env.state[name]), f"state {name}, step {s}"
        n_done += int(a_out[2].all())
    assert n_done == 1


def test_refresh_after_in_place_state_edit():
    """Editing day / price_day of a batch that already HOLDS shares (what bench.py --desync does
    after a reset) makes the carried begin asset stale; finenv_stock_refresh re-evaluates it.  Every
    env then behaves like a reference env constructed on its own start day (no reset before the
    first step): compared against one oracle per env."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, T, N, K = 70, 24, 5, 2
    rng = np.random.default_rng(4)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.02, (T, N)), axis=0))
    tech = rng.normal(0, 1, (T, K, N))
    risk = np.abs(rng.normal(0, 30, T))
    shares0 = rng.integers(1, 40, N)
    kw = dict(hmax=20, initial_amount=20_000, num_stock_shares=shares0)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, auto_reset=False, **kw)
    offs = rng.integers(0, T - 6, E).astype(np.int32)
    for k in ("day", "price_day", "start_day"):
        env.state[k].copy_(torch.from_numpy(offs).cuda())
    stale = env.state["begin_asset"].cpu().numpy().copy()
    env.refresh()
    fresh = env.state["begin_asset"].cpu().numpy()
    assert (stale != fresh).any()
    orcs = [StockOracle(close, tech, risk, n_envs=1, day=int(d), **kw) for d in offs]
    np.testing.assert_array_equal(
        env.observe().cpu().numpy(),
        np.stack([np.concatenate([[20_000.0], close[d], shares0, tech[d].reshape(-1)])
                  for d in offs]).astype(np.float32))
    for s in range(5):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        obs, rew, done, _ = env.step(torch.from_numpy(a).cuda())
        exp = [o.step(a[e:e + 1]) for e, o in enumerate(orcs)]
        np.testing.assert_array_equal(obs.cpu().numpy(),
                                      np.concatenate([x[0] for x in exp]).astype(np.float32))
        np.testing.assert_array_equal(rew.cpu().numpy(),
                                      np.concatenate([x[1] for x in exp]).astype(np.float32),
                                      err_msg=f"reward step {s}")
    np.testing.assert_array_equal(env.state_numpy()["cash"],
                                  np.array([o.state()["cash"][0] for o in orcs]))


def test_step_out_tensors_are_validated():
    """step(out=...) rejects what the kernel would silently mis-write: wrong dtype / device / shape,
    overlapping rows; a single-env batch takes any row stride torch reports."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    T, N, K = 6, 3, 1
    rng = np.random.default_rng(1)
    close = 100 + rng.random((T, N))
    tech = rng.normal(0, 1, (T, K, N))
    for E in (4, 1):
        env = VecStockTradingEnv(StockPanel(close, tech, np.zeros(T)), E)
        env.reset()
        D = env.state_dim
        a = torch.zeros(E, N, device="cuda")
        rew, done = torch.zeros(E, device="cuda"), torch.zeros(E, dtype=torch.uint8, device="cuda")
        good = torch.zeros(3, E, D, device="cuda")[1]
        obs, _, _, _ = env.step(a, out=(good, rew, done))
        assert torch.equal(obs, env.observe())
        with pytest.raises(ValueError):
            env.step(a, out=(torch.zeros(E, D, dtype=torch.float64, device="cuda"), rew, done))
        with pytest.raises(ValueError):
            env.step(a, out=(torch.zeros(E, D), rew, done))
        with pytest.raises(ValueError):
            env.step(a, out=(good, rew.double(), done))
        with pytest.raises(ValueError):
            env.step(a, out=(torch.zeros(E, D + 1, device="cuda"), rew, done))
        if E > 1:
            with pytest.raises(ValueError):
                env.step(a, out=(torch.zeros(1, D, device="cuda").expand(E, D), rew, done))
    npenv = VecStockTradingEnvNP({"price_array": close, "tech_array": tech.reshape(T, -1),
                                  "turbulence_array": np.zeros(T), "if_train": False}, 4)
    npenv.reset()
    with pytest.raises(ValueError):
        npenv.step(torch.zeros(4, N, device="cuda"),
                   out=(torch.zeros(4, npenv.obs.shape[1], dtype=torch.float64, device="cuda"),
                        npenv.reward, npenv.done))

