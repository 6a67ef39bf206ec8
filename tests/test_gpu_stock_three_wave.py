"""The lock-step step kernel for up to 32 tickers runs three waves per block: a sorter wave loads the
action tile, builds and sorts the keys of the canonical trade order and hands them to the trader through
LDS (finenv_stock_kernels.inc, `kThreeWave`), then streams the last rows of the block's observations.
Everything that hand-off could get wrong -- tile rows of
partial blocks, ticker counts that do not fill a float4 or a row, the per-lane terminal and turbulent
flags, ties and zeros among the keys, a flag that is stale in the second launch of a graph or the second
round of a large batch -- against oracle.stock.StockOracle with tolerance 0 on obs, reward, done,
terminal obs and the state blocks.  Every env draws its own actions.

Per-env windows select the desynchronised instantiation whatever the hint says (choose_step); the window
case below pins that this stays so and stays exact beside the three-wave form."""
import functools

import numpy as np
import pytest

import action_domain_cases as adc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(N, T, K=2, seed=0, flag_frac=0.05):
    rng = np.random.default_rng(900 + 31 * N + T + seed)
    close = (50 + rng.uniform(0, 10, (T, N))).astype(np.float32).astype(np.float64)
    tech = rng.normal(0, 1, (T, K, N)).astype(np.float32).astype(np.float64)
    tech[:, 0, :][rng.random((T, N)) < flag_frac] = 1.0        # untradable days (:105 / :174)
    risk = np.abs(rng.normal(0, 30, T))
    return close, tech, risk


def _make(panel, E, **kw):
    """(device env on the plain launch form, oracle), both reset and their first observations compared."""
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    okw = {k: v for k, v in kw.items() if k != "track_stats"}
    env = VecStockTradingEnv(StockPanel(*panel), E, auto_reset=True, **kw)
    env.enable_terminal_obs()
    orc = StockOracle(*panel, n_envs=E, **okw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    return env, orc


_STATE = ("cash", "shares", "cost", "trades", "day", "price_day", "episode", "last_reward", "turbulence")


def _step_and_compare(env, orc, a, msg):
    """One auto-reset step of both; -> the oracle's done."""
    g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda())
    o_obs, o_rew, o_done, o_term = orc.vec_step(a)
    np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done, err_msg=msg)
    np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32), err_msg=msg)
    np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32), err_msg=msg)
    if o_done.any():
        np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done], o_term[o_done].astype(np.float32),
                                      err_msg=msg)
    st, os_ = env.state_numpy(), orc.state()
    for k in _STATE:
        np.testing.assert_array_equal(st[k], os_[k], err_msg=f"{k} {msg}")
    return o_done


@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("N", [1, 2, 7, 30, 31, 32])
def test_shape_sweep(N, E):
    """T = 5, 12 steps: two episode ends with auto-reset; hmax 1 and 100; with and without the Sharpe sums
    (the STATS instantiations).  Per-env cash and holdings, so that no two envs trade alike."""
    _need_gpu()
    T = 5
    panel = _panel(N, T)
    for hmax in (1, 100):
        for stats in (True, False):
            rng = np.random.default_rng(N * 1000 + E * 10 + hmax + stats)
            kw = dict(hmax=hmax, initial_amount=20_000 * rng.uniform(0.5, 1.5, E),
                      num_stock_shares=rng.integers(0, 30, (E, N)), track_stats=stats)
            env, orc = _make(panel, E, **kw)
            ends = 0
            for s in range(12):
                a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
                done = _step_and_compare(env, orc, a, f"hmax {hmax} stats {stats} step {s}")
                assert done.all() or not done.any()
                ends += int(done.all())
            assert ends == 2


@pytest.mark.parametrize("E", [47, 48, 49, 112])
def test_row_split_between_streamer_and_sorter(E):
    """The sorter streams the market-data chunks of a block's rows 48..63, the streamer those before: last
    blocks that end just below, at and just above the split, alone and behind a full block."""
    _need_gpu()
    N, T = 30, 4
    rng = np.random.default_rng(E)
    env, orc = _make(_panel(N, T, K=8), E, hmax=100, initial_amount=30_000 * rng.uniform(0.5, 1.5, E),
                     num_stock_shares=rng.integers(0, 30, (E, N)))
    for s in range(T + 2):
        _step_and_compare(env, orc, rng.uniform(-1, 1, (E, N)).astype(np.float32), f"step {s}")


def test_first_light_one_block():
    """One full block, DOW30 width, three steps: the smallest run of the three-wave kernel."""
    _need_gpu()
    E, N = 64, 30
    rng = np.random.default_rng(1)
    env, orc = _make(_panel(N, 6), E, hmax=100, initial_amount=50_000)
    for s in range(3):
        _step_and_compare(env, orc, rng.uniform(-1, 1, (E, N)).astype(np.float32), f"step {s}")


@functools.lru_cache(maxsize=None)
def _edge_actions(E, N, hmax):
    rng = np.random.default_rng(E + N)
    sub = np.float32(1.0) / np.float32(hmax)
    rows = [np.full((E, N), 0.5, np.float32),                      # all equal: order = ticker index (buys)
            np.full((E, N), -0.5, np.float32),                     # ... (sells)
            np.zeros((E, N), np.float32),                          # +0.0
            -np.zeros((E, N), np.float32),                         # -0.0
            np.where(rng.random((E, N)) < 0.5, 0.0, -0.0).astype(np.float32),
            (rng.uniform(-0.999, 0.999, (E, N)) * sub).astype(np.float32),   # |a * hmax| < 1: truncates to 0
            np.broadcast_to(rng.uniform(-1, 1, (E, 1)).astype(np.float32), (E, N)).copy()]   # equal per env
    assert np.signbit(rows[3]).all() and (adc.scaled(rows[5], hmax) == 0).all()
    return rows


@pytest.mark.parametrize("N", [7, 30, 32])
def test_key_edge_cases(N):
    _need_gpu()
    E, hmax = 130, 128
    rng = np.random.default_rng(N)
    rows = _edge_actions(E, N, hmax)
    kw = dict(hmax=hmax, initial_amount=30_000 * rng.uniform(0.5, 1.5, E),
              num_stock_shares=rng.integers(0, 200, (E, N)))
    env, orc = _make(_panel(N, len(rows) + 3), E, **kw)
    for s, a in enumerate(rows + rows[:4]):                 # the first rows again across the episode end
        _step_and_compare(env, orc, a, f"row {s}")


@pytest.mark.parametrize("case", ["boundary", "inside", "beyond"])
def test_action_domain_values(case):
    """The values of tests/test_gpu_stock_action_domain.py on per-env books: truncation boundaries, scaled
    magnitudes up to the clamp (2^25 for <= 32 tickers), and past it (the oracle on saturated actions)."""
    _need_gpu()
    E, N, T, hmax, amax = 130, 30, 6, 128, 1 << 25
    steps = 2 * T
    if case == "boundary":
        act = adc.boundary_tiles(hmax, E, N, steps, seed=5)
        fed = act
        rng = np.random.default_rng(5)
        kw = dict(hmax=hmax, initial_amount=1_000_000, num_stock_shares=rng.integers(0, 40, (E, N)))
    else:
        mags = adc.magnitudes_inside(amax) if case == "inside" else adc.magnitudes_beyond(amax)
        act, _ = adc.big_tiles(mags, hmax, E, N, steps, seed=6)
        fed = adc.saturated(act, hmax, amax)
        cash0, shares0 = adc.env_books(E, N, seed=6)
        kw = dict(hmax=hmax, initial_amount=cash0, num_stock_shares=shares0)
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    panel = _panel(N, T)
    env = VecStockTradingEnv(StockPanel(*panel), E, **kw)
    orc = StockOracle(*panel, n_envs=E, **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    for s in range(steps):
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(act[s]).cuda())
        o_obs, o_rew, o_done, _ = orc.vec_step(fed[s])
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done, err_msg=f"step {s}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32), err_msg=f"step {s}")
        np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32), err_msg=f"step {s}")
        st, os_ = env.state_numpy(), orc.state()
        for k in ("cash", "shares", "cost", "trades"):
            np.testing.assert_array_equal(st[k], os_[k], err_msg=f"{k} step {s}")


@pytest.mark.parametrize("stats", [True, False])
def test_turbulent_and_calm_days(stats):
    """A threshold at the median of the risk column: some days sell everything, others trade."""
    _need_gpu()
    E, N, T = 130, 30, 9
    panel = _panel(N, T)
    thr = float(np.median(panel[2]))
    assert (panel[2][1:] >= thr).any() and (panel[2][1:] < thr).any()
    rng = np.random.default_rng(3)
    env, orc = _make(panel, E, hmax=100, initial_amount=40_000 * rng.uniform(0.5, 1.5, E),
                     num_stock_shares=rng.integers(0, 50, (E, N)), turbulence_threshold=thr, track_stats=stats)
    seen = set()
    for s in range(2 * T + 1):
        _step_and_compare(env, orc, rng.uniform(-1, 1, (E, N)).astype(np.float32), f"step {s}")
        seen |= set((orc.state()["turbulence"] >= thr).tolist())
    assert seen == {True, False}


def test_window_ends_on_different_steps_in_one_block():
    """Per-env windows of 2 .. 7 rows inside each block: terminal lanes beside trading ones every step."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, N, T = 130, 30, 12
    close, tech, risk = _panel(N, T)
    rng = np.random.default_rng(4)
    length = 2 + np.arange(E) % 6
    start = rng.integers(0, T - 7, E)
    kw = dict(hmax=100, initial_amount=60_000)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, windows=(start, start + length), **kw)
    orcs = [StockOracle(close[a:a + n], tech[a:a + n], risk[a:a + n], n_envs=1, **kw) for a, n in zip(start, length)]
    np.testing.assert_array_equal(env.reset().cpu().numpy(),
                                  np.concatenate([o.reset() for o in orcs]).astype(np.float32))
    for s in range(9):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(a).cuda())
        out = [o.vec_step(a[e:e + 1]) for e, o in enumerate(orcs)]
        done = np.array([x[2][0] for x in out])
        assert 0 < done[:64].sum() < 64 or s == 0
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), done, err_msg=f"step {s}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), np.array([x[1][0] for x in out]).astype(np.float32))
        np.testing.assert_array_equal(g_obs.cpu().numpy(), np.concatenate([x[0] for x in out]).astype(np.float32))
        st = env.state_numpy()
        np.testing.assert_array_equal(st["cash"], np.array([o.state()["cash"][0] for o in orcs]))
        np.testing.assert_array_equal(st["shares"], np.concatenate([o.state()["shares"] for o in orcs]))


def test_out_of_step_batch_without_the_hint():
    """Per-env start days and NO desynchronised hint: the three-wave kernel on lanes that are terminal on
    different steps (per-lane `term`), turbulent on different days, with per-env panel rows."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, N, T = 130, 30, 10
    close, tech, risk = _panel(N, T)
    thr = float(np.median(risk))
    rng = np.random.default_rng(8)
    kw = dict(hmax=100, initial_amount=50_000, num_stock_shares=rng.integers(0, 30, N), turbulence_threshold=thr)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    env.enable_terminal_obs()
    offs = rng.integers(0, T - 1, E).astype(np.int32)
    for k in ("day", "price_day", "start_day"):
        env.state[k].copy_(torch.from_numpy(offs).cuda())
    env.refresh()
    orcs = [StockOracle(close, tech, risk, n_envs=1, day=int(d), **kw) for d in offs]
    ends, mixed = np.zeros(E, np.int64), 0
    for s in range(T + 3):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(a).cuda())
        out = [o.vec_step(a[e:e + 1]) for e, o in enumerate(orcs)]
        done = np.array([x[2][0] for x in out])
        mixed += int(0 < done[:64].sum() < 64)
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), done, err_msg=f"step {s}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), np.array([x[1][0] for x in out]).astype(np.float32),
                                      err_msg=f"step {s}")
        np.testing.assert_array_equal(g_obs.cpu().numpy(), np.concatenate([x[0] for x in out]).astype(np.float32),
                                      err_msg=f"step {s}")
        if done.any():
            np.testing.assert_array_equal(env.term_obs.cpu().numpy()[done],
                                          np.concatenate([x[3] for x in out])[done].astype(np.float32))
        st = env.state_numpy()
        for k in ("cash", "shares", "cost", "trades", "day", "turbulence"):
            np.testing.assert_array_equal(st[k], np.concatenate([np.atleast_1d(o.state()[k]) for o in orcs]),
                                          err_msg=f"{k} step {s}")
        ends += done
    assert (ends >= 1).all() and mixed >= 3


def test_graph_capture_replays_equal_eager():
    """Four steps in one captured graph, replayed twice: the sorter's flag is cleared by every launch."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    E, N, T, S = 130, 30, 7, 4
    panel = StockPanel(*_panel(N, T))
    rng = np.random.default_rng(9)
    kw = dict(hmax=100, initial_amount=40_000 * rng.uniform(0.5, 1.5, E), num_stock_shares=rng.integers(0, 30, (E, N)))
    cap, eager = VecStockTradingEnv(panel, E, **kw), VecStockTradingEnv(panel, E, **kw)
    for env in (cap, eager):
        env.reset()
    pool = [torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda() for _ in range(S)]
    hist = {k: torch.zeros((S,) + tuple(v.shape), dtype=v.dtype, device="cuda")
            for k, v in (("obs", cap.obs), ("reward", cap.reward), ("done", cap.done))}
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
            for k, v in (("obs", o), ("reward", r), ("done", d)):
                hist[k][i].copy_(v)
    for rep in range(2):
        graph.replay()
        ref = {k: [] for k in hist}
        for i in range(S):
            o, r, d, _ = eager.step(pool[i])
            for k, v in (("obs", o), ("reward", r), ("done", d)):
                ref[k].append(v.clone())
        torch.cuda.synchronize()
        for k in hist:
            np.testing.assert_array_equal(hist[k].cpu().numpy(), torch.stack(ref[k]).cpu().numpy(),
                                          err_msg=f"{k} replay {rep}")
        cs, es = cap.state_numpy(), eager.state_numpy()
        for k in ("cash", "shares", "day", "trades"):
            np.testing.assert_array_equal(cs[k], es[k], err_msg=f"{k} replay {rep}")
    assert hist["done"].any()


def test_second_round_of_a_large_batch():
    """65,536 + 64 envs: more blocks than one resident round, so the step is two launches and the second
    one's blocks start at `block_base`.  Sampled envs of both rounds against the oracle, three steps."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, N, T = 65_536 + 64, 30, 6
    panel = _panel(N, T)
    rng = np.random.default_rng(10)
    env = VecStockTradingEnv(StockPanel(*panel), E, hmax=100, initial_amount=50_000)
    sample = np.unique(np.concatenate([np.arange(66), rng.integers(0, E, 60), [E // 2 - 1, E // 2, E // 2 + 64],
                                       np.arange(E - 66, E)]))
    orc = StockOracle(*panel, n_envs=len(sample), hmax=100, initial_amount=50_000)
    np.testing.assert_array_equal(env.reset().cpu().numpy()[sample], orc.reset().astype(np.float32))
    for s in range(3):
        a = torch.rand(E, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(s)) * 2 - 1
        g_obs, g_rew, g_done, _ = env.step(a)
        o_obs, o_rew, o_done, _ = orc.vec_step(a[torch.from_numpy(sample).cuda()].cpu().numpy())
        np.testing.assert_array_equal(g_obs.cpu().numpy()[sample], o_obs.astype(np.float32), err_msg=f"step {s}")
        np.testing.assert_array_equal(g_rew.cpu().numpy()[sample], o_rew.astype(np.float32), err_msg=f"step {s}")
        st, os_ = env.state_numpy(), orc.state()
        np.testing.assert_array_equal(st["cash"][sample], os_["cash"])
        np.testing.assert_array_equal(st["shares"][sample], os_["shares"])
        assert np.isfinite(g_obs.cpu().numpy()).all() and (st["day"] == s + 1).all()
