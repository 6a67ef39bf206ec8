"""The last-episode block (finenv_{stock,portfolio}_set_last_episode) on the MI355X: the step that
reports done latches the finished episode's summary before the auto-reset replaces the state.

Yardsticks: the CPU oracle's episode_stats() taken just before that step, a twin env stepped with
gym semantics (auto_reset=False) whose current-state episode_stats() must equal the latched row bit
for bit, and the reference fixtures under tests/golden/."""
import ctypes as C
import glob
import os
import socket

import numpy as np
import pytest

from _golden import StockFixture, stock_fixture_names

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(seed, T, N, K, flag_frac=0.03):
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.015, (T, N)), axis=0))
    tech = rng.normal(0, 1, (T, K, N))
    if K:
        tech[:, 0, :][rng.random((T, N)) < flag_frac] = 1.0
    risk = np.abs(rng.normal(0, 30, T))
    return close, tech, risk


def _check_latched(g, o, stats, what):
    """latched rows g vs the oracle's pre-step episode_stats o: columns 0-4 bit for bit; Sharpe as
    test_gpu_stock_parity does, or NaN when the GPU keeps no return sums."""
    np.testing.assert_array_equal(g[:, :5], o[:, :5], err_msg=what)
    if stats:
        np.testing.assert_allclose(g[:, 5], o[:, 5], rtol=1e-9, atol=1e-12, equal_nan=True,
                                   err_msg=what)
    else:
        assert np.isnan(g[:, 5]).all(), what


@pytest.mark.parametrize("N,K,thr,stats", [(7, 3, None, True), (30, 8, 45.0, True),
                                           (30, 8, None, False), (50, 2, 40.0, True),
                                           (100, 3, None, True), (100, 3, 40.0, False)])
def test_stock_latch_matches_oracle_and_twin(N, K, thr, stats):
    """Lock-step batch of E = 200 (a partial last wave), distinct random actions per env, three
    episode ends: every latched row equals the oracle's terminal summary and the episode_stats() of
    a gym-semantics twin bit for bit; COUNT / EPISODE count right; the gathered return is the
    finished episode's, not the post-reset 1.0."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, T = 200, 9
    rng = np.random.default_rng(N * 7 + K)
    close, tech, risk = _panel(N, T, N, K)
    kw = dict(hmax=60, initial_amount=200_000 * rng.uniform(0.5, 1.5, E),
              num_stock_shares=rng.integers(0, 10, (E, N)), buy_cost_pct=0.0013,
              sell_cost_pct=0.0007, turbulence_threshold=thr)
    panel = StockPanel(close, tech, risk)
    env = VecStockTradingEnv(panel, E, auto_reset=True, track_stats=stats, **kw)
    twin = VecStockTradingEnv(panel, E, auto_reset=False, track_stats=stats, **kw)
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    blk = env.enable_last_episode()
    assert env.enable_last_episode() is blk                       # idempotent
    assert np.isnan(env.last_episode_stats().cpu().numpy()).all()  # nothing finished yet
    orc.reset(); env.reset(); twin.reset()
    n_done = 0
    for s in range(3 * T):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        pre, ep_pre = orc.episode_stats(), orc.state()["episode"]
        orc.vec_step(a, want_obs=False)
        at = torch.from_numpy(a).cuda()
        _, _, done, _ = env.step(at)
        _, _, tdone, _ = twin.step(at)
        done = done.cpu().numpy().astype(bool)
        assert done.all() or not done.any()                       # lock-step batch
        if not done.any():
            continue
        n_done += 1
        g = env.last_episode_stats().cpu().numpy()
        _check_latched(g, pre, stats, f"step {s}")
        np.testing.assert_array_equal(twin.episode_stats().cpu().numpy(), g)   # NaN positions too
        le = {k: v.cpu().numpy() for k, v in env.last_episode.items()}
        assert (le["count"] == n_done).all()
        np.testing.assert_array_equal(le["episode"], ep_pre)
        assert (le["ret_n"] == T - 1).all()
        r = env.last_episode_return().cpu().numpy()
        assert r.dtype == np.float32 and r.shape == (E,)
        np.testing.assert_array_equal(r, (pre[:, 1] / pre[:, 0]).astype(np.float32))
        assert len(np.unique(r)) > E // 2 and not (r == 1.0).any()
        twin.reset()
    assert n_done == 3


@pytest.mark.parametrize("name", stock_fixture_names())
def test_stock_latch_matches_reference_fixture(name):
    """The recorded reference runs, replayed with auto_reset=True on E = 130 identical envs: each
    latched row carries asset_memory[0], the end asset asset_memory[-1], cost, trades and Sharpe of
    the episode the reference printed."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    fx = StockFixture(name)
    z = fx.z
    E = 130
    env = VecStockTradingEnv(StockPanel(fx.close, fx.tech, fx.risk), E, auto_reset=True,
                             **fx.env_kwargs())
    env.enable_last_episode()
    if -1 in z["reset_step"].tolist():
        env.reset()
    tj = 0
    for s in range(fx.S):
        a = torch.from_numpy(np.broadcast_to(fx.actions[s], (E, fx.N)).copy()).cuda()
        _, _, done, _ = env.step(a)
        assert bool(done[0]) == bool(z["done"][s]), s
        if not z["done"][s]:
            continue
        g = env.last_episode_stats().cpu().numpy()
        assert (g == g[0]).all() or np.isnan(g[:, 5]).all()
        am = z[f"asset_memory_{tj}"]
        assert g[0, 0] == am[0] and g[E - 1, 0] == am[0], (s, g[0, 0], am[0])
        assert g[0, 1] == am[-1] and g[E - 1, 1] == am[-1], (s, g[0, 1], am[-1])
        assert g[0, 3] == z["cost"][s] and g[0, 4] == z["trades"][s]
        sh = fx.sharpe(tj)
        if np.isnan(sh):
            assert np.isnan(g[0, 5])
        else:
            assert g[0, 5] == pytest.approx(sh, rel=1e-9, abs=1e-12)
        assert (env.last_episode["count"] == tj + 1).all()
        tj += 1
    assert tj >= 1


@pytest.mark.parametrize("N,hint", [(30, True), (30, False), (100, True)])
def test_stock_latch_desynchronised_masked_resets(N, hint):
    """Masked host resets drive the batch out of lock step: episodes end on different steps and
    each latches its own summary; a host reset leaves the block untouched."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle, lib, _p
    E, T, K = 200, 14, 3
    close, tech, risk = _panel(5, T, N, K)
    rng = np.random.default_rng(9)
    kw = dict(hmax=100, initial_amount=300_000, turbulence_threshold=50.0)
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, auto_reset=True, **kw)
    env.hint_desynchronised(hint)
    env.enable_last_episode()
    orc.reset(); env.reset()
    count = np.zeros(E)
    partial_done_steps = 0
    for s in range(40):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        pre, ep_pre = orc.episode_stats(), orc.state()["episode"]
        _, _, o_done, _ = orc.vec_step(a, want_obs=False)
        _, _, g_done, _ = env.step(torch.from_numpy(a).cuda())
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done)
        if o_done.any():
            partial_done_steps += int(not o_done.all())
            count[o_done] += 1
            g = env.last_episode_stats().cpu().numpy()
            _check_latched(g[o_done], pre[o_done], True, f"step {s}")
            np.testing.assert_array_equal(env.last_episode["episode"].cpu().numpy()[o_done],
                                          ep_pre[o_done])
        np.testing.assert_array_equal(env.last_episode["count"].cpu().numpy(), count)
        if s in (3, 7, 12, 20):
            m = rng.random(E) < 0.3
            for e in np.nonzero(m)[0]:
                row = np.empty(orc.D)
                lib().stock_oracle_reset_env(orc._h, C.c_int(int(e)), _p(row))
            before = env.last_episode_stats().cpu().numpy().copy()
            blk = env._last.cpu().numpy().copy()
            env.reset(torch.from_numpy(m.astype(np.uint8)).cuda())
            np.testing.assert_array_equal(env._last.cpu().numpy(), blk)
            np.testing.assert_array_equal(env.last_episode_stats().cpu().numpy(), before)
    assert partial_done_steps >= 2 and count.min() >= 1


def test_stock_latch_batch_larger_than_one_round():
    """N = 30, E = 69,700: more 64-env groups than one resident round (several launches per step);
    latched rows of envs sampled around every possible round boundary vs the oracle."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    N, E, T, K = 30, 69_700, 9, 2
    rng = np.random.default_rng(N + E)
    close, tech, risk = _panel(3, T, N, K)
    kw = dict(hmax=40, initial_amount=60_000, turbulence_threshold=45.0)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    env.enable_last_episode()
    sample = np.unique(np.concatenate([[0, 63, 64, E - 1, E - 2, E // 2, E // 2 + 1],
                                       rng.choice(E, 250, replace=False)]))
    blocks = (E + 63) // 64
    for k in (2, 3):
        chunk = (blocks + k - 1) // k
        for b in range(chunk, blocks, chunk):
            sample = np.union1d(sample, [min(E - 1, 64 * b - 1), min(E - 1, 64 * b), min(E - 1, 64 * b + 63)])
    orc = StockOracle(close, tech, risk, n_envs=len(sample), **kw)
    orc.reset(); env.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(E)
    n_done = 0
    for s in range(2 * T + 1):
        a = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
        pre = orc.episode_stats()
        _, _, done, _ = env.step(a)
        _, _, o_done, _ = orc.vec_step(a[sample].cpu().numpy(), want_obs=False)
        if o_done.any():
            n_done += 1
            assert int(done.sum()) == E
            g = env.last_episode_stats()
            _check_latched(g[sample].cpu().numpy(), pre, True, f"step {s}")
            assert bool((env.last_episode["count"] == n_done).all())
            assert bool(torch.isfinite(g[:, :5]).all())
    assert n_done == 2


@pytest.mark.parametrize("N,stats", [(30, True), (30, False), (50, True), (100, False)])
def test_stock_block_has_no_effect_on_results(N, stats):
    """Same inputs with the block enabled and disabled, over two episodes: every output and both
    state blocks bit-identical."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T, K = 150, 7, 2
    close, tech, risk = _panel(11, T, N, K)
    panel = StockPanel(close, tech, risk)
    kw = dict(hmax=50, initial_amount=100_000, turbulence_threshold=40.0, track_stats=stats)
    envs = [VecStockTradingEnv(panel, E, **kw) for _ in range(2)]
    for env in envs:
        env.enable_terminal_obs()
        env.enable_realised()
        env.reset()
    envs[0].enable_last_episode()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(N)
    n_done = 0
    for s in range(2 * T):
        a = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
        outs = [env.step(a)[:3] for env in envs]
        for x, y in zip(*outs):
            assert torch.equal(x, y), s
        n_done += int(outs[0][2].any())
        a_, b_ = envs
        assert torch.equal(a_.term_obs, b_.term_obs) and torch.equal(a_.realised, b_.realised)
        assert torch.equal(a_._state_f64, b_._state_f64) and torch.equal(a_._state_i32, b_._state_i32)
    assert n_done == 2


def test_stock_block_under_graph_capture():
    """A segment containing an episode end, captured in a hipGraph with the block enabled before
    the capture: the replay equals the eager run bit for bit, block included."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    rng = np.random.default_rng(2)
    T, N, K, E = 6, 30, 2, 200
    close, tech, risk = _panel(2, T, N, K)
    panel = StockPanel(close, tech, risk)
    a_env = VecStockTradingEnv(panel, E, hmax=30, initial_amount=40_000)
    b_env = VecStockTradingEnv(panel, E, hmax=30, initial_amount=40_000)
    for env in (a_env, b_env):
        env.enable_last_episode()
    acts = [torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda() for _ in range(8)]
    a_env.reset(); b_env.reset()
    b_env.step(acts[0]); a_env.step(acts[0])         # eager warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(1, 8):
            b_env.step(acts[t])
    for k, v in a_env.state.items():                 # the capture ran nothing: align b, then replay
        b_env.state[k].copy_(v)
    b_env.obs.copy_(a_env.obs)
    b_env._last.copy_(a_env._last)
    for t in range(1, 8):
        a_env.step(acts[t])
    g.replay()
    torch.cuda.synchronize()
    assert int(a_env.last_episode["count"].min()) == 1     # the segment crossed an episode end
    assert torch.equal(a_env.obs, b_env.obs) and torch.equal(a_env.reward, b_env.reward)
    for k in a_env.state:
        assert torch.equal(a_env.state[k], b_env.state[k]), k
    np.testing.assert_array_equal(a_env._last.cpu().numpy(), b_env._last.cpu().numpy())


def test_sb3_adapter_episode_summary():
    """infos[i]["episode_summary"] exactly for done envs, equal to the latched row under the
    reference's printed names; no SB3 "episode" key."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, T, N, K = 70, 8, 7, 2
    rng = np.random.default_rng(3)
    close, tech, risk = _panel(4, T, N, K)
    kw = dict(hmax=30, initial_amount=50_000 * rng.uniform(0.5, 1.5, E))
    venv = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw).as_sb3_vec_env()
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    venv.reset(); orc.reset()
    keys = ["begin_total_asset", "end_total_asset", "total_reward", "total_cost", "total_trades",
            "sharpe"]
    n_done = 0
    for s in range(2 * T):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        pre = orc.episode_stats()
        orc.vec_step(a, want_obs=False)
        _, _, done, infos = venv.step(a)
        for i in range(E):
            assert ("episode_summary" in infos[i]) == bool(done[i]) and "episode" not in infos[i]
        if done.any():
            n_done += 1
            row = venv.env.last_episode_stats().cpu().numpy()
            for i in np.nonzero(done)[0]:
                summ = infos[i]["episode_summary"]
                assert list(summ) == keys
                np.testing.assert_array_equal(np.array([summ[k] for k in keys]), row[i])
                assert summ["begin_total_asset"] == pre[i, 0] and summ["end_total_asset"] == pre[i, 1]
                assert summ["total_trades"] == pre[i, 4]
    assert n_done == 2


# ------------------------------------------------------------------------------------ portfolio
def _pf_inputs(seed, T, N, K):
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    return close, rng.normal(0, 1e-4, (T, N, N)), rng.normal(0, 1, (T, K, N))


def _sharpe_pd(rets):
    """pandas' Sharpe over portfolio_return_memory = [0] + returns (env_portfolio.py:146-153)."""
    import pandas as pd
    s = pd.Series([0.0] + list(rets))
    return np.nan if s.std() == 0 else (252 ** 0.5) * s.mean() / s.std()


def test_portfolio_latch_sums_and_twin():
    """Running sums recomputed in numpy from the GPU's own weights and gross returns, in the
    kernel's order: RET_N / RET_SUM / RET_SUMSQ bit for bit; END equals an auto_reset=False twin's
    terminal value; Sharpe equals pandas' over [0] + returns."""
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    E, T, N, K = 130, 12, 7, 3
    close, cov, tech = _pf_inputs(5, T, N, K)
    panel = PortfolioPanel(close, cov, tech)
    env = VecStockPortfolioEnv(panel, E, initial_amount=1e6, auto_reset=True)
    twin = VecStockPortfolioEnv(panel, E, initial_amount=1e6, auto_reset=False)
    env.enable_weights()
    env.enable_last_episode()
    assert np.isnan(env.last_episode_stats().cpu().numpy()).all()
    env.reset(); twin.reset()
    gr = env._panel_t["gross_ret"].cpu().numpy()
    rng = np.random.default_rng(1)
    s1, s2 = np.zeros(E), np.zeros(E)
    rets = [[] for _ in range(E)]
    n_done = 0
    for s in range(3 * T):
        day = env.state["day"].cpu().numpy().copy()
        a = torch.from_numpy(rng.uniform(0, 1, (E, N)).astype(np.float32)).cuda()
        _, _, done, _ = env.step(a)
        twin.step(a)
        done = done.cpu().numpy().astype(bool)
        if not done.any():
            w = env.weights.cpu().numpy().astype(np.float64)
            r = np.zeros(E)
            for i in range(N):
                r = r + gr[day, i] * w[:, i]
            s1, s2 = s1 + r, s2 + r * r
            for e in range(E):
                rets[e].append(r[e])
            np.testing.assert_array_equal(env.last_episode["run_sum"].cpu().numpy(), s1)
            continue
        assert done.all()
        n_done += 1
        le = {k: v.cpu().numpy() for k, v in env.last_episode.items()}
        assert (le["count"] == n_done).all() and (le["ret_n"] == T).all()
        np.testing.assert_array_equal(le["ret_sum"], s1)
        np.testing.assert_array_equal(le["ret_sumsq"], s2)
        np.testing.assert_array_equal(le["end_value"], twin.state["value"].cpu().numpy())
        assert (le["begin_value"] == 1e6).all() and (le["run_sum"] == 0).all()
        g = env.last_episode_stats().cpu().numpy()
        np.testing.assert_array_equal(g[:, 1], le["end_value"])
        for e in (0, 63, 64, E - 1):
            assert g[e, 2] == pytest.approx(_sharpe_pd(rets[e]), rel=1e-6)
        r = env.last_episode_return().cpu().numpy()
        assert len(np.unique(r)) > E // 2 and not (r == 1.0).any()
        s1, s2 = np.zeros(E), np.zeros(E)
        rets = [[] for _ in range(E)]
        twin.reset()
    assert n_done == 3


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[len("portfolio_"):-4]
                                        for p in glob.glob(os.path.join(GOLDEN, "portfolio_*.npz"))
                                        if not p.endswith("portfolio_domain.npz")))
def test_portfolio_latch_matches_reference_fixture(name):
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    z = np.load(os.path.join(GOLDEN, f"portfolio_{name}.npz"), allow_pickle=False)
    T, N, K, S = z["cfg_int"].tolist()
    cash = float(z["cfg_float"][0])
    E = 70
    env = VecStockPortfolioEnv(PortfolioPanel(z["close"], z["cov"], z["tech"]), E,
                               initial_amount=cash, auto_reset=True)
    env.enable_last_episode()
    env.reset()
    prev, rets, nd = cash, [], 0
    for s in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][s], (E, N)).copy()).cuda()
        _, _, done, _ = env.step(a)
        assert bool(done[0]) == bool(z["done"][s])
        if not z["done"][s]:
            rets.append(z["value"][s] / prev - 1.0)
            prev = z["value"][s]
            continue
        nd += 1
        g = env.last_episode_stats().cpu().numpy()
        assert (g == g[0]).all()
        assert g[0, 0] == cash
        assert g[0, 1] == pytest.approx(z["value"][s], rel=1e-6)
        assert g[0, 2] == pytest.approx(_sharpe_pd(rets), rel=1e-6)
        prev, rets = cash, []
    assert nd == 2


def test_portfolio_masked_reset_clears_running_sums():
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    E, T, N, K = 100, 10, 5, 2
    env = VecStockPortfolioEnv(PortfolioPanel(*_pf_inputs(8, T, N, K)), E)
    env.enable_last_episode()
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(4):
        env.step(torch.from_numpy(rng.uniform(0, 1, (E, N)).astype(np.float32)).cuda())
    run = env.last_episode["run_sum"].cpu().numpy().copy()
    assert (run != 0).all()
    m = rng.random(E) < 0.4
    blk = env._last.cpu().numpy().copy()
    env.reset(torch.from_numpy(m.astype(np.uint8)).cuda())
    after = env._last.cpu().numpy()
    j = {k: i for i, k in enumerate(env.last_episode)}
    for k in ("run_sum", "run_sumsq"):
        assert (after[j[k]][m] == 0).all()
        np.testing.assert_array_equal(after[j[k]][~m], blk[j[k]][~m])
    for k in ("count", "begin_value", "end_value", "ret_n", "ret_sum", "ret_sumsq"):
        np.testing.assert_array_equal(after[j[k]], blk[j[k]])


# ------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_inputs():
    rng = np.random.default_rng(42)
    T, N, K, E = 8, 30, 2, 140
    close, tech, risk = _panel(42, T, N, K)
    kw = dict(initial_amount=1e6 * rng.uniform(0.5, 1.5, E), hmax=80)
    acts = rng.uniform(-1, 1, (T + 2, E, N)).astype(np.float32)
    return (close, tech, risk), kw, E, acts


def _dist_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from finrl_amd import StockPanel
    from finrl_amd.distributed import gather_episode_returns, make_sharded_env, shard_range
    data, kw, E, acts = _dist_inputs()
    env = make_sharded_env(StockPanel(*data), E, kind="stock", rank=rank, world=world,
                           device="cuda:0", **kw)
    env.enable_last_episode()
    lo, hi = shard_range(E, rank, world)
    env.reset()
    for a in acts:
        env.step(torch.from_numpy(a[lo:hi].copy()).cuda())
    ret = gather_episode_returns(env.last_episode_return(), E)
    q.put((rank, ret.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gather_the_latched_returns():
    """Two gloo ranks on one GPU step their shards through an episode end with auto-reset and
    gather last_episode_return(): the global vector equals the single-batch oracle's end / begin
    per env, in global order."""
    _need_gpu()
    import torch.multiprocessing as mp
    from oracle.stock import StockOracle
    data, kw, E, acts = _dist_inputs()
    orc = StockOracle(*data, n_envs=E, **kw)
    orc.reset()
    last = None
    for a in acts:
        pre = orc.episode_stats()
        _, _, done, _ = orc.vec_step(a, want_obs=False)
        if done.any():
            assert done.all()
            last = (pre[:, 1] / pre[:, 0]).astype(np.float32)
    assert last is not None
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank in (0, 1):
        np.testing.assert_array_equal(res[rank], last)
    assert len(np.unique(last)) > E // 2
