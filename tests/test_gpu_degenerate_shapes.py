"""Smallest shapes the kernels accept: one env, one asset, two days, no indicator columns -- a single
partially filled wave per launch, panels of two rows, episodes that end on the first step."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.mark.parametrize("E,T,N,K", [(1, 2, 1, 0), (1, 3, 2, 1), (3, 2, 30, 8), (2, 2, 100, 1)])
def test_stock_env_smallest_shapes(E, T, N, K):
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    rng = np.random.default_rng(E + T + N)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    tech = rng.normal(0, 1, (T, K, N))
    risk = np.abs(rng.normal(0, 30, T))
    kw = dict(hmax=50, initial_amount=20_000, turbulence_threshold=60.0)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    for s in range(3 * T):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        obs, rew, done, _ = env.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, o_done, _ = orc.vec_step(a)
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs.astype(np.float32), err_msg=f"{s}")
        np.testing.assert_array_equal(rew.cpu().numpy(), o_rew.astype(np.float32))
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), o_done)


@pytest.mark.parametrize("kind", ["cashpenalty", "stoploss"])
@pytest.mark.parametrize("E,T,N,C", [(1, 2, 1, 0), (1, 3, 1, 1), (2, 4, 2, 3)])
def test_cashpenalty_stoploss_smallest_shapes(kind, E, T, N, C):
    _need_gpu()
    from finrl_amd.vec_cashpenalty import CashPenaltyPanel, VecCashPenaltyEnv, VecStopLossEnv
    from oracle.cashpenalty import CashPenaltyOracle
    from oracle.stoploss import StopLossOracle
    rng = np.random.default_rng(E + T + N + C)
    close = 50 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    info = rng.normal(0, 10, (T, N, C))
    kw = dict(hmax=5_000, initial_amount=1e5)
    cls, ocls = (VecCashPenaltyEnv, CashPenaltyOracle) if kind == "cashpenalty" else \
        (VecStopLossEnv, StopLossOracle)
    env = cls(CashPenaltyPanel(close, info), E, random_start=False, **kw)
    orc = ocls(close, info, None, n_envs=E, **kw)
    starts = np.zeros(E, np.int32)
    env.set_next_start(starts)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset(starts).astype(np.float32))
    for s in range(3 * T):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        env.set_next_start(starts)
        o_obs, o_rew, o_done, _ = orc.vec_step(a, starts)
        obs, rew, done, _ = env.step(torch.from_numpy(a).cuda())
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), o_done, err_msg=f"{s}")
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs.astype(np.float32))
        np.testing.assert_array_equal(rew.cpu().numpy(), o_rew.astype(np.float32))


def test_crypto_and_stocknp_single_env():
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    from oracle.crypto import CryptoOracle
    rng = np.random.default_rng(3)
    T, N, W = 8, 1, 2
    price = 100 * np.exp(np.cumsum(rng.normal(0, 0.004, (T, N)), axis=0))
    tech = rng.normal(0, 3000, (T, W))
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, 1, lookback=1)
    orc = CryptoOracle(price, tech, n_envs=1, lookback=1)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset())
    for s in range(2 * T):
        a = rng.uniform(-1, 1, (1, N)).astype(np.float32)
        obs, rew, done, _ = env.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, o_done, _ = orc.vec_step(a)
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs, err_msg=f"{s}")
        np.testing.assert_array_equal(rew.cpu().numpy(), o_rew.astype(np.float32))
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), o_done)
    cfg = {"price_array": price.astype(np.float32), "tech_array": rng.normal(0, 50, (T, N * 2)).astype(np.float32),
           "turbulence_array": np.abs(rng.normal(0, 20, T)).astype(np.float32), "if_train": False}
    np_env = VecStockTradingEnvNP(cfg, 1)
    o = np_env.reset()
    assert o.shape == (1, 3 + 3 * N + 2 * N) and bool(torch.isfinite(o).all())
    for s in range(T + 2):
        o, r, d, _ = np_env.step(torch.rand(1, N, device="cuda") * 2 - 1)
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(r).all())


def _btc_run(env, mb, a_of, steps, auto_reset):
    """reset, then `steps` steps of a batched BitcoinEnv against one tests/btc_model.py model per env,
    bit for bit; a step past the end (auto_reset off) is the defined no-trade step, then reset()."""
    import btc_model as bm
    term = env.enable_terminal_obs()
    np.testing.assert_array_equal(bm.bits(env.reset().cpu().numpy()), bm.bits(np.stack(list(mb.reset().values()))))
    bm.assert_state_equal(env.state_numpy(), mb.state(), "reset")
    first = {k: v.copy() for k, v in mb.state().items()}
    ends = np.zeros(env.num_envs, int)
    for k in range(steps):
        a = a_of(k)
        past = mb.state()["day"] >= np.array([m.end - 1 for m in mb.m])
        before = env.state_numpy()
        obs_before = env.obs.clone()
        got = env.step(torch.from_numpy(a[:, None]).cuda())
        want = mb.step(a, auto_reset)
        st = bm.assert_step_equal(env, got, want, f"step {k}")
        bm.assert_state_equal(st, mb.state(), f"step {k}")
        if past.any():                                            # auto_reset off, stepped on the terminal row
            assert not auto_reset and past.all() and want[2].all() and (want[1] == 0).all()
            assert torch.equal(got[0], obs_before) and (st["last_reward"] == 0).all()
            bm.assert_state_equal(st, before, f"past the end {k}")
            obs = env.reset().cpu().numpy()
            np.testing.assert_array_equal(bm.bits(obs), bm.bits(np.stack(list(mb.reset().values()))))
            bm.assert_state_equal(env.state_numpy(), mb.state(), f"reset after {k}")
            continue
        bm.assert_terminal_rows(term, want, f"step {k}")          # the row the reference's step() returned
        ends += want[2]
        done = want[2]
        if auto_reset and done.any():                             # the env stands where reset() puts it
            for f in ("account", "stocks", "total_asset", "stocks_tag", "day"):
                np.testing.assert_array_equal(st[f][done], first[f][done], err_msg=f"step {k}: {f}")
            assert (st["stocks_tag"][done] == bm.PY).all()
    return ends


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "manual"])
@pytest.mark.parametrize("E,T,P,W", [(1, 2, 1, 7), (1, 3, 1, 12), (3, 2, 2, 7), (65, 2, 245, 7)])
def test_btc_env_smallest_shapes(E, T, P, W, auto_reset):
    """One env, two-row panels -- every step is terminal --, more indicator columns than rows, and one
    full wave plus one lane at the widest row."""
    _need_gpu()
    import btc_model as bm
    from finrl_amd.vec_btc import VecBitcoinEnv
    rng = np.random.default_rng(1000 * E + 10 * T + P)
    p0 = 300.0 * np.exp(np.cumsum(rng.normal(0, 0.01, T)))
    price = np.ascontiguousarray(np.stack([p0 * (1 + 0.002 * k) for k in range(P)], 1))
    tech = rng.normal(0, 3e3, (T, W))
    kw = dict(initial_account=1e3, transaction_fee_percent=1e-3, gamma=0.99)
    env = VecBitcoinEnv(price, tech, E, auto_reset=auto_reset, **kw)
    assert env.obs_dim == P + 9 and env.max_step == T
    ends = _btc_run(env, bm.ModelBatch(price, tech, E, **kw),
                    lambda k: rng.uniform(-4, 4, E).astype(np.float32), 6, auto_reset)
    assert (ends == (6 // (T - 1) if auto_reset else 6 // T)).all()


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "manual"])
def test_btc_env_two_row_windows(auto_reset):
    """Windows of length 2 at every start of a six-row panel: each env's every step is terminal, on
    its own rows."""
    _need_gpu()
    import btc_model as bm
    from finrl_amd.vec_btc import VecBitcoinEnv
    rng = np.random.default_rng(12)
    T, E = 6, 5
    price = np.ascontiguousarray((300.0 * np.exp(np.cumsum(rng.normal(0, 0.05, T))))[:, None])
    tech = rng.normal(0, 3e3, (T, 7))
    s = np.arange(E)
    kw = dict(initial_account=1e3, transaction_fee_percent=1e-3, gamma=0.99)
    env = VecBitcoinEnv(price, tech, E, auto_reset=auto_reset, windows=(s, s + 2), **kw)
    assert env.max_step == 2
    ends = _btc_run(env, bm.ModelBatch(price, tech, E, start=s, end=s + 2, **kw),
                    lambda k: rng.uniform(-4, 4, E).astype(np.float32), 6, auto_reset)
    assert (ends == (6 if auto_reset else 3)).all()
    assert len(np.unique(env.state_numpy()["day"])) == E


@pytest.mark.parametrize("E,T,N,K", [
    (1, 2, 1, 0),            # the smallest accepted shape
    (1, 1, 3, 1),            # every step is terminal: the reward is the initial last reward
    (3, 3, 2, 1),            # a small batch
    (31, 4, 7, 1),           # wave 1 of the block has no row to write
    (33, 4, 8, 0),           # wave 1 writes one row; N = 8 is the first pairwise-sum shape
    (65, 4, 15, 1), (65, 4, 16, 1), (65, 4, 17, 2),      # the tail of the pairwise sum
    (65, 3, 32, 32),         # D = 2048: all 8 register chunks of the row template
    (65, 3, 32, 33),         # D = 2080: the first width on the per-row path
    (40, 3, 64, 0),          # D = 4096
])
def test_portfolio_env_smallest_shapes(E, T, N, K):
    """`signed` / `wide` scores against PortfolioOracle with the checks of test_gpu_portfolio_domain.py
    (obs, term_obs, done, day exact; weights and value inside the derived bounds), then one masked reset
    each for a single env, the upper half-wave of block 0 and the last (partial) block: the rows of the
    envs not selected keep their observation, value and day."""
    _need_gpu()
    import portfolio_domain_cases as pc
    import test_gpu_portfolio_domain as pd
    steps = 3 * T + 2
    close, cov, tech = pc.benign_panel(T, N, K, 100 * E + 10 * T + N)
    acts = pc.actions(pc.SMALL_SHAPE_KINDS, E, N, steps, T, E + T + N + K)
    names, _ = pc.kinds_of(E, pc.SMALL_SHAPE_KINDS)
    obs0, trace = pc.oracle_trace(pd._oracle(close, cov, tech, E), acts)
    env = pd._env(close, cov, tech, E)
    assert env.state_dim == (N + K) * N
    np.testing.assert_array_equal(env.reset().cpu().numpy(), obs0.astype(np.float32))
    g = pc.gross_returns(close)
    outs = [pd.checked_step(env, acts[s], trace[s], g, names, f"step {s}") for s in range(steps)]
    assert sum(int(o["done"].all()) for o in outs) == steps // T          # (T = 1: every step)
    if T == 1:
        assert all((o["reward"] == 0).all() for o in outs)
    assert sum(o["bounded"] for o in outs) == E * (steps - steps // T) == sum(o["values"] for o in outs)
    e = np.arange(E)
    masks = [m for m in (e == 40, (e >= 32) & (e < 64), e >= (E - 1) // 64 * 64) if m.any()]
    for j, m in enumerate(masks):
        for k in range(2):             # move on until a selected env is past day 0, so that its reset shows
            if T > 1 and not (env.state_numpy()["day"][m] > 0).any():
                env.step(torch.from_numpy(acts[k]).cuda())
        before, obs_before = env.state_numpy(), env.obs.cpu().numpy().copy()
        assert T == 1 or (before["day"][m] > 0).any()
        obs = env.reset(torch.from_numpy(m.astype(np.uint8))).cpu().numpy()
        st = env.state_numpy()
        np.testing.assert_array_equal(obs[m], obs0[m].astype(np.float32), err_msg=f"mask {j}")
        assert (st["value"][m] == pd.AMOUNT).all() and (st["day"][m] == 0).all(), f"mask {j}"
        np.testing.assert_array_equal(obs[~m], obs_before[~m], err_msg=f"mask {j}")
        np.testing.assert_array_equal(st["value"][~m], before["value"][~m], err_msg=f"mask {j}")
        np.testing.assert_array_equal(st["day"][~m], before["day"][~m], err_msg=f"mask {j}")
