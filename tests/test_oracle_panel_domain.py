"""The stock oracle on the panel domain the tests/test_gpu_*_panel_domain.py files hold the kernels
to: oracle.stock.StockOracle must equal oracle/pandas_env.py -- Python floats, NumPy's stable argsort
and Python's `//`, itself pinned by the reference-recorded fixtures, `stock_pricedomain` among them
(tests/test_oracle_golden.py) -- on every builder of panel_domain_cases: zero closes with and
without the untradable flag, price levels 1e-4 .. 3e5 against cash 1e2 .. 1e9, tech_0 at the
neighbours of 1.0, risk rows at the threshold, its neighbours and +-0.0.  Exact, float64, N in
{5, 100}, turbulence off and on.  CPU only.

One documented deviation: on an unflagged zero close the
reference-shaped env divides by zero in a buy, where the oracle and the kernels fill 0 shares and
count no trade.  The comparison therefore turns such buy requests into sells of the same size and
test_reference_shaped_env_divides_by_zero asserts that the division does raise."""
import numpy as np
import pytest

import panel_domain_cases as pdc

T, E = 8, 16


def _compare(case, hmax, use_turbulence, acts):
    """acts [S, E, N]: every env of one StockOracle batch against its own PandasStockEnv, reset before
    the first step and after every done.  -> the event counts of the oracle trace."""
    from oracle.pandas_env import PandasStockEnv, make_frame
    from oracle.stock import StockOracle
    S, E_, N = acts.shape
    acts = acts.copy()
    thr = case.threshold if use_turbulence else None
    df = make_frame(case.close, case.tech, case.risk)
    orc = StockOracle(case.close, case.tech, case.risk, n_envs=E_, hmax=hmax, initial_amount=case.cash0,
                      num_stock_shares=case.shares0, turbulence_threshold=thr)
    envs = [PandasStockEnv(df, hmax=hmax, initial_amount=float(case.cash0[e]),
                           num_stock_shares=[int(x) for x in case.shares0[e]],
                           turbulence_threshold=thr) for e in range(E_)]
    obs = orc.reset()
    for e, env in enumerate(envs):
        np.testing.assert_array_equal(np.asarray(env.reset(), np.float64), obs[e])
    keys = ("cash", "shares", "cost", "trades", "day", "price_day", "turbulence")
    pre, post, real, n_done = [], [], [], 0
    for s in range(S):
        st = {k: v.copy() for k, v in orc.state().items() if k in keys}
        row = st["price_day"]
        undefined = (case.close[row] == 0.0) & (case.tech[row, 0, :] != 1.0) & (acts[s] > 0)
        acts[s] = np.where(undefined, -acts[s], acts[s])
        pre.append(st)
        obs, rew, done, r = orc.step(acts[s], want_realised=True)
        real.append(r)
        st = orc.state()
        post.append({k: v.copy() for k, v in st.items() if k in keys})
        for e, env in enumerate(envs):
            p_obs, p_rew, p_done, _ = env.step(acts[s, e])
            msg = f"step {s} env {e}"
            assert p_done == done[e] and p_rew == rew[e], msg
            assert env.cash == st["cash"][e] and env.cost == st["cost"][e], msg
            assert env.trades == st["trades"][e], msg
            np.testing.assert_array_equal(np.asarray(env.shares, np.float64), st["shares"][e], err_msg=msg)
            np.testing.assert_array_equal(np.asarray(p_obs, np.float64), obs[e], err_msg=msg)
        if done.all():
            n_done += 1
            obs = orc.reset()
            for e, env in enumerate(envs):
                np.testing.assert_array_equal(np.asarray(env.reset(), np.float64), obs[e])
    assert n_done >= 2
    return pdc.stock_events(case, hmax, use_turbulence, acts, pre, real, post)


@pytest.mark.parametrize("use_turbulence", [False, True])
@pytest.mark.parametrize("N", [5, 100])
@pytest.mark.parametrize("name", list(pdc.STOCK_CASES))
def test_oracle_matches_reference_shaped_env(name, N, use_turbulence):
    case = pdc.STOCK_CASES[name](N, T, E, seed=13 * N + 1)
    acts = pdc.actions(E, N, 2 * T + 2, seed=N)
    ev = _compare(case, 100, use_turbulence, acts)
    if name == "zero_closes":                   # (buys at unflagged zeros were turned into sells)
        assert ev["buy_at_zero"] == 0
        ev["buy_at_zero"] = 1
    pdc.require_stock_events(name, ev, use_turbulence)


def test_reference_shaped_env_divides_by_zero():
    """A buy at an unflagged zero close: ZeroDivisionError in the reference-shaped env (its `//`), 0
    shares and no trade in the oracle.  The same request on a flagged zero close is skipped by both."""
    from oracle.pandas_env import PandasStockEnv, make_frame
    from oracle.stock import StockOracle
    close = np.array([[10.0, 0.0, 0.0], [11.0, 0.0, 0.0], [12.0, 1.0, 1.0]])
    tech = np.zeros((3, 1, 3))
    tech[:, 0, 2] = 1.0                                       # ticker 2: zero close, flagged
    risk = np.zeros(3)
    env = PandasStockEnv(make_frame(close, tech, risk), hmax=10, initial_amount=1000.0)
    env.reset()
    env.step(np.array([0.5, 0.0, 0.5], np.float32))           # flagged zero: no division
    assert env.shares == [5, 0, 0] and env.trades == 1
    with pytest.raises(ZeroDivisionError):
        env.step(np.array([0.0, 0.5, 0.0], np.float32))
    orc = StockOracle(close, tech, risk, hmax=10, initial_amount=1000.0)
    orc.reset()
    orc.step(np.array([[0.5, 0.0, 0.5]], np.float32))
    _, _, _, real = orc.step(np.array([[0.0, 0.5, 0.0]], np.float32), want_realised=True)
    st = orc.state()
    assert (real == 0).all() and st["trades"][0] == 1 and st["shares"][0].tolist() == [5, 0, 0]


def test_signed_close_carries_the_flag_in_the_sign_bit():
    """StockPanel.signed_close(): a negative close is rejected, an unflagged -0.0 becomes +0.0, a
    flagged zero is -0.0, and the flag is the fp64 compare tech_0 == 1.0 -- none of its neighbours."""
    from finrl_amd import StockPanel
    close = np.array([[5.0, -0.0, 0.0, 0.0, 7.0, 7.0, 7.0, 7.0, 7.0]])
    tech = np.zeros((1, 2, 9))
    tech[0, 0, 3] = 1.0
    tech[0, 0, 4:] = pdc.FLAG_VALUES
    tech[0, 1, :] = 1.0                                       # (only the first indicator is the flag)
    out = StockPanel(close, tech, np.zeros(1)).signed_close()
    np.testing.assert_array_equal(np.abs(out), np.abs(close))
    np.testing.assert_array_equal(np.signbit(out)[0],
                                  [False, False, False, True, True, False, False, False, False])
    with pytest.raises(ValueError):
        StockPanel(np.array([[5.0, -1e-300]]), np.zeros((1, 1, 2)), np.zeros(1)).signed_close()
    # without indicators there is no flag at all
    assert not np.signbit(StockPanel(close, None, None).signed_close()).any()
