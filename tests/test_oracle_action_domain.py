"""The oracle on the action domain tests/test_gpu_stock_action_domain.py holds the kernels to:
oracle.stock.StockOracle (int64 scaled actions, no clamp, fmod-based `//`) must equal
oracle/pandas_env.py -- NumPy's own `(actions * hmax).astype(int)`, stable argsort and Python's `//`,
itself pinned by the reference-recorded fixtures, `stock_bigactions` among them
(tests/test_oracle_golden.py) -- on the same action sets: (a) truncation boundaries, (b) scaled
magnitudes from 255 to 2^25 with ties and per-env books, (d) cash-bound buys at quotients of 10^6 and
more where `//` differs from floor(c / unit).  Exact, float64, N in {5, 100}.  CPU only."""
import numpy as np
import pytest

import action_domain_cases as adc

T, K, E = 6, 2, 4


def _panel(N, T_=T):
    rng = np.random.default_rng(31 + N)
    close = (50 + rng.uniform(0, 10, (T_, N))).astype(np.float32).astype(np.float64)
    tech = rng.normal(0, 1, (T_, K, N)).astype(np.float32).astype(np.float64)
    tech[tech == 1.0] = 0.5                   # (1.0 in the first indicator is the fork's untradable flag)
    return close, tech, np.abs(rng.normal(0, 30, T_))


def _compare(close, tech, risk, hmax, cash0, shares0, actions):
    """actions [S, E, N]: every env of one StockOracle batch against its own PandasStockEnv, reset
    before the first step and after every done, as SB3's DummyVecEnv drives the reference."""
    from oracle.pandas_env import PandasStockEnv, make_frame
    from oracle.stock import StockOracle
    S, E_, N = actions.shape
    df = make_frame(close, tech, risk)
    orc = StockOracle(close, tech, risk, n_envs=E_, hmax=hmax, initial_amount=cash0,
                      num_stock_shares=shares0)
    envs = [PandasStockEnv(df, hmax=hmax, initial_amount=float(cash0[e]),
                           num_stock_shares=[int(x) for x in shares0[e]]) for e in range(E_)]
    obs = orc.reset()
    for e, env in enumerate(envs):
        np.testing.assert_array_equal(np.asarray(env.reset(), np.float64), obs[e])
    n_done = 0
    for s in range(S):
        obs, rew, done = orc.step(actions[s])
        st = orc.state()
        for e, env in enumerate(envs):
            p_obs, p_rew, p_done, _ = env.step(actions[s, e])
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
    return n_done, orc


@pytest.mark.parametrize("hmax", [100, 255, 256])
@pytest.mark.parametrize("N", [5, 100])
def test_truncation_boundaries(N, hmax):
    """(a): every value of boundary_values(hmax) (k / hmax and both float32 neighbours, +-0.0, +-1.0,
    smallest normal, denormal, |a * hmax| < 1), dealt over the rows of four envs."""
    vals = adc.boundary_values(hmax)
    rng = np.random.default_rng(hmax + N)
    steps = -(-len(vals) // (E * N))
    steps += -steps % T + 1                   # whole episodes and one step more
    act = np.resize(vals[rng.permutation(len(vals))], steps * E * N).reshape(steps, E, N)
    assert np.isin(vals.view(np.uint32), act.view(np.uint32)).all()
    cash0 = np.full(E, 1e6)
    shares0 = np.broadcast_to(rng.integers(0, 40, N), (E, N))
    n_done, _ = _compare(*_panel(N), hmax, cash0, shares0, act)
    assert n_done >= 1


@pytest.mark.parametrize("N", [5, 100])
def test_beyond_unit_interval(N):
    """(b): scaled magnitudes 255 .. amax of the kernel that steps N tickers, both signs, with ties;
    one env of each kind of env_books(), so the action, the holdings and the cash each bind."""
    hmax, amax = 128, 1 << 25 if N <= 32 else 1 << 23
    steps = 2 * T + 2 if N > 32 else 8 * T    # (N = 5: more rows, so that every magnitude occurs)
    act, signed = adc.big_tiles(adc.magnitudes_inside(amax), hmax, E, N, steps, seed=N)
    cash0, shares0 = adc.env_books(E, N, seed=N)
    assert np.isin(signed, adc.scaled(act, hmax)).all()
    n_done, _ = _compare(*_panel(N), hmax, cash0, shares0, act)
    assert n_done >= 2


@pytest.mark.parametrize("N", [5, 100])
def test_floor_division_at_large_quotients(N):
    """(d): one cash-bound buy per env at cash // unit in [10^6, amax), every env a case where `//`
    differs from floor(cash / unit) or floor(cash * (1 / unit)) (floordiv_cases asserts it)."""
    hmax, amax, E_ = 128, 1 << 25 if N <= 32 else 1 << 23, 16
    close, tech, risk = _panel(N, 3)
    tick, cash, q = adc.floordiv_cases(close[0], 1e-3, E_, 10 ** 6, amax, True, seed=N)
    act = np.zeros((1, E_, N), np.float32)
    act[0, np.arange(E_), tick] = amax / hmax
    _, orc = _compare(close, tech, risk, hmax, cash, np.zeros((E_, N), np.int64), act)
    np.testing.assert_array_equal(orc.state()["shares"][np.arange(E_), tick], q)
