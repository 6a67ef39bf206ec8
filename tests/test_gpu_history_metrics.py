"""The one metrics kernel behind finenv_<kind>_history_metrics (finrl_amd/csrc/finenv_history.hip), for
every env kind, against pandas on records written straight into the history's tensors: the value column
alone (stock, crypto, array-state stock), value plus a second column with the armed flag required
(cash-penalty, stop-loss), and the recorded return column read from entry 0 (portfolio).  300 envs: two
blocks of the kernel, the second partial.  No env is stepped."""
import numpy as np
import pytest
import torch

from twowave_windows_cases import COMMON, classes, make_panel

pytestmark = pytest.mark.gpu

E, CAP, T = 300, 8, 8
KINDS = ("stock", "portfolio", "crypto", "stocknp", "cashpenalty", "stoploss")
TWOWAVE = ("cashpenalty", "stoploss")
# the absolute tolerances of the kinds' own test_metrics_against_pandas (rtol is 1e-9 everywhere):
# (cumulative_return and max_drawdown, mean and std, sharpe)
ATOL = {k: (1e-15, 1e-18, 0.0) if k in TWOWAVE else (1e-12, 1e-12, 1e-12) for k in KINDS}
UNARMED = 5                                                  # the env whose flags are 0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _env(kind):
    """The smallest env of the kind over a random panel of T rows."""
    rng = np.random.default_rng(2)
    price = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, 2)), axis=0))
    if kind == "stock":
        from finrl_amd import StockPanel
        from finrl_amd.vec_env import VecStockTradingEnv
        return VecStockTradingEnv(StockPanel(price, rng.normal(0, 1, (T, 1, 2)), np.zeros(T)), E)
    if kind == "portfolio":
        from finrl_amd.panel import PortfolioPanel
        from finrl_amd.vec_portfolio import VecStockPortfolioEnv
        return VecStockPortfolioEnv(PortfolioPanel(price, rng.normal(0, 1e-4, (T, 2, 2)),
                                                   rng.normal(0, 1, (T, 1, 2))), E)
    if kind == "crypto":
        from finrl_amd.vec_crypto import VecCryptoEnv
        return VecCryptoEnv({"price_array": price, "tech_array": rng.normal(0, 1, (T, 1))}, E, lookback=1)
    if kind == "stocknp":
        from finrl_amd.vec_stocknp import VecStockTradingEnvNP
        return VecStockTradingEnvNP({"price_array": price, "tech_array": rng.normal(0, 1, (T, 2)),
                                     "turbulence_array": np.zeros(T), "if_train": False}, E)
    Panel, Env, _ = classes(kind)
    return Env(Panel(*make_panel(2, 1, T)), E, random_start=False, hmax=100.0, turbulence_threshold=None,
               patient=False, discrete_actions=False, **COMMON)


@pytest.fixture(scope="module")
def record():
    """values [CAP, E], the returns recorded with them, lengths [E] over 0 .. 11 -- drawn once, shared by
    the kinds and never changed."""
    rng = np.random.default_rng(77)
    values = 1e6 * np.cumprod(1 + rng.normal(0, 0.02, (CAP, E)), axis=0)
    values[:, ::17] = values[0, ::17]                        # constant series: std 0, no Sharpe ratio
    ret = np.zeros((CAP, E))
    ret[1:] = values[1:] / values[:-1] - 1
    length = rng.integers(0, 12, E).astype(np.int32)
    length[17:25] = (0, 1, 2, 3, 7, 8, 9, 11)                # every boundary, past the capacity included
    length[[0, 34]] = (6, 1)                                 # constant envs: several entries, and one
    length[UNARMED] = 5
    for a in (values, ret, length):
        a.setflags(write=False)
    return values, ret, length


def _pandas_metrics(v, r, ann):
    """v: the values, r: their returns as a pandas Series (NaNs dropped) -> the six columns."""
    mean = r.mean() if len(r) >= 1 else np.nan
    std = r.std() if len(r) >= 2 else np.nan
    sharpe = ann * mean / std if len(r) >= 2 and std != 0 else np.nan
    return [len(r), v.iloc[-1] / v.iloc[0] - 1, mean, std, sharpe, (v / v.cummax() - 1).min()]


@pytest.mark.parametrize("kind", KINDS)
def test_metrics_against_pandas(kind, record):
    _need_gpu()
    import pandas as pd
    from finrl_amd import _native as nat
    values, ret, length = record
    env = _env(kind)
    env.reset()
    kw = {"stock": dict(actions=False), "portfolio": dict(weights=False), "crypto": dict(stocks=False),
          "stocknp": dict(stocks=False, tags=False)}.get(kind, dict(transactions=False, actions=False))
    hist = env.enable_history(capacity=CAP, **kw)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()     # noqa: E731 (a writable copy)
    if kind in TWOWAVE:                                      # the account value is cash + asset_value
        cash = np.round(values * 0.3, 2)
        hist.cash.copy_(dev(cash))
        hist.asset_value.copy_(dev(values - cash))
        total = cash + (values - cash)
        flags = np.full(E, nat.HIST_ARMED, np.int32)
    else:
        getattr(hist, "value" if kind == "portfolio" else "asset").copy_(dev(values))
        total = values
        flags = np.full(E, nat.HIST_COMPLETE, np.int32)      # (these kinds' metrics read no flag)
    if kind == "portfolio":
        hist.ret.copy_(dev(ret))
    flags[UNARMED] = 0
    hist.length.copy_(dev(length))
    hist.flags.copy_(dev(flags))
    k0 = 0 if kind == "portfolio" else 1                     # the first entry that carries a return
    a_v, a_m, a_s = ATOL[kind]
    for ann in (252 ** 0.5, 4 ** 0.5):
        m = hist.metrics(ann).cpu().numpy()
        assert m.shape == (E, 6)
        seen = set()
        for e in range(E):
            n = min(int(length[e]), CAP)
            if n == 0 or (kind in TWOWAVE and e == UNARMED):
                assert np.isnan(m[e]).all(), e
                continue
            v = pd.Series(total[:n, e])
            r = pd.Series(ret[:n, e]) if kind == "portfolio" else v.pct_change(1).dropna()
            want = _pandas_metrics(v, r, ann)
            assert m[e, 0] == want[0] == n - k0, e
            np.testing.assert_allclose(m[e, [1, 5]], [want[1], want[5]], rtol=1e-9, atol=a_v,
                                       err_msg=f"env {e}")
            if want[0] == 0:                                 # a single entry without a return
                assert np.isnan(m[e, 2:5]).all(), e
                seen.add("no return")
                continue
            np.testing.assert_allclose(m[e, 2], want[2], rtol=1e-9, atol=a_m, err_msg=f"mean {e}")
            if want[0] < 2:
                assert np.isnan(m[e, 3]) and np.isnan(m[e, 4]), e
                seen.add("one return")
            elif e % 17 == 0:
                assert m[e, 3] == 0 and np.isnan(m[e, 4]), e
                seen.add("constant")
            else:
                np.testing.assert_allclose(m[e, 3], want[3], rtol=1e-9, atol=a_m, err_msg=f"std {e}")
                np.testing.assert_allclose(m[e, 4], want[4], rtol=1e-9, atol=a_s, err_msg=f"sharpe {e}")
                seen.add("sharpe")
        assert seen == {"one return", "constant", "sharpe"} | ({"no return"} if k0 else set())
    env._call("set_history", None)                           # detach before the tensors go away
