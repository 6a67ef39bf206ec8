"""CPU-side checks of the per-env episode windows of the batched portfolio env: the header declares
finenv_portfolio_set_windows and the library exports it, the setter validates its handle without a
GPU, the ABI version, the portfolio struct sizes and field enums are those of v3, and
finrl_amd.data.windows_from_dates over a PortfolioPanel's dates selects the rows data_split selects."""
import ctypes as C
import numpy as np
import pandas as pd
import pytest

import abi_header as H


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def test_header_declares_and_library_exports_set_windows(L):
    assert H.prototypes()["finenv_portfolio_set_windows"] == \
        ("int", [("finenv_portfolio *", "h"), ("int32_t *", "win")])
    assert hasattr(L, "finenv_portfolio_set_windows")


def test_set_windows_validates_the_handle(L):
    from finrl_amd import _native as nat
    win = np.zeros((2, 70), dtype=np.int32)
    assert L.finenv_portfolio_set_windows(None, None) == -1
    assert L.finenv_portfolio_set_windows(None, win.ctypes.data_as(C.c_void_p)) == -1
    h = C.c_void_p()
    cfg = nat.PortfolioConfig(70, 30, 8, 100, 1e6)
    assert L.finenv_portfolio_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # attaching and detaching work before bind (the block is only read by launches)
        assert L.finenv_portfolio_set_windows(h, win.ctypes.data_as(C.c_void_p)) == 0
        assert L.finenv_portfolio_set_windows(h, None) == 0
        assert L.finenv_portfolio_set_windows(h, win.ctypes.data_as(C.c_void_p)) == 0
        # launches still need the bound state
        assert L.finenv_portfolio_reset(h, None, None, None) == -2
    finally:
        L.finenv_portfolio_destroy(h)


def test_abi_version_struct_sizes_and_enums_unchanged(L):
    from finrl_amd import _native as nat
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    assert H.constants()["FINENV_ABI_VERSION"] == 3
    cls = (nat.PortfolioConfig, nat.PortfolioPanelPtrs, nat.PortfolioStatePtrs)
    for which, c in zip((3, 4, 5), cls):
        assert L.finenv_struct_size(which) == C.sizeof(c)
    assert tuple(C.sizeof(c) for c in cls) == (24, 16, 16)
    assert H.enum("FINENV_PORTFOLIO_F64_FIELDS") == [
        "FINENV_PF_VALUE", "FINENV_PF_LAST_REWARD", "FINENV_PORTFOLIO_F64_FIELDS"]
    assert H.enum("FINENV_PORTFOLIO_I32_FIELDS") == ["FINENV_PI_DAY", "FINENV_PORTFOLIO_I32_FIELDS"]
    pl = H.enum("FINENV_PORTFOLIO_LAST_FIELDS")[:-1]
    assert all(n.startswith("FINENV_PL_") for n in pl)
    names = [n[len("FINENV_PL_"):] for n in pl]
    assert names == ["COUNT", "BEGIN_VALUE", "END_VALUE", "RET_N", "RET_SUM", "RET_SUMSQ", "RUN_SUM",
                     "RUN_SUMSQ"]
    assert nat.PORTFOLIO_F64_FIELDS == ("value", "last_reward")
    assert nat.PORTFOLIO_I32_FIELDS == ("day",)
    assert [n.lower() for n in names] == list(nat.PORTFOLIO_LAST_FIELDS)


def test_env_exposes_the_window_api():
    import inspect
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    assert "windows" in inspect.signature(VecStockPortfolioEnv.__init__).parameters
    for m in ("set_windows", "window_day"):
        assert callable(getattr(VecStockPortfolioEnv, m)), m


def _cov_frame(dates, tics=("AAA", "BBB", "CCC")):
    """A frame shaped like the portfolio tutorial's: one row per (date, tic) and a per-day cov_list,
    computed over the whole frame before any split."""
    rng = np.random.default_rng(5)
    N = len(tics)
    rows = []
    for d in dates:
        cov = rng.normal(0, 1e-4, (N, N))
        for t in tics:
            rows.append(dict(date=d, tic=t, close=float(rng.uniform(10, 20)), macd=float(rng.normal()),
                             cov_list=cov))
    return pd.DataFrame(rows).sample(frac=1.0, random_state=2)


def test_windows_from_dates_over_portfolio_panel_matches_data_split():
    from finrl_amd.data import data_split, windows_from_dates
    from finrl_amd.panel import PortfolioPanel
    dates = list(pd.bdate_range("2020-06-01", periods=45).strftime("%Y-%m-%d"))
    df = _cov_frame(dates)
    panel = PortfolioPanel.from_dataframe(data_split(df, dates[0], "9999"), ["macd"])
    assert panel.dates == dates
    pairs = [(dates[0], "2020-06-30"), ("2020-07-01", "2020-08-01"), ("2020-06-03", "2020-06-04"),
             ("2020-05-01", "2020-06-05"), (dates[10], dates[-1])]
    s, t = windows_from_dates(panel.dates, [p[0] for p in pairs], [p[1] for p in pairs])
    for (a, b), s_e, t_e in zip(pairs, s, t):
        sub = data_split(df, a, b)
        sp = PortfolioPanel.from_dataframe(sub, ["macd"])
        assert sp.dates == panel.dates[s_e:t_e], (a, b)
        assert sp.T == len(sub.index.unique())                    # the reference env's day count
        np.testing.assert_array_equal(sp.close, panel.close[s_e:t_e])
        np.testing.assert_array_equal(sp.cov, panel.cov[s_e:t_e])
        np.testing.assert_array_equal(sp.obs_template(), panel.obs_template()[s_e:t_e])
        # the slice's returns are the panel's rows inside the window (its last row is never read)
        np.testing.assert_array_equal(sp.gross_returns()[:-1], panel.gross_returns()[s_e:t_e - 1])
