"""CPU-side checks of the per-env episode windows of the batched stock env: the header declares
finenv_stock_set_windows and the library exports it, the setter validates its handle without a GPU,
the ABI version and struct sizes are those of v3, and finrl_amd.data.windows_from_dates maps date
pairs to the panel rows data_split selects."""
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
    assert H.prototypes()["finenv_stock_set_windows"] == ("int", [("finenv_stock *", "h"), ("int32_t *", "win")])
    assert hasattr(L, "finenv_stock_set_windows")


def test_abi_version_and_struct_sizes_unchanged(L):
    from finrl_amd import _native as nat
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    assert H.constants()["FINENV_ABI_VERSION"] == 3
    for which, cls in enumerate((nat.StockConfig, nat.StockPanelPtrs, nat.StockStatePtrs)):
        assert L.finenv_struct_size(which) == C.sizeof(cls)
    # the v3 layouts, as a foreign binding written against them declares them
    assert (C.sizeof(nat.StockConfig), C.sizeof(nat.StockPanelPtrs), C.sizeof(nat.StockStatePtrs)) == \
        (72, 24, 16)
    assert nat.STOCK_I32_FIELDS == ("day", "price_day", "trades", "episode", "start_day")


def test_set_windows_validates_the_handle(L):
    from finrl_amd import _native as nat
    win = np.zeros((2, 64), dtype=np.int32)
    assert L.finenv_stock_set_windows(None, None) == -1
    assert L.finenv_stock_set_windows(None, win.ctypes.data_as(C.c_void_p)) == -1
    h = C.c_void_p()
    cfg = nat.StockConfig(64, 30, 8, 100, 100, 0, 1, 1, 1, 0, 1e-3, 1e-3, 1e-4, 0.0)
    assert L.finenv_stock_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # attaching and detaching work before bind (the block is only read by launches)
        assert L.finenv_stock_set_windows(h, win.ctypes.data_as(C.c_void_p)) == 0
        assert L.finenv_stock_set_windows(h, None) == 0
        assert L.finenv_stock_set_windows(h, win.ctypes.data_as(C.c_void_p)) == 0
        # launches still need the bound state
        assert L.finenv_stock_init(h, 0, None) == -2
    finally:
        L.finenv_stock_destroy(h)


def test_env_exposes_the_window_api():
    import inspect
    from finrl_amd.vec_env import VecStockTradingEnv
    assert "windows" in inspect.signature(VecStockTradingEnv.__init__).parameters
    for m in ("set_windows", "window_day"):
        assert callable(getattr(VecStockTradingEnv, m)), m


def _frame(dates, tics=("AAA", "BBB", "CCC")):
    rng = np.random.default_rng(3)
    rows = [dict(date=d, tic=t, close=float(rng.uniform(10, 20))) for d in dates for t in tics]
    df = pd.DataFrame(rows).sample(frac=1.0, random_state=1)       # data_split sorts
    return df


@pytest.mark.parametrize("kind", ["str", "int"])
def test_windows_from_dates_matches_data_split(kind):
    from finrl_amd.data import data_split, windows_from_dates
    if kind == "str":
        dates = list(pd.bdate_range("2020-01-01", periods=40).strftime("%Y-%m-%d"))
        pairs = [("2020-01-01", "2020-01-15"), ("2020-01-06", "2020-01-07"), ("2020-01-10", "2020-03-01"),
                 ("2019-12-01", "2020-01-03"), ("2020-01-04", "2020-01-08"), (dates[5], dates[-1])]
    else:
        dates = list(range(20200101, 20200101 + 3 * 40, 3))           # gaps: ends between dates too
        pairs = [(20200101, 20200140), (20200102, 20200105), (20200150, 20300000), (0, 20200105),
                 (dates[7], dates[8]), (dates[0], dates[-1])]
    df = _frame(dates)
    full = data_split(df, dates[0], "9999" if kind == "str" else 10 ** 9)
    panel_dates = full.date.unique()                                   # panel row r <-> date r
    s, t = windows_from_dates(df.date, [p[0] for p in pairs], [p[1] for p in pairs])
    assert s.shape == t.shape == (len(pairs),)
    for (a, b), s_e, t_e in zip(pairs, s, t):
        sub = data_split(df, a, b)
        got = list(panel_dates[s_e:t_e])
        assert got == list(sub.date.unique()), (a, b)
        assert len(got) == len(sub.index.unique())                     # the env's T on that frame
    # one pair (scalars) works too
    s1, t1 = windows_from_dates(panel_dates, pairs[0][0], pairs[0][1])
    assert (int(s1[0]), int(t1[0])) == (int(s[0]), int(t[0]))


def test_windows_from_dates_rejects_an_empty_window():
    from finrl_amd.data import windows_from_dates
    dates = ["2020-01-02", "2020-01-03", "2020-01-06"]
    with pytest.raises(ValueError):
        windows_from_dates(dates, ["2020-01-02", "2020-01-04"], ["2020-01-06", "2020-01-05"])
    with pytest.raises(ValueError):
        windows_from_dates(dates, "2020-01-03", "2020-01-03")
    with pytest.raises(ValueError):
        windows_from_dates([1, 2, 3], 4, 9)
