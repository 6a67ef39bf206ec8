"""CPU-side checks of the last-episode block's C ABI: the header declares the setters, readouts and
FINENV_SL_* / FINENV_PL_* field enums, the library exports them, the Python field tuples follow the
header, and the entry points validate their arguments without a GPU."""
import ctypes as C
import numpy as np
import pytest

import abi_header as H


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def _enum(prefix, count_name):
    names = H.enum(count_name)[:-1]
    assert all(n.startswith(f"FINENV_{prefix}_") for n in names)
    return [n[len(f"FINENV_{prefix}_"):] for n in names]


def test_header_declares_and_library_exports_the_block_api(L):
    for fn in ("finenv_stock_set_last_episode", "finenv_stock_last_episode_stats",
               "finenv_portfolio_set_last_episode", "finenv_portfolio_last_episode_stats"):
        assert H.prototypes()[fn][0] == "int", fn
        assert hasattr(L, fn), fn
    assert "FINENV_STOCK_LAST_FIELDS" in H.constants() and "FINENV_PORTFOLIO_LAST_FIELDS" in H.constants()


def test_field_tuples_match_the_header():
    from finrl_amd import _native as nat
    assert tuple(x.lower() for x in _enum("SL", "FINENV_STOCK_LAST_FIELDS")) == nat.STOCK_LAST_FIELDS
    assert tuple(x.lower() for x in _enum("PL", "FINENV_PORTFOLIO_LAST_FIELDS")) == nat.PORTFOLIO_LAST_FIELDS
    assert nat.STOCK_LAST_FIELDS[0] == nat.PORTFOLIO_LAST_FIELDS[0] == "count"


def test_abi_version_and_struct_sizes_unchanged(L):
    from finrl_amd import _native as nat
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    for which, cls in enumerate((nat.StockConfig, nat.StockPanelPtrs, nat.StockStatePtrs,
                                 nat.PortfolioConfig, nat.PortfolioPanelPtrs,
                                 nat.PortfolioStatePtrs)):
        assert L.finenv_struct_size(which) == C.sizeof(cls)


def test_stock_entry_points_validate_arguments(L):
    from finrl_amd import _native as nat
    out = np.zeros((64, 6))
    blk = np.zeros((len(nat.STOCK_LAST_FIELDS), 64))
    assert L.finenv_stock_set_last_episode(None, None) == -1
    assert L.finenv_stock_last_episode_stats(None, out.ctypes.data_as(C.c_void_p), None) == -1
    h = C.c_void_p()
    cfg = nat.StockConfig(64, 30, 8, 100, 100, 0, 1, 1, 1, 0, 1e-3, 1e-3, 1e-4, 0.0)
    assert L.finenv_stock_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # no block attached (the default): the readout refuses, with a message
        assert L.finenv_stock_last_episode_stats(h, out.ctypes.data_as(C.c_void_p), None) == -1
        assert b"last-episode block" in L.finenv_stock_last_error(h)
        assert L.finenv_stock_last_episode_stats(h, None, None) == -1
        # attaching works before bind; the readout then needs the bound state
        assert L.finenv_stock_set_last_episode(h, blk.ctypes.data_as(C.c_void_p)) == 0
        assert L.finenv_stock_last_episode_stats(h, out.ctypes.data_as(C.c_void_p), None) == -2
        # NULL detaches again
        assert L.finenv_stock_set_last_episode(h, None) == 0
        assert L.finenv_stock_last_episode_stats(h, out.ctypes.data_as(C.c_void_p), None) == -1
    finally:
        L.finenv_stock_destroy(h)


def test_portfolio_entry_points_validate_arguments(L):
    from finrl_amd import _native as nat
    out = np.zeros((64, 3))
    blk = np.zeros((len(nat.PORTFOLIO_LAST_FIELDS), 64))
    assert L.finenv_portfolio_set_last_episode(None, None) == -1
    assert L.finenv_portfolio_last_episode_stats(None, out.ctypes.data_as(C.c_void_p), None) == -1
    h = C.c_void_p()
    cfg = nat.PortfolioConfig(64, 30, 8, 100, 1e6)
    assert L.finenv_portfolio_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.finenv_portfolio_last_episode_stats(h, out.ctypes.data_as(C.c_void_p), None) == -1
        assert b"last-episode block" in L.finenv_portfolio_last_error(h)
        assert L.finenv_portfolio_set_last_episode(h, blk.ctypes.data_as(C.c_void_p)) == 0
        assert L.finenv_portfolio_last_episode_stats(h, out.ctypes.data_as(C.c_void_p), None) == -2
        assert L.finenv_portfolio_set_last_episode(h, None) == 0
        assert L.finenv_portfolio_last_episode_stats(h, out.ctypes.data_as(C.c_void_p), None) == -1
    finally:
        L.finenv_portfolio_destroy(h)


def test_envs_expose_the_block_methods():
    from finrl_amd.vec_env import VecStockTradingEnv
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    for cls, n in ((VecStockTradingEnv, 6), (VecStockPortfolioEnv, 3)):
        for m in ("enable_last_episode", "last_episode_stats", "last_episode_return"):
            assert callable(getattr(cls, m)), (cls, m)
        assert len(cls.last_episode_keys) == n and cls.last_episode_keys[-1] == "sharpe"
