"""CPU-side checks of the per-env episode windows of the batched cash-penalty and stop-loss envs: the
header declares finenv_cashpenalty_set_windows / finenv_stoploss_set_windows and the library exports
them, the setters validate their handle without a GPU, the ABI version, the struct sizes and the field
enums of both kinds are those of v3, and the Python classes expose the API through the shared
WindowedEnv code."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_header as H

KINDS = ("cashpenalty", "stoploss")


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def _config(kind):
    from finrl_amd import _native as nat
    base = (70, 5, 2, 40, 0, 1, 0, 0, 1000.0, 1e-3, 1e-3, 1e6, 0.1, 0.0)
    return nat.CashPenaltyConfig(*base) if kind == "cashpenalty" else nat.StopLossConfig(*base, 0.9, 1.2)


@pytest.mark.parametrize("kind", KINDS)
def test_header_declares_and_library_exports_set_windows(L, kind):
    hdr = H.source()
    assert H.prototypes()[f"finenv_{kind}_set_windows"] == ("int", [(f"finenv_{kind} *", "h"), ("int32_t *", "win")])
    assert hasattr(L, f"finenv_{kind}_set_windows")
    # the contract names the [4][E] pending / active layout
    env = "cash-penalty" if kind == "cashpenalty" else "stop-loss"
    body = re.sub(r"\s+", " ", hdr[hdr.index(f"Per-env episode windows of the {env} env"):
                                   hdr.index(f"finenv_{kind}_set_windows(finenv_{kind}")])
    for words in ("int32_t [4][E]", "PENDING", "ACTIVE", "Works before bind"):
        assert words in body, words
    for words in ("draw range", "offset", "clamp", "kernel argument", "FINENV_ERR_INVALID"):
        assert words in body.replace("OFFSET", "offset"), words


@pytest.mark.parametrize("kind", KINDS)
def test_set_windows_validates_the_handle(L, kind):
    fn = lambda name: getattr(L, f"finenv_{kind}_{name}")
    win = np.zeros((4, 70), dtype=np.int32)
    wp = win.ctypes.data_as(C.c_void_p)
    assert fn("set_windows")(None, None) == -1
    assert fn("set_windows")(None, wp) == -1
    h = C.c_void_p()
    cfg = _config(kind)
    assert fn("create")(C.byref(cfg), C.byref(h)) == 0
    try:
        # attaching and detaching work before bind (the block is only read by launches)
        assert fn("set_windows")(h, wp) == 0
        assert fn("set_windows")(h, None) == 0
        assert fn("set_windows")(h, wp) == 0
        # launches still need the bound state
        assert fn("reset")(h, None, None, None) == -2
        assert fn("step")(h, None, None, None, None, None, 1, None) == -2
    finally:
        fn("destroy")(h)


def test_abi_version_struct_sizes_and_enums_unchanged(L):
    from finrl_amd import _native as nat
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    assert H.constants()["FINENV_ABI_VERSION"] == 3
    cls = (nat.CashPenaltyConfig, nat.CashPenaltyPanelPtrs, nat.CashPenaltyStatePtrs,
           nat.StopLossConfig, nat.StopLossPanelPtrs, nat.StopLossStatePtrs)
    for which, c in zip(range(12, 18), cls):
        assert L.finenv_struct_size(which) == C.sizeof(c)
    assert tuple(C.sizeof(c) for c in cls) == (80, 24, 16, 96, 24, 16)
    assert H.enum("FINENV_CASHPENALTY_F64_FIELDS") == [
        "FINENV_KF_COH", "FINENV_KF_TURBULENCE", "FINENV_KF_SUM_TRADES", "FINENV_KF_LOGGED_TOTAL",
        "FINENV_KF_LOGGED_CASH", "FINENV_CASHPENALTY_F64_FIELDS"]
    assert H.enum("FINENV_CASHPENALTY_I32_FIELDS") == [
        "FINENV_KI_DATE_INDEX", "FINENV_KI_START", "FINENV_KI_EPISODE", "FINENV_KI_NEXT_START",
        "FINENV_CASHPENALTY_I32_FIELDS"]
    assert H.enum("FINENV_STOPLOSS_F64_FIELDS") == [
        "FINENV_LF_COH", "FINENV_LF_TURBULENCE", "FINENV_LF_SUM_TRADES", "FINENV_LF_LOGGED_TOTAL",
        "FINENV_LF_LOGGED_CASH", "FINENV_LF_ACTUAL_NUM_TRADES", "FINENV_STOPLOSS_F64_FIELDS"]
    assert H.enum("FINENV_STOPLOSS_I32_FIELDS") == [
        "FINENV_LI_DATE_INDEX", "FINENV_LI_START", "FINENV_LI_EPISODE", "FINENV_LI_NEXT_START",
        "FINENV_STOPLOSS_I32_FIELDS"]
    assert nat.CASHPENALTY_F64_FIELDS == ("coh", "turbulence", "sum_trades", "logged_total",
                                          "logged_cash")
    assert nat.STOPLOSS_F64_FIELDS == nat.CASHPENALTY_F64_FIELDS + ("actual_num_trades",)
    assert nat.CASHPENALTY_I32_FIELDS == nat.STOPLOSS_I32_FIELDS == \
        ("date_index", "start", "episode", "next_start")


def _classes():
    from finrl_amd.vec_cashpenalty import VecCashPenaltyEnv, VecStopLossEnv
    return VecCashPenaltyEnv, VecStopLossEnv


def test_envs_expose_the_window_api():
    import inspect
    from finrl_amd.vec_base import WindowedEnv
    for cls in _classes():
        assert "windows" in inspect.signature(cls.__init__).parameters
        for m in ("set_windows", "window_day"):
            assert callable(getattr(cls, m)), m
        assert list(inspect.signature(cls.set_windows).parameters) == ["self", "start", "end", "mask"]
        # one copy of the host-side window code: the base class's, reached through its hooks
        assert issubclass(cls, WindowedEnv)
        assert cls._check_windows is WindowedEnv._check_windows
        assert cls._attach_windows is WindowedEnv._attach_windows
        assert cls._window_max_step is WindowedEnv._window_max_step
        assert cls._new_window_block is WindowedEnv._new_window_block
        assert cls._window_min == 1 and cls._window_active


def test_host_validation_of_windows():
    """_check_windows (the base class's) with these envs' hooks: a one-row window is legal, inside
    [0, T]."""
    pytest.importorskip("torch")
    from types import SimpleNamespace
    for cls in _classes():
        env = object.__new__(cls)                              # no device: only the host-side hooks
        env.num_envs, env.panel = 5, SimpleNamespace(T=20)
        assert env._window_rows == 20
        s, t = env._check_windows(np.array([0, 3, 19, 0, 7]), np.array([2, 20, 20, 20, 8]))
        assert s.dtype == t.dtype == np.int64 and s.shape == t.shape == (5,)
        s, t = env._check_windows(4, 5)                        # one pair for all envs, one row
        assert s.tolist() == [4] * 5 and t.tolist() == [5] * 5
        with pytest.raises(ValueError):
            env._check_windows(6, 6)
        with pytest.raises(ValueError, match="panel"):
            env._check_windows(-1, 5)
        with pytest.raises(ValueError, match="panel"):
            env._check_windows(0, 21)
        with pytest.raises(ValueError):
            env._check_windows(np.arange(4), 10)               # neither one value nor [E]
        with pytest.raises(ValueError):
            env._check_windows(0.0, 10)                        # rows are integers


@pytest.mark.parametrize("kind", KINDS)
def test_shard_env_kwargs_slices_windows(kind):
    from finrl_amd.distributed import env_class, shard_env_kwargs, shard_range
    assert env_class(kind) is _classes()[KINDS.index(kind)]
    E = 11
    s, t = np.arange(E), np.arange(E) + 7
    for rank in range(3):
        lo, hi = shard_range(E, rank, 3)
        n, kw = shard_env_kwargs(E, rank, 3, windows=(s, t), hmax=500, random_start=False)
        assert n == hi - lo and kw["hmax"] == 500 and kw["random_start"] is False
        np.testing.assert_array_equal(kw["windows"][0], s[lo:hi])
        np.testing.assert_array_equal(kw["windows"][1], t[lo:hi])
    n, kw = shard_env_kwargs(E, 1, 3, windows=(2, t))         # one start for all envs passes through
    assert kw["windows"][0] == 2 and len(kw["windows"][1]) == n
    # the facades hand every keyword, windows included, to the batched class
    import inspect
    from finrl_amd.meta.env_stock_trading.env_stocktrading_cashpenalty import StockTradingEnvCashpenalty
    from finrl_amd.meta.env_stock_trading.env_stocktrading_stoploss import StockTradingEnvStopLoss
    for facade in (StockTradingEnvCashpenalty, StockTradingEnvStopLoss):
        assert inspect.signature(facade.make_vec).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
