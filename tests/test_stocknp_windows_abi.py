"""CPU-side checks of the per-env episode windows of the batched array-state stock env: the header
declares finenv_stocknp_set_windows and the library exports it, the setter validates its handle
without a GPU, the ABI version, the stocknp struct sizes and field enums are those of v3, and the
Python class exposes the API through the shared WindowedEnv code."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_header as H


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def test_header_declares_and_library_exports_set_windows(L):
    hdr = H.source()
    assert H.prototypes()["finenv_stocknp_set_windows"] == ("int", [("finenv_stocknp *", "h"), ("int32_t *", "win")])
    assert hasattr(L, "finenv_stocknp_set_windows")
    # the contract names the [4][E] pending / active layout
    body = re.sub(r"\s+", " ", hdr[hdr.index("Per-env episode windows of the array-state env"):
                                   hdr.index("int finenv_stocknp_set_windows")])
    for words in ("int32_t [4][E]", "PENDING", "ACTIVE", "Works before bind"):
        assert words in body, words


def test_set_windows_validates_the_handle(L):
    from finrl_amd import _native as nat
    win = np.zeros((4, 70), dtype=np.int32)
    wp = win.ctypes.data_as(C.c_void_p)
    assert L.finenv_stocknp_set_windows(None, None) == -1
    assert L.finenv_stocknp_set_windows(None, wp) == -1
    h = C.c_void_p()
    cfg = nat.StockNpConfig(70, 5, 10, 40, 10, 0, 100.0, 1e-3, 1e-3, 2 ** -11, 0.99, 0.0)
    assert L.finenv_stocknp_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # attaching and detaching work before bind (the block is only read by launches)
        assert L.finenv_stocknp_set_windows(h, wp) == 0
        assert L.finenv_stocknp_set_windows(h, None) == 0
        assert L.finenv_stocknp_set_windows(h, wp) == 0
        # launches still need the bound state
        assert L.finenv_stocknp_reset(h, None, None, None) == -2
        assert L.finenv_stocknp_step(h, None, None, None, None, None, 1, None) == -2
    finally:
        L.finenv_stocknp_destroy(h)


def test_abi_version_struct_sizes_and_enums_unchanged(L):
    from finrl_amd import _native as nat
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    assert H.constants()["FINENV_ABI_VERSION"] == 3
    cls = (nat.StockNpConfig, nat.StockNpPanelPtrs, nat.StockNpStatePtrs)
    for which, c in zip((9, 10, 11), cls):
        assert L.finenv_struct_size(which) == C.sizeof(c)
    assert tuple(C.sizeof(c) for c in cls) == (72, 24, 24)
    assert H.enum("FINENV_STOCKNP_F64_FIELDS") == [
        "FINENV_NF_AMOUNT", "FINENV_NF_TOTAL_ASSET", "FINENV_NF_GAMMA_REWARD", "FINENV_NF_INITIAL_TOTAL_ASSET",
        "FINENV_NF_EPISODE_RETURN", "FINENV_NF_LAST_REWARD", "FINENV_NF_AMOUNT0", "FINENV_STOCKNP_F64_FIELDS"]
    assert H.enum("FINENV_STOCKNP_I32_FIELDS") == [
        "FINENV_NI_DAY", "FINENV_NI_TAGS", "FINENV_NI_AMOUNT0_TAG", "FINENV_STOCKNP_I32_FIELDS"]
    assert nat.STOCKNP_F64_FIELDS == ("amount", "total_asset", "gamma_reward",
                                      "initial_total_asset", "episode_return", "last_reward",
                                      "amount0")
    assert nat.STOCKNP_I32_FIELDS == ("day", "tags", "amount0_tag")


def test_env_exposes_the_window_api():
    import inspect
    from finrl_amd.vec_base import WindowedEnv
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    assert "windows" in inspect.signature(VecStockTradingEnvNP.__init__).parameters
    for m in ("set_windows", "window_day", "draw_train_start"):
        assert callable(getattr(VecStockTradingEnvNP, m)), m
    assert list(inspect.signature(VecStockTradingEnvNP.set_windows).parameters) == \
        ["self", "start", "end", "mask"]
    assert list(inspect.signature(VecStockTradingEnvNP.draw_train_start).parameters) == ["self", "mask"]
    # one copy of the host-side window code: the base class's, reached through its hooks
    assert issubclass(VecStockTradingEnvNP, WindowedEnv)
    assert VecStockTradingEnvNP._check_windows is WindowedEnv._check_windows
    assert VecStockTradingEnvNP._attach_windows is WindowedEnv._attach_windows
    assert VecStockTradingEnvNP._window_max_step is WindowedEnv._window_max_step
    assert VecStockTradingEnvNP._new_window_block is WindowedEnv._new_window_block
    assert VecStockTradingEnvNP._window_min == 2 and VecStockTradingEnvNP._window_active


def test_host_validation_of_windows():
    """_check_windows (the base class's) with this env's hooks: a window needs two panel rows
    inside [0, T]."""
    pytest.importorskip("torch")
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    env = object.__new__(VecStockTradingEnvNP)            # no device: only the host-side hooks
    env.num_envs, env.price_ary = 5, np.zeros((20, 3), np.float32)
    assert env._window_rows == 20
    s, t = env._check_windows(np.array([0, 3, 18, 0, 7]), np.array([2, 20, 20, 20, 9]))
    assert s.dtype == t.dtype == np.int64 and s.shape == t.shape == (5,)
    s, t = env._check_windows(4, 6)                        # one pair for all envs
    assert s.tolist() == [4] * 5 and t.tolist() == [6] * 5
    with pytest.raises(ValueError, match="at least 2"):
        env._check_windows(5, 6)                           # one row: no step to take
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


def test_shard_env_kwargs_slices_windows():
    from finrl_amd.distributed import env_class, shard_env_kwargs, shard_range
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    assert env_class("stocknp") is VecStockTradingEnvNP
    E = 11
    s, t = np.arange(E), np.arange(E) + 7
    for rank in range(3):
        lo, hi = shard_range(E, rank, 3)
        n, kw = shard_env_kwargs(E, rank, 3, windows=(s, t), gamma=0.9, initial_capital=1e6)
        assert n == hi - lo and kw["gamma"] == 0.9 and kw["initial_capital"] == 1e6
        np.testing.assert_array_equal(kw["windows"][0], s[lo:hi])
        np.testing.assert_array_equal(kw["windows"][1], t[lo:hi])
    n, kw = shard_env_kwargs(E, 1, 3, windows=(2, t))         # one start for all envs passes through
    assert kw["windows"][0] == 2 and len(kw["windows"][1]) == n
    # the array-state facades hand every keyword, windows included, to the batched class
    import inspect
    from finrl_amd.meta.env_stock_trading.env_nas100_wrds import StockEnvNAS100
    from finrl_amd.meta.env_stock_trading.env_stocktrading_np import StockTradingEnv
    for facade in (StockTradingEnv, StockEnvNAS100):
        assert inspect.signature(facade.make_vec).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
