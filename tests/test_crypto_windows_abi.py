"""CPU-side checks of the per-env episode windows of the batched crypto env: the header declares
finenv_crypto_set_windows and the library exports it, the setter validates its arguments without a
GPU, the ABI version, the crypto struct sizes and field enums are those of v3, the per-row
normaliser table equals action_norm_vector row by row, and the Python classes expose the API."""
import ctypes as C
import numpy as np
import pytest

import abi_header as H


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def test_header_declares_and_library_exports_set_windows(L):
    assert H.prototypes()["finenv_crypto_set_windows"] == \
        ("int", [("finenv_crypto *", "h"), ("int32_t *", "win"), ("const double *", "norm_rows")])
    assert hasattr(L, "finenv_crypto_set_windows")


def test_set_windows_validates_handle_and_table(L):
    from finrl_amd import _native as nat
    win = np.zeros((4, 70), dtype=np.int32)
    norm = np.ones((40, 10))
    wp, npp = win.ctypes.data_as(C.c_void_p), norm.ctypes.data_as(C.c_void_p)
    assert L.finenv_crypto_set_windows(None, None, None) == -1
    assert L.finenv_crypto_set_windows(None, wp, npp) == -1
    h = C.c_void_p()
    cfg = nat.CryptoConfig(70, 10, 40, 40, 1, 0, 1e6, 1e-3, 1e-3, 0.99)
    assert L.finenv_crypto_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # attaching and detaching work before bind (the block is only read by launches)
        assert L.finenv_crypto_set_windows(h, wp, npp) == 0
        assert L.finenv_crypto_set_windows(h, None, None) == 0
        assert L.finenv_crypto_set_windows(h, None, npp) == 0          # detaching ignores the table
        assert L.finenv_crypto_set_windows(h, wp, npp) == 0
        # a window block needs the normaliser table
        assert L.finenv_crypto_set_windows(h, wp, None) == -1
        assert b"norm_rows" in L.finenv_crypto_last_error(h)
        # launches still need the bound state
        assert L.finenv_crypto_reset(h, None, None, None) == -2
    finally:
        L.finenv_crypto_destroy(h)


def test_abi_version_struct_sizes_and_enums_unchanged(L):
    from finrl_amd import _native as nat
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    assert H.constants()["FINENV_ABI_VERSION"] == 3
    cls = (nat.CryptoConfig, nat.CryptoPanelPtrs, nat.CryptoStatePtrs)
    for which, c in zip((6, 7, 8), cls):
        assert L.finenv_struct_size(which) == C.sizeof(c)
    assert tuple(C.sizeof(c) for c in cls) == (56, 24, 24)
    assert H.enum("FINENV_CRYPTO_F64_FIELDS") == [
        "FINENV_CF_CASH", "FINENV_CF_TOTAL_ASSET", "FINENV_CF_GAMMA_RETURN", "FINENV_CF_EPISODE_RETURN",
        "FINENV_CF_LAST_REWARD", "FINENV_CRYPTO_F64_FIELDS"]
    assert H.enum("FINENV_CRYPTO_I32_FIELDS") == ["FINENV_CI_TIME", "FINENV_CRYPTO_I32_FIELDS"]
    assert nat.CRYPTO_F64_FIELDS == ("cash", "total_asset", "gamma_return", "episode_return",
                                     "last_reward")
    assert nat.CRYPTO_I32_FIELDS == ("time",)


def test_norm_table_equals_action_norm_vector_row_by_row():
    """Row r of the table is action_norm_vector(price[r]) bit for bit, also at the prices where a
    vectorised log10 floors differently from math.log(p, 10) (exact powers of ten); rows with a
    price that is not positive are NaN and raise nothing."""
    from finrl_amd.vec_crypto import action_norm_table, action_norm_vector
    from oracle.crypto import action_norm_vector as oracle_norm
    rng = np.random.default_rng(11)
    T, N = 300, 6
    price = 10.0 ** rng.uniform(-6, 16, (T, N))
    price[0] = [1000.0, 1e6, 1e-3, 0.1, 1e15, 1.0]
    price[1] = [10.0, 100.0, 1e-2, 1e3, 1e-6, 1e9]
    price[17] = np.nextafter(price[0], 0)                 # just below the powers of ten
    price[18] = np.nextafter(price[0], np.inf)
    zero_rows = (5, 40, T - 1)
    for k, r in enumerate(zero_rows):
        price[r, k] = 0.0
    price[60, 2] = -3.0
    price[61, 4] = np.nan
    table = action_norm_table(price)
    assert table.shape == (T, N) and table.dtype == np.float64
    for r in range(T):
        if r in zero_rows + (60, 61):
            assert np.isnan(table[r]).all(), r
            continue
        want = oracle_norm(price[r])
        assert table[r].tobytes() == want.tobytes(), (r, table[r], want)
        assert table[r].tobytes() == action_norm_vector(price[r]).tobytes()
    # the cases a vectorised restatement gets wrong on this platform are in the panel
    assert table[0, 0] == 1e4 / 10 ** 2 and np.floor(np.log10(1000.0)) == 3


def test_env_exposes_the_window_api():
    import inspect
    from finrl_amd.vec_base import WindowedEnv
    from finrl_amd.vec_crypto import VecCryptoEnv
    from finrl_amd.vec_env import VecStockTradingEnv
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    assert "windows" in inspect.signature(VecCryptoEnv.__init__).parameters
    for m in ("set_windows", "window_time", "norm_table"):
        assert callable(getattr(VecCryptoEnv, m)), m
    assert list(inspect.signature(VecCryptoEnv.set_windows).parameters) == ["self", "start", "end", "mask"]
    # one copy of the host-side window code for the three envs
    for cls in (VecCryptoEnv, VecStockTradingEnv, VecStockPortfolioEnv):
        assert issubclass(cls, WindowedEnv)
        assert cls._check_windows is WindowedEnv._check_windows


def test_shard_env_kwargs_slices_windows():
    from finrl_amd.distributed import shard_env_kwargs, shard_range
    E = 11
    s, t = np.arange(E), np.arange(E) + 7
    for rank in range(3):
        lo, hi = shard_range(E, rank, 3)
        n, kw = shard_env_kwargs(E, rank, 3, windows=(s, t), gamma=0.9)
        assert n == hi - lo and kw["gamma"] == 0.9
        np.testing.assert_array_equal(kw["windows"][0], s[lo:hi])
        np.testing.assert_array_equal(kw["windows"][1], t[lo:hi])
    n, kw = shard_env_kwargs(E, 1, 3, windows=(2, t))         # one start for all envs passes through
    assert kw["windows"][0] == 2 and len(kw["windows"][1]) == n
    assert "windows" not in shard_env_kwargs(E, 0, 2, gamma=0.9)[1]
