"""CPU-side checks of the stock env's episode history (finenv_stock_set_history; the C ABI of its entry
points is in tests/test_history_abi.py): a step that records actions needs `realised`, and the frame
builders of finrl_amd.history reproduce the reference's frames (tests/golden/harness_sb3_stock.npz) from
hand-made host arrays."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def _cfg(nat, E=64, N=30):
    return nat.StockConfig(E, N, 8, 100, 100, 0, 1, 1, 1, int(N == 1), 1e-3, 1e-3, 1e-4, 0.0)


def _host_history(nat, E=64, N=30, cap=5, actions=True):
    """A history struct over host arrays: enough for the argument checks, which never launch."""
    bufs = dict(asset=np.zeros((cap, E)), row=np.zeros((cap, E), np.int32),
                actions=np.zeros((cap - 1, E, N), np.int32), len=np.zeros(E, np.int32),
                flags=np.zeros(E, np.int32))
    ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in bufs.items()}
    hist = nat.StockHistoryPtrs(ptr["asset"], ptr["row"], ptr["actions"] if actions else None,
                                ptr["len"], ptr["flags"], cap)
    return hist, bufs


def test_step_with_recorded_actions_needs_realised(L):
    """A history that records actions needs step()'s `realised` output: the step refuses before it
    launches anything.  (bind only keeps pointers, so host arrays do for this check.)"""
    from finrl_amd import _native as nat
    E, N, K, T = 64, 30, 8, 100
    D = 1 + 2 * N + K * N
    hist, _ = _host_history(nat, E, N)
    panel = [np.zeros((T, N)), np.zeros((T, D), np.float32), np.zeros(T)]
    state = [np.zeros((len(nat.STOCK_F64_FIELDS), E)),
             np.zeros((len(nat.STOCK_I32_FIELDS) + 2 * N, E), np.int32)]
    pp = nat.StockPanelPtrs(*(a.ctypes.data_as(C.c_void_p) for a in panel))
    sp = nat.StockStatePtrs(*(a.ctypes.data_as(C.c_void_p) for a in state))
    io = [np.zeros((E, N), np.float32), np.zeros((E, D), np.float32), np.zeros(E, np.float32),
          np.zeros(E, np.uint8)]
    a, o, r, d = (x.ctypes.data_as(C.c_void_p) for x in io)
    h = C.c_void_p()
    cfg = _cfg(nat, E, N)
    assert L.finenv_stock_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.finenv_stock_set_history(h, C.byref(hist)) == 0
        # unbound: the existing answer
        assert L.finenv_stock_step(h, a, o, r, d, None, None, 1, None) == -2
        assert L.finenv_stock_bind(h, C.byref(pp), C.byref(sp)) == 0
        assert L.finenv_stock_step(h, a, o, r, d, None, None, 1, None) == -1
        assert b"realised" in L.finenv_stock_last_error(h)
    finally:
        L.finenv_stock_destroy(h)


def _sb3():
    return np.load(os.path.join(GOLDEN, "harness_sb3_stock.npz"), allow_pickle=False)


def test_frame_builders_reproduce_the_reference_frames():
    """asset / row / actions columns as the device holds them (time-major, padded past `length`, the
    env's rows offset into a longer panel) -> the frames DRL_prediction returned for the reference env."""
    from finrl_amd import history as H
    z = _sb3()
    n = len(z["account_value"])
    N = z["actions"].shape[1]
    lo, cap = 4, n + 3
    dates = [f"pre{t}" for t in range(lo)] + z["account_date"].tolist() + ["post0", "post1"]
    tickers = z["action_columns"].tolist()
    asset = np.full(cap, np.nan)
    asset[:n] = z["account_value"]
    row = np.full(cap, -1, np.int32)
    row[:n] = lo + np.arange(n)
    actions = np.full((cap - 1, N), 99, np.int32)
    actions[:n - 1] = z["actions"]

    acct = H.asset_memory_frame(dates, asset, row, n)
    assert acct.columns.tolist() == ["date", "account_value"] and len(acct) == n
    assert acct["date"].tolist() == z["account_date"].tolist()
    np.testing.assert_array_equal(acct["account_value"].to_numpy(np.float64), z["account_value"])

    acts = H.action_memory_frame(dates, tickers, actions, row, n)
    np.testing.assert_array_equal(acts.to_numpy(np.int64), z["actions"])
    assert acts.index.tolist() == z["action_date"].tolist()
    assert acts.columns.tolist() == z["action_columns"].tolist()
    assert str(acts.index.name) == str(z["action_index_name"])

    av = H.account_value_frame(dates, asset, row, n)
    assert av.columns.tolist() == ["account_value", "date", "daily_return"]
    assert av["date"].tolist() == z["account_date"].tolist()
    np.testing.assert_array_equal(av["account_value"].to_numpy(), z["account_value"])
    a = z["account_value"]
    assert np.isnan(av["daily_return"][0])
    np.testing.assert_array_equal(av["daily_return"].to_numpy()[1:], a[1:] / a[:-1] - 1)

    # a record cut short (an armed env before its first step, two entries)
    one = H.asset_memory_frame(dates, asset, row, 1)
    assert one["account_value"].tolist() == [a[0]] and one["date"].tolist() == [z["account_date"][0]]
    assert H.action_memory_frame(dates, tickers, actions, row, 1).shape == (0, N)
    assert H.action_memory_frame(dates, tickers, actions, row, 2).shape == (1, N)


def test_single_ticker_action_frame_shape():
    """One ticker in the frame: {"date", "actions"} with one [1] array per day (:536-542)."""
    from finrl_amd import history as H
    dates = [f"d{t}" for t in range(6)]
    row = np.arange(6, dtype=np.int32)
    actions = np.array([[3], [-2], [0], [7], [9]], np.int32)
    df = H.action_memory_frame(dates, ["ONLY"], actions, row, 5)
    assert df.columns.tolist() == ["date", "actions"] and df.shape == (4, 2)
    assert df["date"].tolist() == dates[:4]
    assert [x.tolist() for x in df["actions"]] == [[3], [-2], [0], [7]]
    assert list(df.index) == [0, 1, 2, 3]


def test_validation_sharpe_special_cases():
    from finrl_amd import history as H
    got = H.validation_sharpe_from([0.01, 0.0, -0.01, 0.02, np.nan], [0.0, 0.0, 0.0, 0.04, np.nan])
    assert got[0] == np.inf and got[1] == 0.0 and got[2] == 0.0
    assert got[3] == (4 ** 0.5) * 0.02 / 0.04 and np.isnan(got[4])
