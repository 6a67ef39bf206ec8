"""CPU-side checks of the portfolio env's episode history (finenv_portfolio_set_history): the header
declares the struct and the three entry points and the library exports them, ABI version and struct
sizes are unchanged, the entry points validate their arguments without a GPU, and the frame builders of
finrl_amd.history reproduce the frames the unmodified reference returned
(tests/golden/harness_portfolio_*.npz, written by tests/golden/make_golden_portfolio_history.py) from
the reference's own memories laid out as the device holds them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "finenv.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def _host_history(nat, E=64, N=5, cap=5, weights=True):
    """A history struct over host arrays: enough for the argument checks, which never launch."""
    bufs = dict(value=np.zeros((cap, E)), ret=np.zeros((cap, E)), row=np.zeros((cap, E), np.int32),
                weights=np.zeros((cap, E, N), np.float32), len=np.zeros(E, np.int32),
                flags=np.zeros(E, np.int32))
    ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in bufs.items()}
    hist = nat.PortfolioHistoryPtrs(ptr["value"], ptr["ret"], ptr["row"],
                                    ptr["weights"] if weights else None, ptr["len"], ptr["flags"], cap)
    return hist, bufs


def test_header_declares_and_library_exports_the_history_api(L):
    hdr = open(HDR).read()
    for fn in ("finenv_portfolio_set_history", "finenv_portfolio_history_arm",
               "finenv_portfolio_history_metrics"):
        assert re.search(rf"\bint\s+{fn}\s*\(", hdr), fn
        assert hasattr(L, fn), fn
    m = re.search(r"typedef struct finenv_portfolio_history \{(.*?)\} finenv_portfolio_history;", hdr,
                  flags=re.S)
    assert m, "struct finenv_portfolio_history"
    fields = re.findall(r"^\s*(double|int32_t|float)\s+\*?(\w+);", m.group(1), flags=re.M)
    assert fields == [("double", "value"), ("double", "ret"), ("int32_t", "row"), ("float", "weights"),
                      ("int32_t", "len"), ("int32_t", "flags"), ("int32_t", "capacity")]
    from finrl_amd import _native as nat
    assert [f[0] for f in nat.PortfolioHistoryPtrs._fields_] == [f[1] for f in fields]
    assert nat.PORTFOLIO_HISTORY_METRICS == ("n_returns", "cumulative_return", "mean", "std", "sharpe",
                                             "max_drawdown")
    # additive: same ABI version, same v3 structs
    assert "#define FINENV_ABI_VERSION 3" in hdr
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    sizes = [72, 24, 16, 24, 16, 16, 56, 24, 24, 72, 24, 24, 80, 24, 16, 96, 24, 16]
    assert [L.finenv_struct_size(i) for i in range(18)] == sizes
    assert L.finenv_struct_size(18) == -1


def test_entry_points_validate_arguments(L):
    from finrl_amd import _native as nat
    hist, bufs = _host_history(nat)
    out = np.zeros((64, 6))
    outp = out.ctypes.data_as(C.c_void_p)
    # NULL handle
    assert L.finenv_portfolio_set_history(None, C.byref(hist)) == -1
    assert L.finenv_portfolio_history_arm(None, None, None) == -1
    assert L.finenv_portfolio_history_metrics(None, 2.0, outp, None) == -1
    h = C.c_void_p()
    cfg = nat.PortfolioConfig(64, 5, 4, 50, 1e6)
    assert L.finenv_portfolio_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # nothing attached (the default): arm / metrics refuse, with a message
        assert L.finenv_portfolio_history_arm(h, None, None) == -1
        assert b"no history attached" in L.finenv_portfolio_last_error(h)
        assert L.finenv_portfolio_history_metrics(h, 2.0, outp, None) == -1
        assert b"no history attached" in L.finenv_portfolio_last_error(h)
        # a NULL mandatory pointer, capacity < 2
        for name in ("value", "ret", "row", "len", "flags"):
            bad, _ = _host_history(nat)
            setattr(bad, name, None)
            assert L.finenv_portfolio_set_history(h, C.byref(bad)) == -1, name
            assert b"null" in L.finenv_portfolio_last_error(h)
        for cap in (1, 0, -3):
            bad, _ = _host_history(nat)
            bad.capacity = cap
            assert L.finenv_portfolio_set_history(h, C.byref(bad)) == -1, cap
            assert b"capacity" in L.finenv_portfolio_last_error(h)
        # a refused struct attaches nothing
        assert L.finenv_portfolio_history_arm(h, None, None) == -1
        # attaching works before bind (weights may be NULL); arm / metrics then need the bound state
        now, _ = _host_history(nat, weights=False)
        assert L.finenv_portfolio_set_history(h, C.byref(now)) == 0
        assert L.finenv_portfolio_set_history(h, C.byref(hist)) == 0
        assert L.finenv_portfolio_history_arm(h, None, None) == -2
        assert L.finenv_portfolio_history_metrics(h, 2.0, outp, None) == -2
        assert L.finenv_portfolio_history_metrics(h, 2.0, None, None) == -1
        # NULL detaches again
        assert L.finenv_portfolio_set_history(h, None) == 0
        assert L.finenv_portfolio_history_arm(h, None, None) == -1
        assert L.finenv_portfolio_history_metrics(h, 2.0, outp, None) == -1
    finally:
        L.finenv_portfolio_destroy(h)
    assert not any(b.any() for b in bufs.values())


FIXTURES = ("dow30", "n5", "n2k1", "const")


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"harness_portfolio_{name}.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", FIXTURES)
def test_frame_builders_reproduce_the_reference_frames(name):
    """The unmodified reference env's own memories on the second-to-last day of DRL_prediction
    (tests/golden/harness_portfolio_<name>.npz), laid out as the device holds them -- time-major columns
    padded past `length`, the env's rows offset into a longer panel, weights in float32 with the armed
    float32(1 / N) first row -> the two frames DRL_prediction returned: values, `date` column / index,
    column names, index name, dtypes; row 0 of the action frame is exactly 1 / N."""
    from finrl_amd import history as H
    z = _fixture(name)
    T, N, K = z["cfg_int"].tolist()
    n, lo, cap = T, 3, T + 2
    assert len(z["asset_memory"]) == len(z["portfolio_return_memory"]) == len(z["date_memory"]) == n
    assert z["actions_memory"].shape == (n, N)
    # the fixture's memories are consistent with each other as the reference builds them (:187-193)
    a, r = z["asset_memory"], z["portfolio_return_memory"]
    assert r[0] == 0 and a[0] == z["cfg_float"][0]
    np.testing.assert_array_equal(a[1:], a[:-1] * (1 + r[1:]))
    dates = [f"pre{t}" for t in range(lo)] + z["dates"].tolist() + ["post0", "post1"]
    tickers = z["tickers"].tolist()
    ret = np.full(cap, np.nan)
    ret[:n] = r
    row = np.full(cap, -1, np.int32)
    row[:n] = lo + np.arange(n)
    w = np.full((cap, N), 7.0, np.float32)
    w[:n] = z["actions_memory"].astype(np.float32)      # rows 1.. are float32 in the reference: exact
    np.testing.assert_array_equal(w[1:n].astype(np.float64), z["actions_memory"][1:])
    assert (w[0] == np.float32(1 / N)).all()
    assert [dates[i] for i in row[:n]] == z["date_memory"].tolist()

    acct = H.portfolio_asset_memory_frame(dates, ret, row, n)
    assert acct.columns.tolist() == z["account_columns"].tolist() == ["date", "daily_return"]
    assert acct["date"].tolist() == z["account_date"].tolist() and len(acct) == n
    assert [str(t) for t in acct.dtypes] == z["account_dtypes"].tolist()
    np.testing.assert_array_equal(acct["daily_return"].to_numpy(), z["account_daily_return"])

    acts = H.portfolio_action_memory_frame(dates, tickers, w, row, n)
    assert acts.columns.tolist() == z["action_columns"].tolist()
    assert acts.index.tolist() == z["action_index"].tolist()
    assert str(acts.index.name) == str(z["action_index_name"]) == "date"
    assert [str(t) for t in acts.dtypes] == z["action_dtypes"].tolist()
    np.testing.assert_array_equal(acts.to_numpy(), z["action_values"])
    assert (acts.to_numpy()[0] == 1 / N).all()

    # a record of one entry (an env armed and not stepped yet)
    one = H.portfolio_asset_memory_frame(dates, ret, row, 1)
    assert one["daily_return"].tolist() == [0] and one["date"].tolist() == [dates[lo]]
    assert H.portfolio_action_memory_frame(dates, tickers, w, row, 1).shape == (1, N)
    # a first row that is not the armed 1 / N is kept as recorded
    w2 = w.copy()
    w2[0, 0] = np.float32(0.25)
    got = H.portfolio_action_memory_frame(dates, tickers, w2, row, 2).to_numpy()
    np.testing.assert_array_equal(got, w2[:2].astype(np.float64))


def test_constant_close_fixture_has_zero_returns_and_no_sharpe():
    """The scenario whose closes are constant: every return of the reference is exactly 0 and its
    terminal branch prints no Sharpe (std == 0, :147); the other scenarios print one."""
    z = _fixture("const")
    assert (z["portfolio_return_memory"] == 0).all() and (z["asset_memory"] == z["cfg_float"][0]).all()
    assert not any("Sharpe" in ln for ln in z["printout"].tolist())
    for name in FIXTURES[:3]:
        assert sum("Sharpe" in ln for ln in _fixture(name)["printout"].tolist()) == 1
