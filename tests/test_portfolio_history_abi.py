"""CPU-side checks of the portfolio env's episode history (finenv_portfolio_set_history; the C ABI of its
entry points is in tests/test_history_abi.py): the frame builders of finrl_amd.history reproduce the
frames the unmodified reference returned
(tests/golden/harness_portfolio_*.npz, written by tests/golden/make_golden_portfolio_history.py) from
the reference's own memories laid out as the device holds them."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
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
