"""CPU-side checks of the episode history of the cash-penalty and stop-loss envs
(finenv_{cashpenalty,stoploss}_set_history; the C ABI of their entry points is in
tests/test_history_abi.py): the frame builders of finrl_amd.history reproduce, from the reference's
recorded account_* / action_* columns of tests/golden/harness_sb3_*.npz laid out as the device holds
them, the frames save_asset_memory() / save_action_memory() return."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KINDS = ("cashpenalty", "stoploss")
FIXTURES = ("sb3_cashpenalty", "sb3_cashpenalty_patient", "sb3_stoploss", "sb3_stoploss_patient")


# ------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------
def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"harness_{name}.npz"), allow_pickle=False)


def _dates(T):
    return [f"D{t:03d}" for t in range(T)]


def _device_layout(z, lo, E, j, rng, pad=3):
    """The fixture's record as the device holds it for env j of E: time-major, junk in every other
    env's column and past ``length``, the fixture's frame rows [lo, lo + T) of a longer date list whose
    rows lo .. lo + T - 1 carry the fixture's own dates."""
    T, N = z["close"].shape
    n = len(z["account_cash"])
    cap = n + pad
    d = dict(cash=rng.normal(size=(cap, E)), asset_value=rng.normal(size=(cap, E)),
             reward=rng.normal(size=(cap, E)), tx=rng.normal(size=(cap, E, N)),
             actions=rng.normal(size=(cap, E, N)),
             start=rng.integers(0, 9, E).astype(np.int32), end=rng.integers(60, 70, E).astype(np.int32),
             ntx=rng.integers(0, 3, E).astype(np.int32), length=rng.integers(1, cap, E).astype(np.int32))
    d["cash"][:n, j], d["asset_value"][:n, j] = z["account_cash"], z["account_asset_value"]
    d["reward"][:n, j] = z["account_reward"]
    d["tx"][:n, j], d["actions"][:n, j] = z["action_transactions"], z["action_actions"]
    d["start"][j], d["end"][j], d["ntx"][j], d["length"][j] = lo, lo + T, n, n
    dates = _dates(lo) + [f"2020-{1 + t // 28:02d}-{1 + t % 28:02d}" for t in range(T)] + _dates(7)
    return d, dates, n


@pytest.mark.parametrize("name", FIXTURES)
def test_builders_return_the_reference_frames(name):
    from finrl_amd import history as H
    z = _fixture(name)
    rng = np.random.default_rng(len(name))
    E, j, lo = 5, 3, 11
    d, dates, n = _device_layout(z, lo, E, j, rng)
    assert n == z["close"].shape[0] - 1            # the loop reads the memories one day before the end
    am = H.dollar_asset_memory_frame(dates, d["cash"][:, j], d["asset_value"][:, j], d["reward"][:, j],
                                     d["end"][j], d["length"][j])
    assert am.columns.tolist() == ["cash", "asset_value", "total_assets", "reward", "date"]
    assert len(am) == n
    for k in ("cash", "asset_value", "total_assets", "reward"):
        assert am[k].dtype == np.float64
        np.testing.assert_array_equal(am[k].to_numpy(), z[f"account_{k}"], err_msg=k)
    # the date quirk: the LAST n dates of the env's own frame, not the dates the steps were taken on
    assert am["date"].tolist() == z["account_date"].tolist() == dates[lo + 1:lo + 1 + n]
    ac = H.dollar_action_memory_frame(dates, d["actions"][:, j], d["tx"][:, j], d["end"][j],
                                      d["length"][j], d["ntx"][j])
    assert ac.columns.tolist() == ["date", "actions", "transactions"] and len(ac) == n
    assert ac["date"].tolist() == z["action_date"].tolist()
    np.testing.assert_array_equal(np.stack(ac["actions"].tolist()), z["action_actions"])
    np.testing.assert_array_equal(np.stack(ac["transactions"].tolist()), z["action_transactions"])
    # a shorter record of the same env: the dates move with its length, the values do not
    am5 = H.dollar_asset_memory_frame(dates, d["cash"][:, j], d["asset_value"][:, j], d["reward"][:, j],
                                      d["end"][j], 5)
    assert am5["date"].tolist() == dates[lo + n - 4:lo + n + 1]
    np.testing.assert_array_equal(am5["cash"].to_numpy(), z["account_cash"][:5])
    # an empty record (current_step == 0): None from both
    assert H.dollar_asset_memory_frame(dates, d["cash"][:, j], d["asset_value"][:, j],
                                       d["reward"][:, j], d["end"][j], 0) is None
    assert H.dollar_action_memory_frame(dates, d["actions"][:, j], d["tx"][:, j], d["end"][j], 0, 0) is None
    # an episode ended by a cash shortage: one transaction row fewer, pandas' own ValueError
    with pytest.raises(ValueError, match="same length"):
        H.dollar_action_memory_frame(dates, d["actions"][:, j], d["tx"][:, j], d["end"][j], n, n - 1)


def test_stoploss_action_scaling():
    """actions_memory of the stop-loss env (:321-324): (a32 * hmax) * closings, the first product in
    float32 (the caller's dtype), the second in float64."""
    from finrl_amd import history as H
    rng = np.random.default_rng(3)
    n, N, hmax = 17, 6, 60000.0
    raw = rng.uniform(-1, 1, (n, N)).astype(np.float32)
    close = 50 * np.exp(rng.normal(0, 0.3, (40, N)))
    row = 9 + np.arange(n)
    got = H.stoploss_actions_memory(raw, hmax, close[row])
    assert got.dtype == np.float64 and got.shape == (n, N)
    for k in range(n):
        for i in range(N):
            a32 = np.float32(raw[k, i]) * np.float32(hmax)
            assert type(a32) is np.float32
            assert got[k, i] == np.float64(a32) * close[row[k], i], (k, i)
    # not the float64 product: the float32 rounding of a32 * hmax is visible
    assert (got != (raw.astype(np.float64) * hmax) * close[row]).any()


@pytest.mark.parametrize("kind", KINDS)
def test_readers_on_host_tensors(kind):
    """TwoWaveEpisodeHistory's readers over the same layout held in host tensors (no kernel runs: the
    object is assembled by hand): one env index gives one result, a sequence a list."""
    import torch
    from finrl_amd import _native as nat
    from finrl_amd import history as H
    z = _fixture("sb3_stoploss" if kind == "stoploss" else "sb3_cashpenalty")
    T, N = z["close"].shape
    rng = np.random.default_rng(11)
    E, j, lo, hmax = 5, 2, 6, 300.0
    d, dates, n = _device_layout(z, lo, E, j, rng)
    raw = rng.uniform(-1, 1, d["actions"].shape).astype(np.float32)
    d["actions"] = raw
    d["length"][0], d["ntx"][0], d["start"][0], d["end"][0] = 0, 0, 4, 30           # an empty record
    d["length"][4], d["ntx"][4], d["start"][4], d["end"][4] = 6, 5, 2, 20           # a cash shortage
    close = np.abs(rng.normal(50, 5, (len(dates), N)))
    hist = object.__new__(H.TwoWaveEpisodeHistory)
    hist.env = type("Env", (), dict(device=torch.device("cpu"), num_envs=E, _kind=kind,
                                    _cfg=type("Cfg", (), dict(hmax=hmax))(),
                                    panel=type("Panel", (), dict(dates=dates, close=close))()))()
    hist.capacity = d["cash"].shape[0]
    for k, v in d.items():
        setattr(hist, k, torch.from_numpy(v))
    hist.reason = torch.from_numpy(rng.integers(0, 64, (hist.capacity, E)).astype(np.int32))
    hist.flags = torch.full((E,), nat.HIST_ARMED, dtype=torch.int32)
    assert hist.nbytes == E * (28 * hist.capacity + 20) + 12 * E * N * hist.capacity
    assert hist.armed.all() and not hist.complete.any() and not hist.overflow.any()
    am = hist.save_asset_memory(j)
    np.testing.assert_array_equal(am["total_assets"].to_numpy(), z["account_total_assets"])
    assert am["date"].tolist() == z["account_date"].tolist()
    both = hist.save_asset_memory([0, j])
    assert isinstance(both, list) and both[0] is None and both[1].equals(am)
    np.testing.assert_array_equal(hist.account_values(j), z["account_total_assets"])
    np.testing.assert_array_equal(hist.rows(j), lo + np.arange(n))
    np.testing.assert_array_equal(hist.reasons(j), hist.reason[:n, j].numpy())
    np.testing.assert_array_equal(hist.raw_actions(j), raw[:n, j])
    np.testing.assert_array_equal(hist.transactions([4, j])[1], z["action_transactions"])
    assert hist.transactions(4).shape == (5, N) and hist.raw_actions(4).shape == (6, N)
    ac = hist.save_action_memory(j)
    want = raw[:n, j] if kind == "cashpenalty" else (raw[:n, j] * np.float32(hmax)) * close[lo:lo + n]
    got = np.stack(ac["actions"].tolist())
    assert got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.stack(ac["transactions"].tolist()), z["action_transactions"])
    assert hist.save_action_memory(0) is None
    with pytest.raises(ValueError, match="same length"):
        hist.save_action_memory(4)
    hist.tx = None                                         # transactions=False
    with pytest.raises(Exception, match="transactions=False"):
        hist.transactions(j)
    hist.actions = None
    with pytest.raises(Exception, match="actions=False"):
        hist.raw_actions(j)
    assert am.equals(hist.save_asset_memory(j))            # the account frame needs neither
