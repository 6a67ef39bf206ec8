"""CPU-side checks of the crypto env's episode history (finenv_crypto_set_history; the C ABI of its entry
points is in tests/test_history_abi.py): the builders and readers of finrl_amd.history reproduce, from the
reference-recorded state of tests/golden/crypto_*.npz laid out as the device holds it, the true account
value and the list DRLAgent.DRL_prediction_load_from_file builds
(agents/stablebaselines3/models.py:146-156)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("n1", "n9_poor", "pairs10", "lookback3")


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"crypto_{name}.npz"), allow_pickle=False)


def _episodes(z):
    """(first step, last step) of every finished episode of the fixture: the steps between two
    ``reset_step`` marks (-1: the reset before step 0)."""
    marks = z["reset_step"].tolist()
    return [(a + 1, b) for a, b in zip(marks[:-1], marks[1:])]


def _reference_list(z, s0, s1, initial_total_asset):
    """models.py:146-156 over the recorded state of steps s0 .. s1, expression for expression."""
    episode_total_assets = [initial_total_asset]
    for s in range(s0, s1 + 1):
        total_asset = initial_total_asset + (z["price"][z["time"][s]] * z["stocks"][s]).sum()
        episode_total_assets.append(total_asset)
    return episode_total_assets


def _device_layout(z, s0, s1, lo, E, j, rng):
    """The record of steps s0 .. s1 as the device holds it for env j of E: time-major, junk in every
    other env's column and past ``length``, the env's rows offset by ``lo`` into a longer panel."""
    T, N, W, S, L = z["cfg_int"].tolist()
    cap0 = z["cfg_float"][0]
    n = s1 - s0 + 2                                          # the armed entry and one per step
    cap = n + 3
    asset, hold = rng.normal(size=(cap, E)), rng.normal(size=(cap, E))
    stocks = rng.normal(size=(cap, N, E)).astype(np.float32)
    start, length = rng.integers(0, 99, E).astype(np.int32), rng.integers(1, cap, E).astype(np.int32)
    asset[0, j], hold[0, j], stocks[0, :, j] = cap0, 0.0, 0.0
    for k, s in enumerate(range(s0, s1 + 1), start=1):
        asset[k, j] = z["total_asset"][s]
        hold[k, j] = (z["stocks"][s] * z["price"][z["time"][s]]).sum()      # :82
        stocks[k, :, j] = z["stocks"][s]
    start[j], length[j] = lo + L - 1, n
    return dict(asset=asset, holdings=hold, stocks=stocks, start=start, length=length), n


@pytest.mark.parametrize("name", FIXTURES)
def test_builders_reproduce_the_account_value_and_the_reference_list(name):
    from finrl_amd import history as H
    z = _fixture(name)
    T, N, W, S, L = z["cfg_int"].tolist()
    cap0 = float(z["cfg_float"][0])
    rng = np.random.default_rng(T + N)
    # the consistency premise: the fixture's total_asset is cash + np.sum(stocks * price[time]) (:82)
    hold_all = np.array([(z["stocks"][s] * z["price"][z["time"][s]]).sum() for s in range(S)])
    np.testing.assert_array_equal(z["cash"] + hold_all, z["total_asset"])
    assert (hold_all != 0).mean() >= 7 / 9                  # 0.78 .. 1.0: the holdings column is exercised
    eps = _episodes(z)
    assert len(eps) == 2 and all(z["done"][b] for _, b in eps)
    for (s0, s1), j in zip(eps, (1, 2)):
        lo, E = 5 + j, 4
        d, n = _device_layout(z, s0, s1, lo, E, j, rng)
        assert n == T - 2 * L + 1
        av = H.crypto_account_values(d["asset"][:, j], d["length"][j])
        assert av.dtype == np.float64 and av.shape == (n,) and av[0] == cap0
        np.testing.assert_array_equal(av[1:], z["total_asset"][s0:s1 + 1])
        got = H.crypto_episode_total_assets(d["holdings"][:, j], d["length"][j], cap0)
        want = _reference_list(z, s0, s1, cap0)
        assert all(type(x) is float for x in got) and got == [float(x) for x in want]
        assert got[0] == cap0 and len(got) == n
        # the reference's list is NOT the account value once cash has been spent
        if (z["cash"][s0:s1 + 1] != cap0).any():
            assert got != av.tolist()
        # another initial_total_asset shifts every entry (the reference reads the env's attribute)
        assert H.crypto_episode_total_assets(d["holdings"][:, j], n, 5.0) == \
            [float(x) for x in _reference_list(z, s0, s1, 5.0)]
        pos = H.crypto_positions(d["stocks"][:, :, j], d["length"][j])
        assert pos.dtype == np.float32 and pos.shape == (n, N) and not pos[0].any()
        np.testing.assert_array_equal(pos[1:], z["stocks"][s0:s1 + 1])
        rows = H.crypto_rows(d["start"][j], d["length"][j])
        np.testing.assert_array_equal(rows[1:], lo + z["time"][s0:s1 + 1])
        assert rows[0] == lo + L - 1 and (np.diff(rows) == 1).all()
        # a record of one entry (an env armed and not stepped yet)
        assert H.crypto_episode_total_assets(d["holdings"][:, j], 1, cap0) == [cap0]
        assert H.crypto_account_values(d["asset"][:, j], 1).tolist() == [cap0]
        assert H.crypto_positions(d["stocks"][:, :, j], 1).shape == (1, N)
        assert H.crypto_rows(d["start"][j], 1).tolist() == [lo + L - 1]


@pytest.mark.parametrize("name", FIXTURES)
def test_readers_on_host_tensors(name):
    """CryptoEpisodeHistory's readers over the same layout held in host tensors (no kernel runs: the
    object is assembled by hand): one env index gives one result, a sequence a list, and the
    [capacity, N, E] holdings come back per env as [length, N]."""
    import torch
    from finrl_amd import history as H
    z = _fixture(name)
    T, N, W, S, L = z["cfg_int"].tolist()
    cap0 = float(z["cfg_float"][0])
    rng = np.random.default_rng(N)
    (s0, s1), (t0, t1) = _episodes(z)
    E, lo = 5, 11
    d, n = _device_layout(z, s0, s1, lo, E, 3, rng)
    d2, _ = _device_layout(z, t0, t1, lo, E, 0, rng)
    for k in ("asset", "holdings", "start", "length"):
        d[k][..., 0] = d2[k][..., 0]
    d["stocks"][:, :, 0] = d2["stocks"][:, :, 0]
    hist = object.__new__(H.CryptoEpisodeHistory)
    hist.env = type("Env", (), dict(device=torch.device("cpu"), initial_cash=cap0, num_envs=E))()
    hist.capacity = d["asset"].shape[0]
    for k, v in d.items():
        setattr(hist, k, torch.from_numpy(v))
    hist.flags = torch.zeros(E, dtype=torch.int32)
    assert hist.nbytes == E * (16 * hist.capacity + 12) + 4 * E * N * hist.capacity
    one = hist.account_values(3)
    np.testing.assert_array_equal(one[1:], z["total_asset"][s0:s1 + 1])
    both = hist.account_values([0, 3])
    assert isinstance(both, list) and len(both) == 2
    np.testing.assert_array_equal(both[0][1:], z["total_asset"][t0:t1 + 1])
    np.testing.assert_array_equal(both[1], one)
    assert hist.episode_total_assets(3) == [float(x) for x in _reference_list(z, s0, s1, cap0)]
    assert hist.episode_total_assets([3, 0], 7.0) == [
        [float(x) for x in _reference_list(z, s0, s1, 7.0)],
        [float(x) for x in _reference_list(z, t0, t1, 7.0)]]
    pos = hist.positions([0, 3])
    np.testing.assert_array_equal(pos[0][1:], z["stocks"][t0:t1 + 1])
    np.testing.assert_array_equal(pos[1][1:], z["stocks"][s0:s1 + 1])
    np.testing.assert_array_equal(hist.rows(3), lo + L - 1 + np.arange(n))
    hist.stocks = None
    with pytest.raises(Exception, match="stocks=False"):
        hist.positions(0)
