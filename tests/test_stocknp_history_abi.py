"""CPU-side checks of the array-state stock env's episode history (finenv_stocknp_set_history; the C ABI
of its entry points is in tests/test_history_abi.py): the builders and readers of finrl_amd.history
reproduce, from the reference-recorded total_asset / ta_tag of
tests/golden/stocknp_*.npz laid out as the device holds them, the list DRLAgent.DRL_prediction returns
(agents/elegantrl/models.py:105-131), element types included."""
import glob
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = sorted(os.path.basename(p)[len("stocknp_"):-4]
               for p in glob.glob(os.path.join(GOLDEN, "stocknp_*.npz")))
SCALARS = (float, np.float32, np.float64)          # FINENV_NT_PY / _F32 / _F64


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"stocknp_{name}.npz"), allow_pickle=False)


def _episodes(z):
    """(first step, last step) of every episode of the fixture: the steps between two ``reset_step``
    marks (-1: the reset before step 0) and those behind the last one."""
    marks = z["reset_step"].tolist() + [len(z["done"]) - 1]
    return [(a + 1, b) for a, b in zip(marks[:-1], marks[1:])]


def _initial(z, r):
    """total_asset and its tag behind the r-th reset (:93-95): amount0 + (stocks0 * price[0]).sum(),
    the sum a float32, in the dtype NumPy promotes the two to."""
    price0 = z["price_array"][0].astype(np.float32)
    hold = (z["reset_stocks0"][r] * price0).sum()
    assert type(hold) is np.float32
    amount = SCALARS[int(z["reset_amount0_tag"][r])](z["reset_amount0"][r])
    with np.errstate(over="ignore"):
        ta = amount + hold
    return ta


def _reference_list(z, r, s0, s1):
    """models.py:107-131 from the recorded scalars of steps s0 .. s1, types as the reference holds them."""
    out = [_initial(z, r)]
    for s in range(s0, s1 + 1):
        out.append(SCALARS[int(z["ta_tag"][s])](z["total_asset"][s]))
    returns = [x / out[0] for x in out[1:]]
    return out, returns


def _device_layout(z, r, s0, s1, lo, E, j, rng):
    """The record of steps s0 .. s1 as the device holds it for env j of E: time-major, junk in every
    other env's column and past ``length``, the env's rows offset by ``lo`` into a longer panel."""
    N = z["stocks"].shape[1]
    n = s1 - s0 + 2                                          # the armed entry and one per step
    cap = n + 3
    asset = rng.normal(size=(cap, E))
    tag = rng.integers(0, 3, (cap, E)).astype(np.uint8)
    stocks = rng.normal(size=(cap, N, E)).astype(np.float32)
    start, length = rng.integers(0, 99, E).astype(np.int32), rng.integers(1, cap, E).astype(np.int32)
    first = _initial(z, r)
    asset[0, j], tag[0, j], stocks[0, :, j] = float(first), SCALARS.index(type(first)), z["reset_stocks0"][r]
    asset[1:n, j], tag[1:n, j] = z["total_asset"][s0:s1 + 1], z["ta_tag"][s0:s1 + 1]
    stocks[1:n, :, j] = z["stocks"][s0:s1 + 1]
    start[j], length[j] = lo, n
    return dict(asset=asset, tag=tag, stocks=stocks, start=start, length=length), n


def _same_scalars(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert type(g) is type(w), (k, type(g), type(w))
        assert g == w, (k, g, w)


SEEN_KINDS = {}


@pytest.mark.parametrize("name", NAMES)
def test_builders_reproduce_the_reference_list_and_its_element_types(name):
    from finrl_amd import history as H
    assert len(NAMES) == 10
    z = _fixture(name)
    rng = np.random.default_rng(len(name))
    eps = _episodes(z)
    assert len(eps) == 3 and all(z["done"][b] for _, b in eps[:2])
    kinds = set()
    for r, ((s0, s1), j) in enumerate(zip(eps, (1, 2, 0))):
        lo, E = 5 + j, 4
        d, n = _device_layout(z, r, s0, s1, lo, E, j, rng)
        want, want_ret = _reference_list(z, r, s0, s1)
        kinds |= {type(x) for x in want}
        # the fixture's initial total asset is the one the env latched: episode_return of the terminal
        # step is total_asset / initial_total_asset (:145)
        if z["done"][s1]:
            assert float(want_ret[-1]) == z["episode_return"][s1]
        got = H.stocknp_episode_total_assets(d["asset"][:, j], d["tag"][:, j], d["length"][j])
        _same_scalars(got, want)
        _same_scalars(H.stocknp_episode_returns(d["asset"][:, j], d["tag"][:, j], d["length"][j]), want_ret)
        # without the tags: the same values as Python floats
        plain = H.stocknp_episode_total_assets(d["asset"][:, j], None, n)
        _same_scalars(plain, [float(x) for x in want])
        _same_scalars(H.stocknp_episode_returns(d["asset"][:, j], None, n),
                      [float(x) / float(want[0]) for x in want[1:]])
        av = H.stocknp_account_values(d["asset"][:, j], d["length"][j])
        assert av.dtype == np.float64 and av.shape == (n,)
        np.testing.assert_array_equal(av[1:], z["total_asset"][s0:s1 + 1])
        pos = H.crypto_positions(d["stocks"][:, :, j], d["length"][j])
        assert pos.dtype == np.float32 and pos.shape == (n, z["stocks"].shape[1])
        np.testing.assert_array_equal(pos[1:], z["stocks"][s0:s1 + 1])
        rows = H.crypto_rows(d["start"][j], d["length"][j])
        np.testing.assert_array_equal(rows[1:], lo + z["day"][s0:s1 + 1])
        assert rows[0] == lo
        # a record of one entry (an env armed and not stepped yet)
        _same_scalars(H.stocknp_episode_total_assets(d["asset"][:, j], d["tag"][:, j], 1), want[:1])
        assert H.stocknp_episode_returns(d["asset"][:, j], d["tag"][:, j], 1) == []
    SEEN_KINDS[name] = kinds
    if name in ("eval_n3", "nas100_dow30"):
        assert {np.float32, np.float64} <= kinds, kinds      # both kinds of NumPy scalar were seen


@pytest.mark.parametrize("name", NAMES)
def test_readers_on_host_tensors(name):
    """StockNpEpisodeHistory's readers over the same layout held in host tensors (no kernel runs: the
    object is assembled by hand): one env index gives one result, a sequence a list."""
    import torch
    from finrl_amd import history as H
    z = _fixture(name)
    rng = np.random.default_rng(7)
    (s0, s1), (t0, t1) = _episodes(z)[:2]
    E, lo = 5, 11
    d, n = _device_layout(z, 0, s0, s1, lo, E, 3, rng)
    d2, _ = _device_layout(z, 1, t0, t1, lo, E, 0, rng)
    for k in ("asset", "tag", "start", "length"):
        d[k][..., 0] = d2[k][..., 0]
    d["stocks"][:, :, 0] = d2["stocks"][:, :, 0]
    hist = object.__new__(H.StockNpEpisodeHistory)
    hist.env = type("Env", (), dict(device=torch.device("cpu"), num_envs=E))()
    hist.capacity = d["asset"].shape[0]
    for k, v in d.items():
        setattr(hist, k, torch.from_numpy(v))
    hist.flags = torch.zeros(E, dtype=torch.int32)
    N = z["stocks"].shape[1]
    assert hist.nbytes == E * (9 * hist.capacity + 12) + 4 * E * N * hist.capacity
    w3, r3 = _reference_list(z, 0, s0, s1)
    w0, r0 = _reference_list(z, 1, t0, t1)
    _same_scalars(hist.episode_total_assets(3), w3)
    both = hist.episode_total_assets([0, 3])
    assert isinstance(both, list) and len(both) == 2
    _same_scalars(both[0], w0)
    _same_scalars(both[1], w3)
    _same_scalars(hist.episode_returns(3), r3)
    _same_scalars(hist.episode_returns([3, 0])[1], r0)
    np.testing.assert_array_equal(hist.account_values(0), np.array([float(x) for x in w0]))
    pos = hist.positions([0, 3])
    np.testing.assert_array_equal(pos[0][1:], z["stocks"][t0:t1 + 1])
    np.testing.assert_array_equal(pos[1][1:], z["stocks"][s0:s1 + 1])
    np.testing.assert_array_equal(hist.rows(3), lo + np.arange(n))
    hist.tag = None                                          # tags=False: Python floats
    _same_scalars(hist.episode_total_assets(3), [float(x) for x in w3])
    hist.stocks = None
    with pytest.raises(Exception, match="stocks=False"):
        hist.positions(0)


def test_harness_lists_from_their_recorded_values():
    """harness_erl_stocknp.npz holds the two lists of the reference's prediction loop as float64
    arrays: recorded values laid out as a history give them back, whatever the tags say about the
    scalar types (a float32 quotient widened is the fixture's entry: tags 1 throughout; float64: 2)."""
    from finrl_amd import history as H
    z = np.load(os.path.join(GOLDEN, "harness_erl_stocknp.npz"), allow_pickle=False)
    want, want_ret = z["episode_total_assets"], z["episode_returns"]
    n = len(want)
    assert len(want_ret) == n - 1
    asset = np.concatenate([want, [-1.0, -2.0]])
    # the tags of the fixture's scalars: a value that is no float32 cannot have been one
    is32 = want.astype(np.float32).astype(np.float64) == want
    tag = np.where(is32, 1, 2).astype(np.uint8)
    tag = np.concatenate([tag, [0, 0]]).astype(np.uint8)
    got = H.stocknp_episode_total_assets(asset, tag, n)
    np.testing.assert_array_equal(np.asarray(got, np.float64), want)
    np.testing.assert_array_equal(H.stocknp_account_values(asset, n), want)
    # the quotient's dtype follows the two tags; the fixture's returns are one of the candidates the
    # tags admit for every entry, and with the tags NumPy itself would have produced: exactly equal
    ret = H.stocknp_episode_returns(asset, tag, n)
    first = got[0]
    for k, x in enumerate(got[1:]):
        assert type(ret[k]) is type(x / first) and ret[k] == x / first
    np.testing.assert_array_equal(np.asarray(ret, np.float64), want_ret)
