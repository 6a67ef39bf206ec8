"""CPU-side checks of the crypto env's episode history (finenv_crypto_set_history): the header declares
the struct and the three entry points and the library exports them, ABI version and struct sizes are
unchanged, the entry points validate their arguments without a GPU, and the builders and readers of
finrl_amd.history reproduce, from the reference-recorded state of tests/golden/crypto_*.npz laid out as
the device holds it, the true account value and the list DRLAgent.DRL_prediction_load_from_file builds
(agents/stablebaselines3/models.py:146-156)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "finenv.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANDATORY = ("asset", "holdings", "start", "len", "flags")


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def _host_history(nat, E=64, N=5, cap=5, stocks=True):
    """A history struct over host arrays: enough for the argument checks, which never launch."""
    bufs = dict(asset=np.zeros((cap, E)), holdings=np.zeros((cap, E)),
                stocks=np.zeros((cap, N, E), np.float32), start=np.zeros(E, np.int32),
                len=np.zeros(E, np.int32), flags=np.zeros(E, np.int32))
    ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in bufs.items()}
    hist = nat.CryptoHistoryPtrs(ptr["asset"], ptr["holdings"], ptr["stocks"] if stocks else None,
                                 ptr["start"], ptr["len"], ptr["flags"], cap)
    return hist, bufs


def test_header_declares_and_library_exports_the_history_api(L):
    hdr = open(HDR).read()
    for fn in ("finenv_crypto_set_history", "finenv_crypto_history_arm", "finenv_crypto_history_metrics"):
        assert re.search(rf"\bint\s+{fn}\s*\(", hdr), fn
        assert hasattr(L, fn), fn
    m = re.search(r"typedef struct finenv_crypto_history \{(.*?)\} finenv_crypto_history;", hdr, flags=re.S)
    assert m, "struct finenv_crypto_history"
    fields = re.findall(r"^\s*(double|int32_t|float)\s+\*?(\w+);", m.group(1), flags=re.M)
    assert fields == [("double", "asset"), ("double", "holdings"), ("float", "stocks"),
                      ("int32_t", "start"), ("int32_t", "len"), ("int32_t", "flags"),
                      ("int32_t", "capacity")]
    pointers = re.findall(r"^\s*\w+\s+\*(\w+);", m.group(1), flags=re.M)
    assert pointers == [f[1] for f in fields[:-1]]          # every member but capacity is a pointer
    from finrl_amd import _native as nat
    assert [f[0] for f in nat.CryptoHistoryPtrs._fields_] == [f[1] for f in fields]
    assert [f[1] for f in nat.CryptoHistoryPtrs._fields_] == [C.c_void_p] * 6 + [C.c_int32]
    assert nat.CRYPTO_HISTORY_METRICS == nat.STOCK_HISTORY_METRICS == (
        "n_returns", "cumulative_return", "mean", "std", "sharpe", "max_drawdown")
    # additive: same ABI version, same v3 structs (the history structs are in no size table)
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
    assert L.finenv_crypto_set_history(None, C.byref(hist)) == -1
    assert L.finenv_crypto_history_arm(None, None, None) == -1
    assert L.finenv_crypto_history_metrics(None, 2.0, outp, None) == -1
    h = C.c_void_p()
    cfg = nat.CryptoConfig(64, 5, 4, 50, 1, 0, 1e6, 1e-3, 1e-3, 0.99)
    assert L.finenv_crypto_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # nothing attached (the default): arm / metrics refuse, with a message
        assert L.finenv_crypto_history_arm(h, None, None) == -1
        assert b"no history attached" in L.finenv_crypto_last_error(h)
        assert L.finenv_crypto_history_metrics(h, 2.0, outp, None) == -1
        assert b"no history attached" in L.finenv_crypto_last_error(h)
        # a NULL mandatory pointer, capacity < 2
        for name in MANDATORY:
            bad, _ = _host_history(nat)
            setattr(bad, name, None)
            assert L.finenv_crypto_set_history(h, C.byref(bad)) == -1, name
            assert b"null" in L.finenv_crypto_last_error(h)
        for cap in (1, 0, -3):
            bad, _ = _host_history(nat)
            bad.capacity = cap
            assert L.finenv_crypto_set_history(h, C.byref(bad)) == -1, cap
            assert b"capacity" in L.finenv_crypto_last_error(h)
        # a refused struct attaches nothing
        assert L.finenv_crypto_history_arm(h, None, None) == -1
        # attaching works before bind (stocks may be NULL); arm / metrics then need the bound state
        now, _ = _host_history(nat, stocks=False)
        assert L.finenv_crypto_set_history(h, C.byref(now)) == 0
        assert L.finenv_crypto_set_history(h, C.byref(hist)) == 0
        assert L.finenv_crypto_history_arm(h, None, None) == -2
        assert L.finenv_crypto_history_metrics(h, 2.0, outp, None) == -2
        assert L.finenv_crypto_history_metrics(h, 2.0, None, None) == -1
        # NULL detaches again
        assert L.finenv_crypto_set_history(h, None) == 0
        assert L.finenv_crypto_history_arm(h, None, None) == -1
        assert L.finenv_crypto_history_metrics(h, 2.0, outp, None) == -1
    finally:
        L.finenv_crypto_destroy(h)
    assert not any(b.any() for b in bufs.values()) and not out.any()


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
