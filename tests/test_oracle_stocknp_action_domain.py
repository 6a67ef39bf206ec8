"""The cases of tests/stocknp_action_cases.py through the CPU oracle alone, at every parametrisation that
tests/test_gpu_stocknp_action_domain.py uses: each case must reach the events it exists for, in a wave
on the all-float64 trade loops and in one on the tagged loops, so a seed that stops doing so fails here,
without a GPU.  What pins the oracle itself on this domain are the fixtures recorded from the unmodified
reference (tests/golden/stocknp_actdom_boundary / _ties / _beyond.npz, replayed by
tests/test_oracle_stocknp.py); this file checks that they hold what they were recorded for."""
import os

import numpy as np
import pytest

import stocknp_action_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAIN = [(c, N, ms, r, False) for c, ms, r in sc.CONFIGS for N in sc.NS]
WINDOWED = [(c, N, 128, 0.1, True) for c in sc.FORM_CASES for N in sc.FORM_NS]


def _id(p):
    return f"{p[0]}-N{p[1]}-ms{p[2]:g}-rate{p[3]:g}" + ("-windows" if p[4] else "")


def test_every_parametrisation_is_there():
    assert {c for c, _, _ in sc.CONFIGS} == set(sc.REQUIRE) == {"boundary", "ties", "beyond", "past", "quotient"}
    assert sc.NS == (1, 5, 30, 32) and len(PLAIN) == 44 and len(WINDOWED) == 6
    assert {ms for c, ms, _ in sc.CONFIGS if c == "boundary"} == {128, 100, 1e6}
    assert {ms for c, ms, _ in sc.CONFIGS if c == "beyond"} == {128, 1e6}
    assert {r for c, _, r in sc.CONFIGS if c == "boundary"} == {0.1, 0.0}
    assert all(sc.SEEDS[k] > 0 for k in sc.SEEDS) and set(sc.SEEDS) <= set(PLAIN + WINDOWED)
    assert float(np.float32(sc.S)) == sc.S == 2 ** 31 - 128


@pytest.mark.parametrize("param", PLAIN + WINDOWED, ids=_id)
def test_oracle_reaches_the_events_of_the_case(param):
    tr = sc.trace(*param)
    ev = sc.require_events(tr)
    case = tr.case
    price, _, turb = case.arrays
    assert price.min() < 3e-3 or case.N == 1
    assert price.max() > 3e4 or case.N == 1
    assert int((turb > 99).sum()) == int(case.name == "beyond")
    stocks0, amount0, tag0 = case.starts
    assert amount0.min() == 1e2 and amount0.max() == 1e12
    top = 22 if case.name == "ties" else 30
    assert stocks0.max() >= 2 ** top and stocks0.min() < 40 and (tag0[:sc.WAVE] == sc.TAG_F64).all()
    assert ev["steady_wave_steps"] == sc.STEPS and ev["mixed_wave_steps"] == sc.STEPS
    for st in tr.steps:
        assert np.isfinite(st["obs"]).all() and np.isfinite(st["rew"]).all()
        assert (st["state"]["amount_tag"][sc.IDLE] != sc.TAG_F64)           # env 70 never trades
    if case.sat:                                     # the env is fed what the oracle is not
        x = sc.product(tr.acts, case.max_stock)
        assert (np.abs(x) > sc.S).any() and (sc.product(tr.fed, case.max_stock) != x).any()
        assert np.abs(sc.product(tr.fed, case.max_stock)).max() == sc.S
    else:
        np.testing.assert_array_equal(tr.fed, tr.acts)


@pytest.mark.parametrize("seed_key", sorted(sc.SEEDS), ids=_id)
def test_recorded_seeds_are_the_first_that_reach_every_event(seed_key):
    saved = sc.SEEDS[seed_key]
    try:
        for seed in range(saved):
            sc.SEEDS[seed_key] = seed
            sc.trace.cache_clear()
            with pytest.raises(AssertionError):
                sc.require_events(sc.trace(*seed_key))
    finally:
        sc.SEEDS[seed_key] = saved
        sc.trace.cache_clear()


def test_saturated_actions_are_exact_and_keep_the_sign():
    a = np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 40, -2.0 ** 40, 3e38, -3e38, sc.S, -sc.S, 5.0, -0.3],
                 np.float32) / np.float32(128)
    want = [sc.S, -sc.S, sc.S, -sc.S, sc.S, -sc.S, sc.S, -sc.S, 5, 0]
    np.testing.assert_array_equal(sc.effective(a, 128), want)
    np.testing.assert_array_equal(sc.scaled(sc.saturated(a, 128), 128), want)
    with pytest.raises(AssertionError):
        sc.saturated(a, 100)


# ---------------------------------------------------------------- the reference's own records
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, f"stocknp_actdom_{name}.npz"), allow_pickle=False)
    assert any(m.startswith("numpy=2.") for m in z["meta"].tolist())     # recorded under NEP 50 promotion
    assert os.path.getsize(os.path.join(GOLDEN, f"stocknp_actdom_{name}.npz")) < 64 * 1024
    T, N, K, S, if_train = z["cfg_int"].tolist()
    assert (T, N, K, S, if_train) == (sc.FIX_T, sc.FIX_N, sc.K, sc.FIX_STEPS, 0)
    assert z["cfg_float"][1] == sc.FIX_MAX_STOCK
    return z


def _before(z, key, s):
    """The env's `key` before step s: the reset value behind an episode end, else the step before."""
    r = z["reset_step"].tolist()
    if s - 1 in r:
        return z["reset_" + key + "0"][r.index(s - 1)]
    return z[key][s - 1]


def test_boundary_fixture_holds_every_value_and_both_strict_compares():
    z = _fixture("boundary")
    vals = sc.boundary_values(sc.FIX_MAX_STOCK, 0.1)
    assert np.isin(vals.view(np.uint32), z["actions"].view(np.uint32)).all()
    m = sc.min_action_of(sc.FIX_MAX_STOCK, 0.1)
    a = sc.scaled(z["actions"], sc.FIX_MAX_STOCK)
    seen = dict(plus=0, minus=0, over=0, under=0)
    for s in range(len(a)):
        held = _before(z, "stocks", s) > 0
        traded = z["cool_down"][s] == 0
        np.testing.assert_array_equal(traded, (a[s] > m) | (a[s] < -m))     # (no turbulent day, prices > 0)
        seen["plus"] += int((a[s] == m).sum())
        seen["minus"] += int(((a[s] == -m) & held).sum())
        seen["over"] += int((a[s] == m + 1).sum())
        seen["under"] += int(((a[s] == -m - 1) & held).sum())
    assert min(seen.values()) > 0, seen


def test_ties_fixture_holds_both_ties_and_the_float32_tag():
    z = _fixture("ties")
    a = sc.scaled(z["actions"], sc.FIX_MAX_STOCK)
    price = z["price_array"].astype(np.float32)
    sell = buy = kept32 = 0
    for s in range(len(a)):
        s0, am0 = _before(z, "stocks", s), _before(z, "amount", s)
        r = z["reset_step"].tolist()
        tag0 = int(z["reset_amount0_tag"][r.index(s - 1)] if s - 1 in r else z["amount_tag"][s - 1])
        tie = (a[s] < -12) & (-a[s] == s0)
        if tie.any() and not ((a[s] != 0) & ~tie).any():
            sell += int(tie.sum())
            assert (z["stocks"][s][tie] == 0).all()
            assert z["amount_tag"][s] == (sc.TAG_F32 if tag0 == sc.TAG_PY else tag0)
            kept32 += int(tag0 != sc.TAG_F64)
        j = np.flatnonzero(a[s] != 0)
        if len(j) == 1 and a[s][j[0]] == sc.floordiv_as_numpy(am0, tag0, price[z["day"][s]][j[0]]):
            buy += 1
            assert z["stocks"][s][j[0]] == np.float32(np.float64(s0[j[0]]) + a[s][j[0]])
    assert sell > 0 and buy > 0 and kept32 > 0, (sell, buy, kept32)


def test_beyond_fixture_holds_every_magnitude_and_the_int64_step():
    z = _fixture("beyond")
    a = sc.scaled(z["actions"], sc.FIX_MAX_STOCK)
    for v in sc.signed_beyond():
        assert (a == v).any(), v
    assert int((z["turbulence_array"] > 99).sum()) == 1
    # step 1: -2^40 on ticker 0, +2^40 on ticker 1 -- all the holdings go, the cash buys what it can:
    # min(stocks, 2^40) and min(amount // price, 2^40), neither wrapped to an int32 (which would be 0 here)
    assert a[1, :2].tolist() == [-(1 << 40), 1 << 40]
    assert z["stocks"][0][0] >= 2 ** 30 and z["stocks"][1][0] == 0
    bought = np.float64(z["stocks"][1][1]) - np.float64(z["stocks"][0][1])
    assert 2 ** 20 < bought < sc.S and (z["cool_down"][1][:2] == 0).all()
    assert abs(z["amount"][1]) < 1e-2 * z["amount"][0]                      # it spent the cash
