"""The cases of tests/twowave_domain_cases.py through the CPU oracles alone, at every shape the GPU files
(tests/test_gpu_{cashpenalty,stoploss}_panel_domain.py) use: each case must reach the events it exists
for, so a seed that stops doing so fails here, without a GPU.  And what pins the oracles themselves
on these panels: the NumPy expression of the reference's discretisation on the tick-price closes, and the
five fixtures recorded from the unmodified reference (stoploss_zerocloses / _ties / _ticks, cashpenalty_ticks /
_pricescales; the glob-based fixture tests replay them)."""
import os

import numpy as np
import pytest

import twowave_domain_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = [(kind,) + c for kind in tc.KINDS for c in tc.cases(kind)]
WINDOWED = [(kind,) + c for kind in tc.KINDS for c in tc.window_cases(kind)]


def _ids(cases):
    return [f"{c[0]}-{tc.case_id(*c[1:])}" for c in cases]


def test_every_launch_form_and_builder_is_there():
    for kind in tc.KINDS:
        have = {(name, shape) for name, shape, _ in tc.cases(kind)}
        for name in tc.BUILDERS:
            if name == "zero_closes" and kind == "cashpenalty":
                assert not any(n == name for n, _ in have)       # close > 0 is that env's domain
                continue
            assert {(name, s) for s in tc.SHAPES} <= have, (kind, name)
        assert {n for n, _, _ in tc.window_cases(kind)} == {n for n, _ in have}
    assert 60 <= len(ALL) + len(WINDOWED) <= 90


@pytest.mark.parametrize("kind,name,shape,args", ALL, ids=_ids(ALL))
def test_oracle_reaches_the_events_of_the_case(kind, name, shape, args):
    case, starts0, obs0, steps = tc.trace(kind, name, shape, args)
    assert case.close.shape == (tc.T, shape[0]) and case.info.shape == (tc.T,) + tuple(shape)
    if kind == "cashpenalty":
        assert case.close.min() > 0
    tc.require_events(kind, case, tc.events(kind, case, steps))
    assert sum(bool(st["done"].any()) for st in steps) >= 2
    for st in steps:
        assert np.isfinite(st["obs"]).all() and np.isfinite(st["rew"]).all()


@pytest.mark.parametrize("kind,name,shape,args", WINDOWED, ids=_ids(WINDOWED))
def test_windowed_twins_reach_the_events_of_the_case(kind, name, shape, args):
    case, steps, end = tc.window_trace(kind, name, shape, args)
    tc.require_events(kind, case, tc.events(kind, case, steps, end))


TICKS = [c for c in ALL if c[1] == "tick_prices"]


@pytest.mark.parametrize("kind,name,shape,args", TICKS, ids=_ids(TICKS))
def test_first_step_transactions_are_the_numpy_expression(kind, name, shape, args):
    """Discrete transactions of the first step of an episode (no holdings: no sell fills, every buy is
    unclipped) are what :335-343 of the stop-loss reference (:263-274 of the cash-penalty one) give in
    NumPy -- `//` on float64, astype(int), `//` on integers -- and not what floor(a / close) gives."""
    case, _, _, steps = tc.trace(kind, name, shape, args)
    inc, hmax = case.kw["shares_increment"], case.kw["hmax"]
    checked = differ = 0
    for st in steps:
        pre, post = st["pre"], st["post"]
        m = (pre["date_index"] == pre["start"]) & ~st["done"]
        assert (pre["holdings"][m] == 0).all()
        closings = np.array(case.close[pre["date_index"][m]], np.float64)
        actions = st["a"][m] * hmax                                      # float32, :321
        assert actions.dtype == np.float32
        actions = np.where(closings > 0, actions, 0)
        actions = np.where(closings > 0, actions // closings, 0)
        actions = actions.astype(int)
        actions = np.where(actions >= 0, (actions // inc) * inc, ((actions + inc) // inc) * inc)
        want = np.maximum(actions, 0)
        got = post["holdings"][m]
        if case.kw["patient"]:                                           # a cancelled step buys nothing
            kept = (got != 0).any(1) | (want == 0).all(1)
            want, got, closings, raw = want[kept], got[kept], closings[kept], st["a"][m][kept]
        else:
            raw = st["a"][m]
        np.testing.assert_array_equal(got, want)
        floor = np.floor((raw * np.float32(hmax)).astype(np.float64) / closings)
        floor = np.maximum(np.where(floor >= 0, floor // inc * inc, (floor + inc) // inc * inc), 0)
        checked += want.size
        differ += int((floor != want).sum())
    assert checked >= tc.E * shape[0] and differ > 0, (checked, differ)      # (every env starts at least once)


def test_reference_keeps_zero_closes_finite_in_the_stop_loss_env():
    """stoploss_zerocloses.npz, recorded from the unmodified reference on a panel with zero closes (row 0
    included): it neither raises nor yields NaN; nothing is bought or sold by request at such a close, and
    a held asset whose close is 0 is sold for nothing by the stop-loss of an armed env."""
    z = np.load(os.path.join(GOLDEN, "stoploss_zerocloses.npz"), allow_pickle=False)
    assert (z["close"] == 0).any() and z["close"][0, 0] == 0
    for k in ("obs", "reward", "coh", "holdings", "avg_buy_price", "closing_diff_avg_buy"):
        assert np.isfinite(z[k]).all(), k
    h, di, done, close = z["holdings"], z["date_index"], z["done"], z["close"]
    slp, init = z["cfg_float"][6], z["cfg_float"][3]
    kept = given = asked = 0
    for s in range(1, len(h)):
        if done[s] or done[s - 1]:
            continue
        zero = close[di[s - 1]] == 0
        armed = z["coh"][s - 1] >= slp * init
        held = h[s - 1] > 0
        asked += int((zero & (z["actions"][s] != 0)).sum())
        if armed:
            assert (h[s][zero & held] == 0).all()
            given += int((zero & held).sum())
        else:
            np.testing.assert_array_equal(h[s][zero], h[s - 1][zero])
            kept += int((zero & held).sum())
    assert asked > 0 and kept + given > 0, (asked, kept, given)


def test_ties_fixture_holds_both_scripted_ties():
    """stoploss_ties.npz: a forced sale at cash == stoploss_penalty * initial_amount (`>=`, :353) and a
    step that spends the cash exactly and goes on (`>`, :372)."""
    z = np.load(os.path.join(GOLDEN, "stoploss_ties.npz"), allow_pickle=False)
    coh, h, di, done = z["coh"], z["holdings"], z["date_index"], z["done"]
    slp, init, thr = z["cfg_float"][6], z["cfg_float"][3], z["cfg_float"][5]
    armed = short = 0
    for s in range(1, len(coh)):
        if done[s]:
            continue
        if (not done[s - 1] and coh[s - 1] == slp * init and h[s - 1].sum() > 0 and h[s].sum() == 0
                and z["turb"][di[s - 1]] < thr and (z["actions"][s] == 0).all()):
            armed += 1
        short += int(coh[s] == 0.0 and h[s].sum() > 0)
    assert armed > 0 and short > 0, (armed, short)
