"""CPU only, oracles only: the scenarios of tests/twowave_windows_cases.py, which the GPU window tests of
the cash-penalty and stop-loss envs replay, reach every path those tests rely on -- so no GPU test can
pass by never getting there."""
import numpy as np
import pytest

from twowave_windows_cases import KINDS, SCENARIOS, SCENARIO_IDS, Script, Twins, make_panel


def run_twins(kind, sc):
    close, info, turb = make_panel(sc["N"], sc["C"])
    script = Script(sc)
    tw = Twins(kind, sc, close, info, turb, script.start, script.end)
    tw.reset(script.offsets0)
    pending_differs_at_reset = 0
    for s in range(sc["steps"]):
        a, off, redraw = script.step(s)
        if redraw is not None:
            tw.set_pending(*redraw)
        differs = (tw.pending != tw.active).any(axis=0)
        _, _, done, _ = tw.step(a, off, sc["auto"])
        if not sc["auto"] and done.any():
            tw.reset(off, done)
        pending_differs_at_reset += int((differs & done).sum())
    return tw, pending_differs_at_reset


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sc", SCENARIOS, ids=SCENARIO_IDS)
def test_scenario_reaches_every_path(kind, sc):
    tw, pending_differs_at_reset = run_twins(kind, sc)
    assert tw.episodes_done.min() >= 2, "every env finishes at least 2 episodes"
    if not sc["patient"]:
        assert tw.n_cash_end_inside >= 1, "a cash shortage strictly inside a window"
    assert tw.n_last_date_end >= 1, "an episode ends at its window's last date"
    assert pending_differs_at_reset >= 1 and tw.n_reset_on_new_window >= 1, \
        "a reset while pending != active"
    assert tw.one_row_episodes >= 1, "an env on a one-row window"
    if kind == "stoploss":
        assert tw.n_forced_sales >= 1, "a forced stop-loss sale"


def test_broke_scenario_overflows_the_register_fixups():
    """d181-broke: in some step more envs of one 64-env block end on a cash shortage (their decided row
    differs from the streamer's speculation) than the kFix = 4 rows the streamer patches in registers."""
    sc = next(s for s in SCENARIOS if s["name"] == "d181-broke")
    close, info, turb = make_panel(sc["N"], sc["C"])
    script = Script(sc)
    tw = Twins("cashpenalty", sc, close, info, turb, script.start, script.end)
    tw.reset(script.offsets0)
    most = 0
    for s in range(sc["steps"]):
        a, off, redraw = script.step(s)
        if redraw is not None:
            tw.set_pending(*redraw)
        before = tw.n_cash_end_inside
        inside = np.array([o.state()["date_index"][0] for o in tw.orc]) + tw.active[0] < tw.active[1] - 1
        _, _, done, _ = tw.step(a, off, True)
        broke = done & inside
        assert tw.n_cash_end_inside - before == int(broke.sum())
        most = max(most, max(int(broke[b:b + 64].sum()) for b in range(0, sc["E"], 64)))
    assert most > 4
