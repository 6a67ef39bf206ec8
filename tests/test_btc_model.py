"""tests/btc_model.py equals the recorded runs of the reference BitcoinEnv (tests/golden/btc_*.npz,
written by tests/golden/make_golden_btc.py) on every recorded quantity -- observation, float64
reward, done, account, stocks and its scalar-type tag, total_asset, gamma_return, episode_return --
bit for bit.  The GPU tests then compare the kernel with this model where no recording exists."""
import numpy as np
import pytest

import btc_model as bm

FIXTURES = ("btc_basic", "btc_caps", "btc_wide", "btc_modes", "btc_midreset", "btc_draw", "btc_widths",
            "btc_domain")
CASES = [(f, c) for f in FIXTURES for c in bm.load_fixture(f)]


@pytest.mark.parametrize("fixture,case", CASES)
def test_model_equals_reference_recording(fixture, case):
    c = bm.load_fixture(fixture)[case]
    m = bm.BtcModel(c["price_ary"], c["tech_ary"], **bm.model_kwargs(c["kwargs"]))
    assert len(c["ops"]) >= 1
    for i, op in enumerate(c["ops"]):
        if op == bm.OP_RESET:
            obs, reward, done = m.reset(), None, None
        else:
            obs, reward, done = m.step(c["actions"][i])
        bm.check_against(c, i, obs, reward, done, m.record(), f"{fixture}/{case}")
    assert int(c["max_step"]) == c["price_ary"].shape[0]
    assert int(c["state_dim"]) == 2 + c["price_ary"].shape[1] + c["tech_ary"].shape[1]


def test_fixtures_reach_the_rules():
    """What the generator asserted when it ran, checked again on the files that are committed."""
    caps = bm.load_fixture("btc_caps")["caps"]
    tags = caps["tag"].tolist()
    assert [t for i, t in enumerate(tags) if i == 0 or t != tags[i - 1]] == [bm.PY, bm.F32, bm.F64]
    assert (caps["stocks"] < 0).any() and (caps["account"] < 0).any()      # short, and overdrawn
    basic = bm.load_fixture("btc_basic")["basic"]
    assert set(basic["tag"].tolist()) == {bm.PY, bm.F32} and (basic["ops"] == bm.OP_RESET).sum() == 2
    assert basic["done"].sum() == 2
    wide = bm.load_fixture("btc_wide")
    assert wide["p3w9"]["obs"].shape[1] == 12 and int(wide["p3w9"]["state_dim"]) == 14
    assert wide["p2w7"]["obs"].shape[1] == 11
    mid = bm.load_fixture("btc_midreset")["midreset"]
    k = int(np.flatnonzero(mid["ops"] == bm.OP_RESET)[1])
    assert mid["gamma_return"][k] == mid["gamma_return"][k - 1] != 0.0


@pytest.mark.parametrize("fixture", ["btc_widths", "btc_domain"])
def test_wide_and_domain_fixtures_reach_the_rules(fixture):
    """Over the whole fixture: every cap branch at least twice, all three tags, short and overdrawn
    states, nothing non-finite; btc_widths has the five widths, btc_domain every special action (by
    its bits) and both extremes of price level and account."""
    cases = bm.load_fixture(fixture)
    counts = [bm.fixture_branches(c) for c in cases.values()]
    assert min(sum(n[k] for n in counts) for k in counts[0]) >= 2, counts
    assert set(np.concatenate([c["tag"] for c in cases.values()]).tolist()) == {bm.PY, bm.F32, bm.F64}
    assert any((c["stocks"] < 0).any() for c in cases.values())
    assert any((c["account"] < 0).any() for c in cases.values())
    for c in cases.values():
        steps = c["ops"] == bm.OP_STEP
        assert c["ops"][0] == bm.OP_RESET and c["done"].sum() == 1 and c["done"][-1] == 1
        assert np.isfinite(c["obs"]).all() and np.isfinite(c["reward"][steps]).all()
        assert all(np.isfinite(c[k]).all() for k in bm.STATE_F64)
    if fixture == "btc_widths":
        assert [c["obs"].shape[1] for c in cases.values()] == [62, 63, 126, 127, 254]
        assert all(c["price_ary"].shape[0] == 8 for c in cases.values())
    else:
        assert len(cases) == 6 and all(c["price_ary"].shape == (40, 1) for c in cases.values())
        for c in cases.values():
            applied = set(bm.bits(c["actions"][c["ops"] == bm.OP_STEP]).tolist())
            assert set(bm.bits(bm.SPECIAL_ACTIONS).tolist()) <= applied
        level = sorted({round(float(np.log10(c["price_ary"][0, 0]))) for c in cases.values()})
        account = sorted({c["kwargs"]["initial_account"] for c in cases.values()})
        assert (level[0], level[-1]) == (-4, 8) and (account[0], account[-1]) == (1e2, 1e12)


def test_mode_rows_equal_load_data():
    modes = bm.load_fixture("btc_modes")
    for mode, c in modes.items():
        kw = c["kwargs"]
        assert kw["mode"] == mode
        rows = bm.mode_rows(c["raw_price"].shape[0], kw["time_frequency"], kw["start"], kw["mid1"],
                            kw["mid2"], kw["end"])[mode]
        assert np.array_equal(c["raw_price"][rows], c["price_ary"])
        assert np.array_equal(c["raw_tech"][rows], c["tech_ary"])
        assert len(rows) >= 7 and rows[1] - rows[0] == kw["time_frequency"]


def test_model_draw_equals_reference_recording():
    """The loop of draw_cumulative_return over the model, with the recorded run's stub actor."""
    c = bm.load_fixture("btc_draw")["draw"]
    m = bm.BtcModel(c["price_ary"], c["tech_ary"], **bm.model_kwargs(c["kwargs"]))
    agent = bm.StubAgent()
    state = m.reset()
    returns, btc = [1], []
    for i in range(c["price_ary"].shape[0]):
        btc.append(m.price[m.day, 0] / m.price[0, 0])
        a = agent.act(np.asarray((state,))).numpy()[0]
        state, _, done = m.step(a[0])
        returns.append(m.total_asset / 1e6)
        if done:
            break
    assert np.array_equal(np.asarray(returns, np.float64), c["episode_returns"])
    assert np.array_equal(np.asarray(btc, np.float64), c["btc_returns"])
    assert c["kwargs"]["initial_account"] != 1e6 and returns[1] < 0.9      # the hard-coded 1e6 shows
