"""oracle/portfolio_oracle.c vs the unmodified reference StockPortfolioEnv on the action and panel domain
(tests/golden/portfolio_domain.npz, made by `tests/golden/make_golden.py portfolio:domain` from
tests/portfolio_domain_cases.py): every action kind in rotation -- negative scores, exponentials that
overflow, sums that overflow, subnormal and zero exponentials, -inf -- on a panel with zero closes, a
flat day and x1e6 jumps.

Exact: done, day, observations, reset observations; the NaN / inf / zero positions of weights and value;
the weights wherever they are 0 or NaN by overflow or underflow.  Finite weights and values: the derived
bounds of portfolio_domain_cases (no tolerance is measured here)."""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import portfolio_domain_cases as pc  # noqa: E402


def load():
    return np.load(os.path.join(HERE, "golden", "portfolio_domain.npz"), allow_pickle=False)


def test_fixture_holds_what_its_builders_say():
    """The committed arrays are what the builders give today, every kind is there, and the events the
    panel exists for meet a finite value in the reference's own run."""
    z = load()
    T, N, K, S = z["cfg_int"].tolist()
    act, kinds = pc.fixture_actions(S, N, T, 37)
    np.testing.assert_array_equal(act.view(np.uint32), z["actions"].view(np.uint32))
    assert kinds == z["kinds"].tolist() and set(kinds) == set(pc.KINDS)
    variant = str(z["panel_variant"])
    roles = pc.panel_roles(T, N, variant)
    base = z["close"].copy()
    assert (base == 0).sum() == 5 and (base[0] > 0).all() and base[roles.zero_day, roles.zero] == 0
    for s, k in enumerate(kinds):
        pc.check_rows(k, z["actions"][s][None])
    v0 = pc.fixture_values_before(z)
    trace = [dict(done=z["done"][s:s + 1], value0=v0[s:s + 1], day0=z["day"][s:s + 1] - (not z["done"][s]),
                  weights=z["weights"][s][None], rew=z["reward"][s:s + 1]) for s in range(S)]
    ev = pc.panel_events(pc.gross_returns(z["close"]), trace)
    pc.require_panel_events(variant, ev)
    assert pc.finite_share(trace) >= 0.5
    # what the action kinds make of a finite value, in the reference's own outputs
    seen = collections.Counter()
    for s, k in enumerate(kinds):
        if z["done"][s] or not np.isfinite(v0[s]):
            continue
        w, v = z["weights"][s], z["value"][s]
        if k == "sum_overflow":
            assert (w == 0).all() and v == v0[s]
        if k in pc.POISONING:
            assert np.isnan(w).any() and np.isnan(v)
        if k in ("subnormal", "sub_mixed"):
            assert np.isfinite(w).all() and abs(float(w.sum()) - 1) < 0.2
        seen[k] += 1
    assert seen["sum_overflow"] and seen["all_underflow"] and seen["subnormal"] and seen["sub_mixed"], seen


def test_portfolio_oracle_matches_reference_on_the_domain():
    from oracle.portfolio import PortfolioOracle
    z = load()
    T, N, K, S = z["cfg_int"].tolist()
    o = PortfolioOracle(z["close"], z["cov"], z["tech"], n_envs=1, initial_amount=z["cfg_float"][0])
    resets = dict(zip(z["reset_step"].tolist(), z["reset_obs"]))
    np.testing.assert_array_equal(o.reset()[0], resets[-1])
    n_done = n_bounded = 0
    for s in range(S):
        v0 = o.state()["value"][0]
        obs, rew, done, _, w = o.vec_step_weights(z["actions"][s], auto_reset=False)
        st = o.state()
        assert done[0] == z["done"][s] and st["day"][0] == z["day"][s], s
        np.testing.assert_array_equal(obs[0], z["obs"][s], err_msg=f"obs step {s}")
        pc.same_class(rew, z["reward"][s:s + 1], f"reward step {s}")
        if done[0]:
            pc.same_class(st["value"], z["value"][s:s + 1], f"value step {s}")
            n_done += 1
            np.testing.assert_array_equal(o.reset()[0], resets[s])
            assert o.state()["value"][0] == z["cfg_float"][0]
            continue
        assert np.array_equal(rew, st["value"], equal_nan=True)
        n_bounded += pc.check_fixture_step(z, s, w[0], v0, st["value"][0], "oracle")
    assert n_done == 3 and n_bounded >= 20, (n_done, n_bounded)
