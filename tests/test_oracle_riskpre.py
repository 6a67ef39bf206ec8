"""oracle/riskpre.py vs committed outputs of the unmodified reference
FeatureEngineer.calculate_turbulence (preprocessors.py:215-267) and the tutorial's cov_list lines
(tests/golden/riskpre_*.npz).  Float work: rtol 1e-9 on the turbulence index (the quadratic form
goes through an SVD-based pseudo-inverse), 1e-12 of the covariance scale on cov."""
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[len("riskpre_"):-4]
               for p in glob.glob(os.path.join(GOLDEN, "riskpre_*.npz")))


def test_fixtures_present():
    assert len(NAMES) >= 3


@pytest.mark.parametrize("name", NAMES)
def test_turbulence_oracle_matches_reference(name):
    from oracle import riskpre
    z = np.load(os.path.join(GOLDEN, f"riskpre_{name}.npz"), allow_pickle=False)
    got = riskpre.calculate_turbulence(z["close"])
    ref = z["turbulence"]
    np.testing.assert_array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=1e-9)
    assert (ref[:252] == 0).all() and (ref > 0).sum() >= 5


@pytest.mark.parametrize("name", NAMES)
def test_rolling_covariance_oracle_matches_reference(name):
    from oracle import riskpre
    z = np.load(os.path.join(GOLDEN, f"riskpre_{name}.npz"), allow_pickle=False)
    cov = riskpre.rolling_covariance(z["close"], int(z["lookback"]))
    scale = np.abs(z["cov"]).max()
    np.testing.assert_allclose(cov[z["cov_index"]], z["cov"], rtol=0, atol=1e-12 * scale)


def test_short_panel_raises():
    from oracle import riskpre
    with pytest.raises(ValueError):
        riskpre.calculate_turbulence(np.ones((100, 3)))


def test_oracle_single_ticker_is_x2_over_var():
    """N = 1: pinv of the 1 x 1 covariance is 1 / var (np.atleast_2d keeps pinv on a matrix)."""
    from oracle import riskpre
    c = 40 * np.exp(np.cumsum(np.random.default_rng(3).normal(0, 0.01, (80, 1)), axis=0))
    q = riskpre.turbulence_quadratic_forms(c, 20)
    r = riskpre.pct_change(c)[:, 0]
    for d in (20, 21, 79):
        h = r[max(d - 20, 1):d]
        np.testing.assert_allclose(q[d], (r[d] - h.mean()) ** 2 / h.var(ddof=1), rtol=1e-13)
    assert riskpre.rolling_covariance(c, 20).shape == (60, 1, 1)


# ------------------------------------------------- oracle/riskpre_exact.py certified by mpmath
def _exact_cases():
    from oracle import riskpre_exact as rx
    p = rx.panel
    return {
        "wellcond_n33": (p(11, 80, 33), 64),
        "lowvol_n8_1e-5": (rx.low_vol(p(12, 80, 8), 7, 1e-5), 62),
        "degenerate_n12": (rx.halted(rx.constant(rx.duplicate(p(13, 150, 12), 0, 11), 2),
                                     3, 5, 90), 63),
        "dup_lowvol_n65": (rx.low_vol(rx.duplicate(p(14, 254, 65), 10, 40), 64, 1e-5), 252),
        "parting_n8": (rx.parting(p(17, 80, 8), 1, 6, 64), 63),
    }


@pytest.mark.parametrize("case", ["wellcond_n33", "lowvol_n8_1e-5", "degenerate_n12",
                                  "dup_lowvol_n65", "parting_n8"])
def test_exact_reference_certified_by_mpmath(case):
    """The longdouble quadratic forms agree with 40-digit mpmath within their own reported bound,
    and that bound is far below the GPU tests' tightest tolerance (1e-11)."""
    from oracle import riskpre_exact as rx
    close, W = _exact_cases()[case]
    ex = rx.quadratic_forms_exact(close, W)
    assert ex.bound.max() < 1e-12
    T = close.shape[0]
    days = sorted({W, W + 1, T - 1} if close.shape[1] < 50 else {W + 1})
    for d in days:
        k = d - W
        qm = rx.mp_quadratic_form(close, W, d)
        err = abs(float(qm - rx.mpmath_value(ex.q[k])))
        assert err <= ex.bound[k] * float(qm), (d, err / float(qm), ex.bound[k])
    if case == "degenerate_n12":
        assert set(ex.rank.tolist()) == {10, 9}       # duplicate + constant, + halted on some days
    if case.startswith("lowvol"):
        assert (ex.pivot_ratio < rx.PIVOT_SWITCH).all() and (ex.eig_ratio >= rx.EIG_MARGIN).all()


@pytest.mark.parametrize("case", ["degenerate_n12", "parting_n8"])
def test_exact_reduction_is_numpy_pinv(case):
    """On days singular by construction the reduced full-rank problem is what np.linalg.pinv
    computes: zero columns dropped, duplicates merged (x averaged over the pair on the day the
    pair parts)."""
    from oracle import riskpre
    from oracle import riskpre_exact as rx
    close, W = _exact_cases()[case]
    ex = rx.quadratic_forms_exact(close, W)
    assert (ex.rank < close.shape[1]).any()
    np.testing.assert_allclose(riskpre.turbulence_quadratic_forms(close, W)[W:], ex.q64,
                               rtol=1e-11)


def test_exact_reference_refuses_ill_posed_days():
    """A scale of 1e-7 puts an eigenvalue within 1000x of pinv's cutoff: not a test day."""
    from oracle import riskpre_exact as rx
    close = rx.low_vol(rx.panel(15, 80, 8), 7, 1e-7)
    with pytest.raises(AssertionError, match="pinv cutoff"):
        rx.quadratic_forms_exact(close, 62)


def test_exact_covariance_certified_by_mpmath():
    import mpmath
    from oracle import riskpre_exact as rx
    close = rx.panel(16, 30, 5, level=1e5)
    cov, budget = rx.covariance_exact(close, 20)
    r = rx.returns(close)
    with mpmath.workdps(40):
        for i in (20, 29):
            rows = [[mpmath.mpf(v) for v in r[t]] for t in range(i - 19, i + 1)]
            m = [mpmath.fsum(row[j] for row in rows) / 20 for j in range(5)]
            for a in range(5):
                for b in range(5):
                    c = mpmath.fsum((row[a] - m[a]) * (row[b] - m[b]) for row in rows) / 19
                    err = abs(float(c - rx.mpmath_value(cov[i - 20, a, b])))
                    assert err <= 1e-17 * budget[i - 20, a, b]
