"""HIP risk precompute (finenv_riskpre.hip) at the shapes, scalings and degeneracies where its
paths differ, against the extended-precision reference oracle/riskpre_exact.py (and
oracle.riskpre, NumPy pinv, to show the reference semantics are well-posed on every day tested).

Paths of rolling_risk_kernel<true> and who reaches them:
  Cholesky fast path (every pivot > 1e-6 x max diag)       test_cholesky_well_conditioned
  Jacobi fallback, even and odd N (odd N: dummy player)    test_jacobi_degenerate,
                                                           test_jacobi_duplicates_part,
                                                           test_jacobi_low_volatility,
                                                           test_jacobi_converges_at_n128
  either side of the 1e-6 switch                           test_switch_sides
  > 64 KiB dynamic LDS opt-in (N >= 91; 135,184 B at 128)  every N in {127, 128} case
  turbulence_filter_kernel's carry across 64-day chunks    test_filter_chunk_carry
  returns_kernel's grid-stride loop (> 4096 blocks)        test_returns_past_one_grid
  rolling_risk_kernel<false> (cov_list)                    test_rolling_covariance

Bounds on the quadratic form q = x' pinv(C) x, relative to the exact value (the reference's own
error bound, a worst-case one, is asserted to be at least 2x below each of them):
  well-conditioned Cholesky days (min pivot ratio >= 1e-2)                 RT_CHOL  1e-11
  full-rank days with a smaller pivot ratio (near the switch, low-vol)     RT_ILL   1e-8
  days singular by construction (duplicate / constant / halted columns)    RT_DEGEN 1e-9
  (a duplicate pair's entries of x are replaced by their mean: x's projection on C's range)
  days whose every column is constant in the window: q == 0 exactly.
Each test prints its maximum relative error per class."""
import numpy as np
import pytest

from oracle import riskpre as orc
from oracle import riskpre_exact as rx

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RT_CHOL, RT_ILL, RT_DEGEN = 1e-11, 1e-8, 1e-9
NS = [1, 2, 3, 31, 33, 63, 64, 65, 127, 128]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _turbulence(close, window):
    from finrl_amd import riskpre
    turb, quad = riskpre.calculate_turbulence(close, window=window, return_quadratic_forms=True)
    return turb.cpu().numpy(), quad.cpu().numpy()


def _check(label, close, window, expect=None):
    """GPU quadratic forms vs the exact reference (and NumPy pinv vs the same), filtered index vs
    the first-two-positive rule.  expect: 'cholesky' / 'jacobi' asserts the path every day takes
    (by the exact min pivot ratio); returns the exact-reference result."""
    _need_gpu()
    turb, quad = _turbulence(close, window)
    T, N = close.shape
    assert not np.isnan(quad).any() and not np.isnan(turb).any()
    np.testing.assert_array_equal(quad[:window], 0.0)
    np.testing.assert_array_equal(turb[:window], 0.0)
    ex = rx.quadratic_forms_exact(close, window)
    g, e = quad[window:], ex.q64
    npy = orc.turbulence_quadratic_forms(close, window)[window:]
    zero = ex.rank == 0
    degen = (ex.rank < N) & ~zero
    chol = (ex.rank == N) & (ex.pivot_ratio >= 1e-2)
    ill = (ex.rank == N) & ~chol
    if expect == "cholesky":
        assert chol.all(), f"{label}: min pivot ratio {ex.pivot_ratio.min():.1e} < 1e-2"
    elif expect == "jacobi":
        assert (ex.pivot_ratio < rx.PIVOT_SWITCH).all(), \
            f"{label}: a day takes the Cholesky path (pivot ratio {ex.pivot_ratio.max():.1e})"
    np.testing.assert_array_equal(g[zero], 0.0)
    np.testing.assert_array_equal(npy[zero], 0.0)
    msg = [label]
    for name, mask, rt in (("chol", chol, RT_CHOL), ("ill", ill, RT_ILL),
                           ("degen", degen, RT_DEGEN)):
        if not mask.any():
            continue
        assert ex.bound[mask].max() < rt / 2, f"{label}: reference bound {ex.bound.max():.1e}"
        rel = np.abs(g[mask] - e[mask]) / e[mask]
        rel_np = np.abs(npy[mask] - e[mask]) / e[mask]
        msg.append(f"{name}[{int(mask.sum())}d] gpu {rel.max():.1e} numpy {rel_np.max():.1e}")
        assert rel_np.max() <= rt, f"{label} {name}: NumPy pinv off by {rel_np.max():.1e}"
        worst = int(np.argmax(rel))
        assert rel.max() <= rt, (f"{label} {name}: GPU off by {rel.max():.2e} > {rt:.0e} on day "
                                 f"{window + np.flatnonzero(mask)[worst]}")
    if zero.any():
        msg.append(f"zero[{int(zero.sum())}d] exact")
    print(" | ".join(msg))
    # :247-257 on the GPU's own quadratic forms, exactly, and the same zero pattern as NumPy's
    np.testing.assert_array_equal(turb, orc.suppress_first_two(quad, window))
    np.testing.assert_array_equal(turb == 0, orc.calculate_turbulence(close, window) == 0)
    return ex


def _window_for(N):
    """A window with comfortably more return rows than assets (a well-posed full-rank day);
    the 62-64 windows straddle the filter's chunk boundary."""
    return {1: 3, 2: 62, 3: 63, 31: 64, 33: 252}.get(N, 252)


# ------------------------------------------------------------------------------------ Cholesky
@pytest.mark.parametrize("N", NS)
def test_cholesky_well_conditioned(N):
    W = _window_for(N)
    close = rx.panel(100 + N, W + 30, N)
    _check(f"chol N={N} W={W}", close, W, expect="cholesky")


# -------------------------------------------------------------------------------------- Jacobi
def _degenerate_panel(N, W, seed):
    """Duplicates, a constant ticker and a ticker halted for longer than the window (so some days
    see an all-zero column, then the resumption inside the window), as fits N."""
    T = W + 40
    c = rx.panel(seed, T, N)
    if N == 2:
        return rx.duplicate(c, 0, 1)
    if N == 3:
        return rx.constant(rx.duplicate(c, 0, 2), 1)
    c = rx.duplicate(c, 0, N - 1)
    c = rx.duplicate(c, 1, N // 2)
    c = rx.constant(c, 2)
    return rx.halted(c, 3, 5, W + 20)


@pytest.mark.parametrize("N", NS[1:])
def test_jacobi_degenerate(N):
    """Singular by construction at every even and odd N (odd N pairs a dummy player)."""
    W = {2: 3, 3: 62}.get(N, 252 if N > 31 else 64)
    close = _degenerate_panel(N, W, 200 + N)
    ex = _check(f"degen N={N} W={W}", close, W, expect="jacobi")
    assert (ex.rank < N).all()


@pytest.mark.parametrize("N", NS[1:])
def test_jacobi_duplicates_part(N):
    """Duplicated tickers that part ways: on the first day a pair differs, the window's two
    columns are still identical while x is not, so x has a component in the exact null direction
    that pinv drops (the answer uses the pair's mean); the days after are full rank.  A fast path
    that let an exact duplicate through on a rounding-noise pivot would divide that component by
    sqrt(noise) here."""
    W = {2: 3, 3: 62}.get(N, 252 if N > 31 else 64)
    close = rx.panel(250 + N, W + 14, N)
    for i, day in enumerate((W + 3, W + 6, W + 9)[:1 if N < 8 else 3]):
        close = rx.parting(close, i, N - 1 - i, day, seed=N + i)
    ex = _check(f"parting N={N} W={W}", close, W)
    assert (ex.rank[:3] < N).all() and (ex.rank[-3:] == N).all()


@pytest.mark.parametrize("N", [1, 2, 65])
def test_constant_panel(N):
    """Every ticker constant: C == 0, q == 0 exactly on every day (pinv(0) == 0), no NaN."""
    close = np.full((80, N), 12.5)
    ex = _check(f"const N={N}", close, 63)
    assert (ex.rank == 0).all()


@pytest.mark.parametrize("N,scale", [(2, 1e-5), (3, 1e-3), (31, 1e-4), (33, 1e-5), (63, 1e-3),
                                     (64, 1e-5), (65, 1e-4), (127, 1e-4), (128, 1e-4)])
def test_jacobi_low_volatility(N, scale):
    """A full-rank but badly scaled matrix: one asset's returns scaled by `scale` sends every day
    to the Jacobi path (pivot ratio ~ scale^2 x 0.5); pinv is its inverse there.  (At N >= 127 a
    scale of 1e-5 would put the smallest eigenvalue within 1000x of pinv's cutoff.)"""
    W = 252 if N > 3 else 63
    close = rx.low_vol(rx.panel(300 + N, W + 30, N), N - 1, scale)
    ex = _check(f"lowvol N={N} s={scale:.0e}", close, W, expect="jacobi")
    assert (ex.rank == N).all()


@pytest.mark.parametrize("N", [8, 65])
@pytest.mark.parametrize("target", [3e-6, 3e-7])
def test_switch_sides(N, target):
    """A low-volatility asset scaled so that the median day's min pivot ratio is `target`: 3e-6
    stays on the Cholesky path, 3e-7 goes to Jacobi; both meet the same bound (RT_ILL)."""
    W = 252 if N > 8 else 63
    base = rx.panel(400 + N, W + 30, N)
    r1 = np.median(rx.quadratic_forms_exact(base, W).pivot_ratio)
    # the last column's pivot scales with scale^2; the others and max diag do not
    close = rx.low_vol(base, N - 1, np.sqrt(target / r1))
    ex = _check(f"switch N={N} target={target:.0e}", close, W)
    side = ex.pivot_ratio > rx.PIVOT_SWITCH
    assert side.all() if target > rx.PIVOT_SWITCH else not side.any()


def test_jacobi_converges_at_n128():
    """N = 128 (the 132 KiB LDS launch) with a duplicate and a low-volatility asset over 32
    consecutive days: the 40-sweep cap is not what ends these diagonalisations."""
    W = 252
    c = rx.panel(500, W + 32, 128)
    c = rx.duplicate(c, 10, 77)
    close = rx.low_vol(c, 127, 1e-4)
    ex = _check("converge N=128", close, W, expect="jacobi")
    assert len(ex.days) >= 30 and (ex.rank == 127).all()


# ------------------------------------------------------------------------------- filter / shapes
@pytest.mark.parametrize("W", [3, 62, 63, 64, 252])
def test_filter_chunk_carry(W):
    """The first three positive days at window, window+1, window+2 sit on either side of the
    64-day chunk boundary for W = 62, 63; a panel that only starts moving on day 126 puts them
    across the next boundary (128) for every W < 128."""
    n = 5 if W > 3 else 1
    _check(f"filter N={n} W={W}", rx.panel(600 + W, W + 70, n), W)
    late = np.full((max(W, 126) + 70, 2), [20.0, 40.0])
    late[126:] = rx.panel(700 + W, late.shape[0] - 126, 1) * [1.0, 2.0]   # N = 2, duplicated
    ex = _check(f"filter-late N=2 W={W}", late, W)
    first = W + np.flatnonzero(ex.q64 > 0)[:3]
    assert first[0] <= 127 < first[2] or W > 128


def test_t_equals_window():
    """T == window: nothing to compute (all zeros, no rolling launch); T == window + 1: one day."""
    _need_gpu()
    c = rx.panel(800, 64, 7)
    turb, quad = _turbulence(c, 64)
    np.testing.assert_array_equal(turb, 0.0)
    np.testing.assert_array_equal(quad, 0.0)
    _check("T=W+1 N=7", rx.panel(801, 65, 7), 64)
    _check("T=W+1 N=128", rx.panel(802, 253, 128), 252)


def test_refused_shapes():
    _need_gpu()
    from finrl_amd import _native as nat
    from finrl_amd import riskpre
    with pytest.raises(nat.FinenvError):
        riskpre.calculate_turbulence(rx.panel(900, 300, 129), window=252)
    with pytest.raises(nat.FinenvError):
        riskpre.calculate_turbulence(rx.panel(901, 30, 4), window=2)
    with pytest.raises(nat.FinenvError):
        riskpre.rolling_covariance(rx.panel(902, 300, 129), lookback=252)
    with pytest.raises(nat.FinenvError):
        riskpre.rolling_covariance(rx.panel(903, 30, 4), lookback=1)


def test_non_finite_tensor_rejected():
    """A torch.Tensor close is checked for NaN / inf exactly like an ndarray."""
    _need_gpu()
    from finrl_amd import _native as nat
    from finrl_amd import riskpre
    c = rx.panel(910, 80, 4)
    for bad in (np.nan, np.inf):
        c2 = c.copy()
        c2[40, 2] = bad
        for arg in (c2, torch.from_numpy(c2), torch.from_numpy(c2).cuda()):
            with pytest.raises(nat.FinenvError, match="NaN"):
                riskpre.calculate_turbulence(arg, window=63)
            with pytest.raises(nat.FinenvError, match="NaN"):
                riskpre.rolling_covariance(arg, lookback=63)


def test_add_turbulence_single_ticker():
    """add_turbulence on a one-ticker frame returns the reference's values (FeatureEngineer
    handles N = 1: 1 x 1 cov, pinv, x^2 / var)."""
    _need_gpu()
    import os

    import pandas as pd
    from finrl_amd import riskpre
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "riskpre_n1.npz"), allow_pickle=False)
    T = z["close"].shape[0]
    dates = pd.bdate_range("2015-01-01", periods=T).strftime("%Y-%m-%d")
    df = pd.DataFrame({"date": dates, "tic": "T0", "close": z["close"][:, 0]})
    out = riskpre.add_turbulence(df)
    np.testing.assert_array_equal(out["turbulence"].to_numpy() == 0, z["turbulence"] == 0)
    np.testing.assert_allclose(out["turbulence"].to_numpy(), z["turbulence"], rtol=1e-12)


# -------------------------------------------------------------------------------------- returns
def test_returns_past_one_grid():
    """T x N = 1,062,400 > 4096 blocks x 256 threads: the grid-stride loop runs a second pass.
    fp64 division is IEEE-rounded on both sides: bit equality."""
    _need_gpu()
    from finrl_amd import riskpre
    T, N = 8300, 128
    assert T * N > 4096 * 256
    close = rx.panel(920, T, N, sigma=0.002)
    ret, _ = riskpre._returns(torch.from_numpy(close).cuda())
    got = ret.cpu().numpy()
    assert np.isnan(got[0]).all()
    np.testing.assert_array_equal(got[1:], close[1:] / close[:-1] - 1)


# ----------------------------------------------------------------------------- rolling covariance
@pytest.mark.parametrize("N", [1, 2, 33, 128])
@pytest.mark.parametrize("L,T,level", [(2, 3, 50.0), (2, 40, 1e5), (252, 253, 1e-3),
                                       (252, 262, 50.0)])
def test_rolling_covariance(N, L, T, level):
    """cov_list vs the exact covariance, elementwise within the fp64 rounding budget
    (n + 4) x 2^-53 x sum_t (|r_a| + |m_a|)(|r_b| + |m_b|) / (n - 1); symmetry exact."""
    _need_gpu()
    from finrl_amd import riskpre
    close = rx.panel(1000 + N + L, T, N, level=level)
    got = riskpre.rolling_covariance(close, lookback=L).cpu().numpy()
    exact, budget = rx.covariance_exact(close, L)
    assert got.shape == (T - L, N, N)
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
    err = np.abs(got - exact.astype(np.float64))
    lim = (L + 4) * rx.U64 * budget
    print(f"cov N={N} L={L} T={T} level={level:.0e}: max err / budget "
          f"{(err / budget).max() / rx.U64:.2f} ulp-units")
    assert (err <= lim).all()
