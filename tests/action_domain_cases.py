"""Action sets outside the interval every other stock test draws from (uniform(-1, 1)), shared by
tests/test_gpu_stock_action_domain.py (HIP kernels vs the oracle) and tests/test_oracle_action_domain.py
(the oracle vs oracle/pandas_env.py).  Everything here is host-side NumPy and checks its own
constructions: a case that does not hold what its name says raises instead of testing less.

The reference env does not clip: `actions * hmax` (a float32 multiply) then `.astype(int)`
(env_stocktrading.py:304-305).  A kernel saturates the scaled integer at its `amax` (include/finenv.h,
"Action domain"); expectations for saturated actions come from the oracle fed `saturated()` actions.
NaN and +-inf actions are out of scope: the reference's own cast is undefined there."""
import math

import numpy as np

F32 = np.float32


def scaled(actions, hmax):
    """trunc(f32(action) * f32(hmax)) as int64: :304-305."""
    x = np.asarray(actions, F32) * F32(hmax)
    assert x.dtype == F32
    return np.trunc(x).astype(np.int64)


def pow2_hmax(hmax):
    """The power-of-two hmax that steps the same kernel as `hmax` does (the N = 100 fast kernel takes
    hmax <= 255): k / hmax and f32(k / hmax) * f32(hmax) are then exact for every integer k an f32
    holds, so an action asks for exactly the scaled integer it was built from."""
    return 128 if hmax <= 255 else 512


def saturated(actions, hmax, amax):
    """The actions a kernel that saturates at +-amax effectively sees: clip(trunc(a*hmax)) / hmax."""
    assert hmax & (hmax - 1) == 0, "exact only for a power-of-two hmax"
    want = np.clip(scaled(actions, hmax), -amax, amax)
    out = (want / hmax).astype(F32)
    np.testing.assert_array_equal(scaled(out, hmax), want)
    return out


def below(amax):
    """`amax - 1` as an f32 product can hold it: the largest integer below amax that float32 represents
    (amax - 1 up to 2^24, amax - 2 at 2^25)."""
    return int(np.nextafter(F32(amax), F32(0)))


def above(amax):
    """`amax + 1` likewise: the smallest float32 integer above amax."""
    return int(np.nextafter(F32(amax), F32(np.inf))) if amax >= 1 << 24 else amax + 1


# ---------------------------------------------------------------- (a) truncation boundaries
def boundary_values(hmax):
    """k / hmax and its two float32 neighbours for every integer k in [-hmax, hmax]; +-0.0, +-1.0, the
    smallest normal, a denormal, and values with |a * hmax| < 1."""
    k = np.arange(-hmax, hmax + 1)
    base = (k / hmax).astype(F32)
    tiny, den = np.finfo(F32).tiny, F32(1e-42)
    sub = F32(1.0) / F32(hmax)
    extra = np.array([0.0, -0.0, 1.0, -1.0, tiny, -tiny, den, -den, sub / 2, -sub / 2,
                      np.nextafter(sub, F32(0)), -np.nextafter(sub, F32(0)),
                      F32(0.999) * sub, -F32(0.999) * sub], F32)
    assert (np.abs(scaled(extra[4:], hmax)) == 0).all()
    return np.concatenate([base, np.nextafter(base, F32(-np.inf)), np.nextafter(base, F32(np.inf)),
                           extra])


def boundary_tiles(hmax, E, N, steps, seed):
    """[steps, E, N] float32: every step a fresh permutation of boundary_values(hmax), repeated over
    the flat tile -- each full 64-env block holds every value in every step, in other columns each
    time."""
    vals = boundary_values(hmax)
    assert 64 * N >= len(vals) and E >= 128
    rng = np.random.default_rng(seed)
    out = np.empty((steps, E, N), F32)
    for s in range(steps):
        out[s] = np.resize(vals[rng.permutation(len(vals))], E * N).reshape(E, N)
        for blk in (out[s, :64], out[s, 64:128]):
            assert np.isin(vals.view(np.uint32), blk.view(np.uint32)).all()
    return out


# ---------------------------------------------------------------- (b), (c) beyond [-1, 1]
def magnitudes_inside(amax):
    """(b): scaled magnitudes outside [-1, 1] * hmax, up to the clamp."""
    return [255, 256, 257, 511, 512, 32767, 32768, 65535, 1 << 16, 1 << 20, below(amax), amax]


def magnitudes_beyond(amax):
    """(c): at and past the clamp."""
    return [above(amax), 2 * amax, 1 << 30, (1 << 31) - 128]


def big_tiles(mags, hmax, E, N, steps, seed):
    """[steps, E, N] float32 rows mixing +-m / hmax for m in mags (45 %), a few in-range values
    repeated all over the row (exact ties, 30 %) and uniform(-1, 1) draws."""
    assert hmax & (hmax - 1) == 0
    rng = np.random.default_rng(seed)
    signed = np.array([s * m for m in mags for s in (1, -1)], np.int64)
    big = (signed / hmax).astype(F32)
    np.testing.assert_array_equal(scaled(big, hmax), signed)      # each asks for exactly its integer
    ties = np.array([-1.0, -0.5, -3.0 / hmax, 0.0, 3.0 / hmax, 0.5, 1.0], F32)
    u = rng.random((steps, E, N))
    out = rng.uniform(-1, 1, (steps, E, N)).astype(F32)
    out = np.where(u < 0.75, ties[rng.integers(0, len(ties), u.shape)], out)
    out = np.where(u < 0.45, big[rng.integers(0, len(big), u.shape)], out)
    return out.astype(F32), signed


def env_books(E, N, seed):
    """Per-env (initial_amount [E], num_stock_shares [E, N]) in four kinds, e % 4:
    0 holdings far above 2^25 per ticker and cash 10^12 -- the action binds on both sides;
    1 a few shares and cash 10^5 -- holdings bind the sells, cash the buys;
    2 large holdings and cash 10^4;   3 up to 300 shares and cash 10^12."""
    rng = np.random.default_rng(seed)
    kind = np.arange(E) % 4
    cash = np.choose(kind, [1e12, 1e5, 1e4, 1e12]).astype(np.float64)
    large = (1 << 28) + rng.integers(0, 1 << 20, (E, N))
    small = np.where((kind == 3)[:, None], rng.integers(0, 300, (E, N)), rng.integers(0, 40, (E, N)))
    shares = np.where((kind % 2 == 0)[:, None], large, small).astype(np.int64)
    return cash, shares


def assert_both_bind(want, realised, values):
    """For every requested scaled integer in `values`: somewhere the trade is the action itself, and
    somewhere holdings or cash cut it short.  want / realised: int [steps, E, N] (oracle)."""
    for v in sorted(set(int(x) for x in values)):
        got = realised[want == v]
        assert got.size and (got == v).any(), f"scaled action {v} never binds"
        assert (np.abs(got) < abs(v)).any(), f"scaled action {v}: holdings / cash never bind"


# ---------------------------------------------------------------- (d) floor division
def floordiv_cases(close_row, buy_cost_pct, E, k_lo, k_hi, need_differ, seed):
    """One buy per env: ticker e % N, cash c[e] one of {fl(k * unit), its two float64 neighbours} for
    a random k in [k_lo, k_hi), unit = close * (1 + buy_cost_pct).  With need_differ every case is one
    where Python's exact `c // unit` differs from floor(c / unit) or from floor(c * (1 / unit)).
    -> tickers [E], cash [E], q [E] = c // unit."""
    rng = np.random.default_rng(seed)
    N = len(close_row)
    tick = np.arange(E) % N
    cash, q = np.empty(E), np.empty(E, np.int64)
    for e in range(E):
        unit = float(close_row[tick[e]]) * (1 + buy_cost_pct)
        for _ in range(10_000):
            k = int(rng.integers(k_lo, k_hi))
            c = float(np.nextafter(k * unit, [-np.inf, k * unit, np.inf][int(rng.integers(0, 3))]))
            exact = c // unit
            if not need_differ or exact != math.floor(c / unit) or exact != math.floor(c * (1 / unit)):
                break
        else:
            raise AssertionError("no floor-division case found")
        assert k - 1 <= exact <= k
        cash[e], q[e] = c, int(exact)
    return tick, cash, q
