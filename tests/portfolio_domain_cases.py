"""Portfolio scores and closes outside the range every other portfolio test draws from (scores in
[0, 3], closes within 10 % of 100), shared by tests/test_gpu_portfolio_domain.py and the portfolio cases
of tests/test_gpu_degenerate_shapes.py (HIP kernel vs oracle/portfolio_oracle.c),
tests/test_oracle_portfolio_domain.py (the oracle vs the unmodified reference's recorded outputs) and
tests/golden/make_golden.py (scenario portfolio:domain).  Everything here is host-side NumPy and checks
its own constructions: a case that does not hold what its name says raises instead of testing less.

The reference does not stabilise its softmax: `np.exp(actions) / np.sum(np.exp(actions))` in float32
(env_portfolio.py:225-229), whatever IEEE makes of it -- include/finenv.h, "Portfolio action and panel
domain".  Two kinds of expectation follow.  Where every exponential and their sum are finite and the sum
is positive, a weight must lie in an interval DERIVED from "expf is within 1 ulp" (weight_bounds); the
oracle's and the device's expf may both be honest and still differ by thousands of ulp of a weight once
the exponentials are subnormal, so no ulp bound against the oracle exists there.  Everywhere else
(overflow, sum overflow, complete underflow) the weights are 0 or NaN and must equal the oracle's.

The portfolio value of a step is bounded the same way from the weight intervals (value_bounds), given
the value BEFORE the step as an input.

Out of scope: NaN and +inf scores (unspecified in include/finenv.h); -inf is a score like any other
(its exponential is 0).  Negative closes, and the metrics of NaN series."""
import collections

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
SUB = 2.0 ** -149                       # the float32 subnormal unit
# float32 exp: overflows above ln(FLT_MAX), subnormal below ln(2^-126), zero below ln(2^-150)
THRESHOLDS = (88.7228, -87.3365, -103.9721)

KINDS = ("signed", "wide", "ties", "one_hot", "sum_overflow", "exp_overflow", "subnormal", "sub_mixed",
         "all_underflow", "part_underflow", "sum_order")
POISONING = ("exp_overflow", "all_underflow")          # their weights are NaN: the value is NaN until reset
PANEL_KINDS = ("signed", "wide", "one_hot", "part_underflow")
SMALL_SHAPE_KINDS = ("signed", "wide")
SUM_ORDER_TOL = 3 * 2.0 ** -24


def _exp32(a):
    with np.errstate(over="ignore", under="ignore"):
        x = np.exp(np.asarray(a, F32))
    assert x.dtype == F32
    return x


def _sum32(x):
    with np.errstate(over="ignore"):
        s = np.sum(x, axis=-1)
    assert s.dtype == F32
    return s


def hot_column(rank, step, N):
    """The column a `one_hot` env holds on a step: it moves on by one every step, and differs by env."""
    return (np.asarray(rank) + step) % N


# ---------------------------------------------------------------- action rows
def rows(kind, rng, M, N, hot=None):
    """[M, N] float32 rows of one kind (hot [M]: the column a `one_hot` row holds; drawn if None).  Checked
    by check_rows before they are returned."""
    if kind == "sum_overflow" and N < 2:
        kind = "wide"                       # one finite exponential cannot overflow a sum
    if kind == "signed":
        a = rng.uniform(-1, 1, (M, N))
        u = rng.random((M, N))
        a[u < 0.1] = 0.0
        a[u > 0.9] = -0.0
        if a.size >= 2:                     # both zeros are there whatever was drawn
            i = rng.permutation(a.size)[:2]
            a.flat[i[0]], a.flat[i[1]] = 0.0, -0.0
    elif kind == "wide":
        a = rng.uniform(-80, 80, (M, N))
    elif kind == "ties":
        a = np.repeat(rng.uniform(-80, 80, (M, 1)), N, axis=1)
    elif kind == "one_hot":
        a = np.full((M, N), -60.0)
        a[np.arange(M), rng.integers(0, N, M) if hot is None else hot] = 60.0
    elif kind == "sum_overflow":
        # every exponential finite, N of them past FLT_MAX: a_i >= ln(FLT_MAX) - ln(N), with a margin
        a = rng.uniform(max(88.0, 88.7228 - np.log(N) + 0.03), 88.7, (M, N))
    elif kind == "exp_overflow":
        a = rng.uniform(-5, 88, (M, N))
        over = rng.random((M, N)) < 0.3
        over[np.arange(M), rng.integers(0, N, M)] = True
        a = np.where(over, rng.uniform(89, 200, (M, N)), a)
    elif kind == "subnormal":
        a = rng.uniform(-103, -88, (M, N))
    elif kind == "sub_mixed":
        a = rng.uniform(-103, -88, (M, N))
        upper = np.argsort(rng.random((M, N)), axis=1) < N // 2
        a = np.where(upper, rng.uniform(-87, -60, (M, N)), a)
    elif kind == "all_underflow":
        a = rng.uniform(-300, -105, (M, N))
    elif kind == "part_underflow":
        a = np.where(rng.random((M, N)) < 0.5, -200.0, -np.inf)
        zero = rng.random((M, N)) < 0.4
        zero[np.arange(M), rng.integers(0, N, M)] = True
        a[zero] = 0.0
    elif kind == "sum_order":
        # column 0 at 0 (exp = 1), the rest at exp ~ 0.95 * 2^-24, just under half an ulp of 1: a
        # left-to-right float32 sum drops every one of them, NumPy's pairwise sum (8 accumulators from
        # N = 8 on) keeps those that meet each other first -- the sums differ by 3 ulp at N = 8, 9
        # and by more at every larger N, see check_sum_order
        a = rng.uniform(np.log(0.94 * 2.0 ** -24), np.log(0.96 * 2.0 ** -24), (M, N))
        a[:, 0] = 0.0
    else:
        raise ValueError(kind)
    a = a.astype(F32)
    check_rows(kind, a)
    return a


def check_rows(kind, a):
    """Raise unless every row of a [M, N] holds what `kind` says."""
    a = np.asarray(a)
    M, N = a.shape
    assert a.dtype == F32 and not np.isnan(a).any() and not (a == np.inf).any()
    fin = a[np.isfinite(a)].astype(np.float64)
    for t in THRESHOLDS:
        assert (np.abs(fin - t) > 0.01).all(), f"{kind}: a score within 0.01 of {t}"
    x = _exp32(a)
    den = _sum32(x)
    normal = (x >= np.finfo(F32).tiny) & np.isfinite(x)
    sub = (x > 0) & (x < np.finfo(F32).tiny)
    if kind == "sum_overflow" and N < 2:
        kind = "wide"
    if kind == "signed":
        assert (np.abs(a) <= 1).all()
        zero = a == 0
        if a.size >= 2:
            assert (zero & ~np.signbit(a)).any() and (zero & np.signbit(a)).any(), "signed: no +0.0 / -0.0"
        if a.size >= 64:
            assert (a < 0).any() and (a > 0).any()
    elif kind == "wide":
        assert (np.abs(a) <= 80).all() and normal.all()
    elif kind == "ties":
        assert (a == a[:, :1]).all() and (np.abs(a) <= 80).all()
    elif kind == "one_hot":
        assert ((a == 60).sum(1) == 1).all() and ((a == -60).sum(1) == N - 1).all()
    elif kind == "sum_overflow":
        assert (a >= 88.0).all() and (a <= 88.7).all()
        assert np.isfinite(x).all() and np.isinf(den).all()
    elif kind == "exp_overflow":
        over = a >= 89
        assert over.any(1).all() and (a <= 200).all() and (a[~over] <= 88).all() and (a >= -5).all()
        assert np.isinf(x[over]).all() and np.isfinite(x[~over]).all()
    elif kind == "subnormal":
        assert (a >= -103).all() and (a <= -88).all() and sub.all()
    elif kind == "sub_mixed":
        low = a <= -88
        assert (low.sum(1) == N - N // 2).all() and (a >= -103).all() and (a[~low] >= -87).all() and \
            (a[~low] <= -60).all()
        assert sub[low].all() and normal[~low].all()
    elif kind == "all_underflow":
        assert (a >= -300).all() and (a <= -105).all() and (x == 0).all()
    elif kind == "part_underflow":
        assert ((a == 0) | (a == -200) | (a == -np.inf)).all() and (a == 0).any(1).all()
        assert ((x == 0) | (x == 1)).all()
    elif kind == "sum_order":
        t = x[:, 1:].astype(np.float64) * 2.0 ** 24
        assert (x[:, 0] == 1).all() and (t > 0.93).all() and (t < 0.97).all()
    else:
        raise ValueError(kind)


def kinds_of(E, kinds):
    """-> names [E] (env e is of kind e % len(kinds): every 64-env block holds them all), rank [E]."""
    e = np.arange(E)
    return np.array(kinds)[e % len(kinds)], e // len(kinds)


def poison_step(rank, T):
    """The step of its episode on which a poisoning env gets its poisoning row (0 .. T - 2)."""
    return np.asarray(rank) % max(T - 1, 1)


def actions(kinds, E, N, steps, T, seed):
    """[steps, E, N] float32 for a lock-step batch whose episodes take T steps (T - 1 that trade and the
    terminal one, after which the batch is reset).  Env e is of kind kinds[e % len(kinds)].  An env of
    a poisoning kind gets its own kind's row on ONE step per episode, poison_step(e // len(kinds), T),
    and `wide` rows on the others, so that the NaN lands early in some envs and late in others."""
    rng = np.random.default_rng(seed)
    names, rank = kinds_of(E, kinds)
    out = np.empty((steps, E, N), F32)
    for s in range(steps):
        for k in kinds:
            m = names == k
            if not m.any():
                continue
            if k in POISONING:
                hit = m & (poison_step(rank, T) == s % T)
                out[s, m & ~hit] = rows("wide", rng, int((m & ~hit).sum()), N)
                if hit.any():
                    out[s, hit] = rows(k, rng, int(hit.sum()), N)
            else:
                out[s, m] = rows(k, rng, int(m.sum()), N, hot=hot_column(rank[m], s, N))
    if steps >= T - 1:                                   # every env of a poisoning kind was poisoned
        for k in set(kinds) & set(POISONING):
            for e in np.flatnonzero(names == k):
                check_rows(k, out[int(poison_step(rank[e], T)), e][None])
    return out


def fixture_actions(S, N, T, seed):
    """[S, N] for the one env of the reference fixture on the `zeros` panel (T = 14, three episodes), and
    the kind of every row.  Every kind occurs, each episode opens with the kinds that leave a finite value:
      episode 0: finite up to day 9, where `signed` weights meet the +inf return (value +inf), then
                 `exp_overflow` (NaN weights on a value of +inf);
      episode 1: the `one_hot` row of step 8 holds exactly the ticker that goes to 0 (value 0.0), then
                 `part_underflow` on day 9 (0 * inf);
      episode 2: `all_underflow` on step 6 turns a finite value into NaN."""
    assert T == 14 and S == 3 * T
    rng = np.random.default_rng(seed)
    z = panel_roles(T, N, "zeros").zero
    np_ = ["signed", "wide", "ties", "one_hot", "sum_overflow", "subnormal", "sub_mixed", "part_underflow",
           "sum_order"]
    plan = [np_[4:] + np_[:4] + ["signed", "exp_overflow", "all_underflow", "ties", "wide"],
            np_[4:] + np_[:4] + ["part_underflow", "subnormal", "exp_overflow", "sum_order", "wide"],
            np_[:6] + ["all_underflow"] + np_[6:] + ["one_hot", "exp_overflow", "sub_mixed", "wide"]]
    plan[0][8], plan[0][7] = "wide", "one_hot"          # episode 0 reaches day 9 with a positive value
    names = [k for ep in plan for k in ep]
    assert len(names) == S and set(names) == set(KINDS) and plan[1][8] == "one_hot"
    out = np.stack([rows(k, rng, 1, N, hot=np.array([z if s == T + 8 else (z + 1 + s) % N]))[0]
                    for s, k in enumerate(names)])
    return out, names


# ---------------------------------------------------------------- panels
def benign_panel(T, N, K, seed):
    """The panel the other portfolio tests draw: a 1 % walk around 100."""
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    return close, rng.normal(0, 1e-4, (T, N, N)), rng.normal(0, 1, (T, K, N))


PanelRoles = collections.namedtuple("PanelRoles", "zero_day zero flat up down zero2 late_zero pair pair_day")


def panel_roles(T, N, variant):
    """Which (day, ticker) cells edit_close edits.  The ticker that goes to 0 on `zero_day` is the one
    a `one_hot` env of rank 1 holds on the step into that day (hot_column)."""
    assert T >= 14 and N >= 8
    zd = 9
    z = int(hot_column(1, zd - 1, N))
    t = [(z + j) % N for j in range(7)]
    pair_day = {"zeros": T - 2, "nan": zd}[variant]
    return PanelRoles(zd, t[0], t[1], t[2], t[3], t[4], t[5], t[6] if variant == "zeros" else t[0], pair_day)


def edit_close(close, variant="zeros"):
    """close [T, N] f64 (a usual-scale base, all > 0) -> an edited copy:
      * one ticker flat over days 2 -> 3 (return exactly 0), a x1e6 jump on day 4, a /1e6 jump on day 6;
      * day 9: one ticker goes to 0 (return -1 into the day; a `one_hot` env that holds exactly that
        ticker ends at a value of exactly 0.0);
      * variant "zeros": that zero and a second one on day 9 are followed by positive closes (return
        +inf out of the day: +inf for an env with weight on the ticker, NaN for one with weight 0), a
        third zero on day 11, and two consecutive zeros on the last two days (0 / 0 = NaN);
      * variant "nan": the zero of day 9 stays on day 10 (return NaN out of day 9), one more zero on
        day 12.
    A return of +inf or NaN leaves no env of a lock-step batch with a finite value, so the events that
    must meet a finite value share day 9, and the NaN return has a variant of its own.  No zero in row 0."""
    close = np.array(close, np.float64)
    T, N = close.shape
    assert (close > 0).all()
    r = panel_roles(T, N, variant)
    close[3, r.flat] = close[2, r.flat]
    close[4:, r.up] *= 1e6
    close[6:, r.down] /= 1e6
    close[r.zero_day, r.zero] = 0.0
    if variant == "zeros":
        close[r.zero_day, r.zero2] = 0.0
        close[11, r.late_zero] = 0.0
        close[r.pair_day:r.pair_day + 2, r.pair] = 0.0
    else:
        close[r.zero_day + 1, r.zero] = 0.0
        close[12, r.late_zero] = 0.0
    assert (close[0] > 0).all()
    g = gross_returns(close)
    assert g[2, r.flat] == 0.0 and g[3, r.up] > 9e5 and -1 < g[5, r.down] < -0.99999
    assert g[r.zero_day - 1, r.zero] == -1.0 and np.isnan(g[r.pair_day, r.pair])
    assert np.isfinite(g[:r.zero_day]).all()
    if variant == "zeros":
        assert g[r.zero_day, r.zero] == np.inf and g[r.zero_day, r.zero2] == np.inf
    return close


def gross_returns(close):
    """close[t + 1] / close[t] - 1 in fp64, [T, N] with a last row of zeros (PortfolioPanel.gross_returns)."""
    g = np.zeros(close.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        g[:-1] = (close[1:] / close[:-1]) - 1
    return g


# ---------------------------------------------------------------- the derived bounds
def weight_bounds(a):
    """-> wlo, whi [M, N] f64 and applies [M] for score rows a [M, N] f32.  With x_i the float32 rounding
    of exp(a_i), lo_i / hi_i its float32 neighbours (an expf within 1 ulp -- one unit of 2^-149 for a
    subnormal result -- lies between them), L = sum lo, H = sum hi and s = (N + 4) * 2^-24 for the
    roundings of the float32 sum and the division, the weight lies in
    [lo_i / H * (1 - s) - 2^-149, hi_i / L * (1 + s) + 2^-149].
    applies: every hi_i finite, H < FLT_MAX and L > 0; the other rows must equal the oracle's."""
    a = np.asarray(a, F32)
    N = a.shape[-1]
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        x = np.exp(a.astype(np.float64)).astype(F32)
        lo = np.maximum(0.0, np.nextafter(x, F32(-np.inf)).astype(np.float64))
        hi = np.nextafter(x, F32(np.inf)).astype(np.float64)
        L, H = lo.sum(-1, keepdims=True), hi.sum(-1, keepdims=True)
        applies = np.isfinite(hi).all(-1) & (H[..., 0] < FLT_MAX) & (L[..., 0] > 0)
        s = (N + 4) * 2.0 ** -24
        wlo = lo / H * (1 - s) - SUB
        whi = hi / L * (1 + s) + SUB
    return wlo, whi, applies


def same_class(got, want, what=""):
    """NaN, +inf, -inf and exact zeros of `want` must be NaN, +inf, -inf and zeros of `got`, and the
    other way round."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for name, f in (("NaN", np.isnan), ("+inf", lambda v: v == np.inf), ("-inf", lambda v: v == -np.inf),
                    ("zero", lambda v: v == 0)):
        np.testing.assert_array_equal(f(got), f(want), err_msg=f"{what}: {name} positions")


def check_weights(a, got, oracle, what=""):
    """got / oracle [M, N] f32 softmax weights of score rows a [M, N]: inside weight_bounds where they
    apply, equal to the oracle's (NaN at the same places) elsewhere.  -> number of rows bounded."""
    got, oracle = np.asarray(got, F32), np.asarray(oracle, F32)
    wlo, whi, applies = weight_bounds(a)
    g64 = got.astype(np.float64)
    bad = applies[:, None] & ~((g64 >= wlo) & (g64 <= whi))
    assert not bad.any(), (what, "weights outside the derived bound", np.argwhere(bad)[:5],
                           a[bad][:5], got[bad][:5], wlo[bad][:5], whi[bad][:5])
    o64 = oracle.astype(np.float64)
    assert ((o64 >= wlo) & (o64 <= whi))[applies].all(), (what, "the oracle leaves the derived bound")
    np.testing.assert_array_equal(got[~applies], oracle[~applies], err_msg=f"{what}: degenerate rows")
    return int(applies.sum())


def check_sum_order(a, got, oracle, what=""):
    """Rows of kind `sum_order` (column 0 at 0, the others tiny): w_0 = x_0 / den, and den = x_0 + (what
    the summation order keeps of the tiny terms) -- a 1-ulp error of x_0 cancels in the quotient to first
    order, one of a tiny term is 2^-47.  What is left between two honest pairwise sums is one rounding
    of den that falls the other way (2^-23 relative) and the two roundings of the division (2^-25 each
    below 1): 3 * 2^-24.  A left-to-right sum keeps none of the tiny terms and is off by 2^-23 per kept
    pair: 3 * 2^-23 at N = 8, 9 and more beyond."""
    d = np.abs(np.asarray(got, np.float64)[:, 0] - np.asarray(oracle, np.float64)[:, 0])
    assert (d <= SUM_ORDER_TOL).all(), (what, "w_0 of sum_order rows", d.max(), SUM_ORDER_TOL)


def value_bounds(v, g, wlo, whi):
    """Interval of v * (1 + sum_i g_i * w_i) for w_i in [wlo_i, whi_i]: v [M] f64 (the value before the
    step, an input), g [M, N] f64 gross returns.  ret_lo / ret_hi take the smaller / larger end of every
    term, widened by N * 2^-52 * sum |g_i| * whi_i for the fp64 sum's roundings; the ends are sorted
    (v < 0) and widened by 2 ulp.  Rows with a non-finite end come back as NaN: the class check decides."""
    v = np.asarray(v, np.float64)
    N = g.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        t0, t1 = g * wlo, g * whi
        slack = N * 2.0 ** -52 * np.sum(np.abs(g) * whi, axis=-1)
        ret_lo = np.sum(np.minimum(t0, t1), axis=-1) - slack
        ret_hi = np.sum(np.maximum(t0, t1), axis=-1) + slack
        e0, e1 = v * (1 + ret_lo), v * (1 + ret_hi)
        lo, hi = np.minimum(e0, e1), np.maximum(e0, e1)
        ok = np.isfinite(lo) & np.isfinite(hi)
        lo = np.where(ok, lo - 2 * np.spacing(np.abs(np.where(ok, lo, 0.0))), np.nan)
        hi = np.where(ok, hi + 2 * np.spacing(np.abs(np.where(ok, hi, 0.0))), np.nan)
    return lo, hi


def check_values(a, v_before, g, got, oracle, oracle_w, what=""):
    """got / oracle [M]: the new portfolio values of rows that traded.  Same class as the oracle's where
    that is NaN, +-inf or 0; inside value_bounds wherever the interval is finite and the oracle's value
    is.  Rows whose weights are bounded use the weight interval, the others the oracle's own weights."""
    wlo, whi, applies = weight_bounds(a)
    ow = np.asarray(oracle_w, np.float64)
    wlo = np.where(applies[:, None], wlo, ow)
    whi = np.where(applies[:, None], whi, ow)
    same_class(got, oracle, what)
    lo, hi = value_bounds(v_before, g, wlo, whi)
    chk = np.isfinite(lo) & np.isfinite(oracle)
    got = np.asarray(got, np.float64)
    bad = chk & ~((got >= lo) & (got <= hi))
    assert not bad.any(), (what, "value outside the derived bound", np.flatnonzero(bad)[:5], got[bad][:5],
                           lo[bad][:5], hi[bad][:5])
    return int(chk.sum())


# ---------------------------------------------------------------- oracle traces and what they hold
def oracle_trace(orc, acts, auto_reset=True):
    """Drive a lock-step PortfolioOracle batch over acts [S, E, N]; with auto_reset off it is reset when
    every env is done.  -> obs0, per step a dict: day / value before the step, done, the weights (NaN rows
    on a terminal step), the fp64 reward (the new value where the step traded, else the last reward),
    obs (after any reset), term (the row a terminal step returned), value / day after the step."""
    obs0 = orc.reset()
    trace = []
    for s in range(len(acts)):
        pre = orc.state()
        obs, rew, done, term, w = orc.vec_step_weights(acts[s], auto_reset=auto_reset)
        if not auto_reset:
            term = obs
            if done.all():
                obs = orc.reset()
            else:
                assert not done.any()
        post = orc.state()
        trace.append(dict(day0=pre["day"].copy(), value0=pre["value"].copy(), done=done, weights=w, rew=rew,
                          obs=obs, term=term, value=post["value"].copy(), day=post["day"].copy()))
    return obs0, trace


def finite_share(trace):
    """Share of the (env, step) pairs that trade whose oracle value before the step is finite."""
    live = np.stack([~t["done"] for t in trace])
    fin = np.stack([np.isfinite(t["value0"]) for t in trace])
    return float((live & fin).sum()) / max(int(live.sum()), 1)


def panel_events(g, trace):
    """Counts, from the oracle's outputs alone and among the (env, step) pairs that trade on a finite value,
    of what edit_close plants; raises where the oracle's new value is not what the event gives."""
    ev = collections.Counter()
    for t in trace:
        m = ~t["done"] & np.isfinite(t["value0"])
        if not m.any():
            continue
        gr = g[t["day0"][m]]
        w = t["weights"][m].astype(np.float64)
        v0, v1 = t["value0"][m], t["rew"][m]
        nan_ret = np.isnan(gr).any(1)
        inf_pos = ((gr == np.inf) & (w > 0)).any(1)
        inf_zero = ((gr == np.inf) & (w == 0)).any(1)
        wiped = ((gr == -1.0) & (w == 1.0)).any(1) & ((w != 0).sum(1) == 1) & np.isfinite(gr).all(1)
        assert np.isnan(v1[nan_ret | inf_zero]).all()
        only_pos = inf_pos & ~inf_zero & ~nan_ret & (v0 > 0)
        assert (v1[only_pos] == np.inf).all()
        assert (v1[wiped] == 0.0).all() and not np.signbit(v1[wiped]).any()
        ev["nan_return"] += int(nan_ret.sum())
        ev["inf_return_weight_pos"] += int(inf_pos.sum())
        ev["inf_return_weight_zero"] += int(inf_zero.sum())
        ev["value_plus_inf"] += int(only_pos.sum())
        ev["minus_one_weight_one"] += int(wiped.sum())
        ev["flat_return"] += int(((gr == 0.0) & (w > 0)).any(1).sum())
        ev["jump_up"] += int(((gr > 9e5) & np.isfinite(gr) & (w > 0)).any(1).sum())
        ev["jump_down"] += int(((gr < -0.99999) & (gr > -1) & (w > 0)).any(1).sum())
        ev["zero_value_steps"] += int((v0 == 0).sum())
    return ev


def require_panel_events(variant, ev):
    need = ["minus_one_weight_one", "flat_return", "jump_up", "jump_down", "zero_value_steps"]
    need += {"zeros": ["inf_return_weight_pos", "inf_return_weight_zero", "value_plus_inf"],
             "nan": ["nan_return"]}[variant]
    for k in need:
        assert ev[k] > 0, f"{variant}: event {k} never meets a finite value ({dict(ev)})"


# ---------------------------------------------------------------- the reference fixture
def fixture_values_before(z):
    """The reference's portfolio value before every step of tests/golden/portfolio_domain.npz."""
    v = np.empty(len(z["value"]))
    v[0] = z["cfg_float"][0]
    v[1:] = np.where(z["done"][:-1], z["cfg_float"][0], z["value"][:-1])
    return v


def check_fixture_step(z, s, weights, value_before, value, what=""):
    """One trading step of a candidate (the oracle, or one env of the device batch) against step s of the
    fixture: weights [N] f32, the candidate's own value before the step, its new value.
      * the weights against the reference's: check_weights, the same NaN / inf / zero positions, and
        check_sum_order on rows of that kind;
      * the new value: the class of the reference's, and inside value_bounds taken from the candidate's own
        value before the step (an input of the step, as on the device);
      * the reference itself: its value of step s inside value_bounds taken from ITS value before the step,
        its weights inside weight_bounds -- the derived bounds hold for NumPy's exp and sum, too."""
    assert not z["done"][s]
    a = z["actions"][s][None]
    ref_w = z["weights"][s][None]
    g = gross_returns(z["close"])[z["day"][s] - 1][None]
    weights = np.asarray(weights, F32)[None]
    what = f"{what} step {s} ({z['kinds'][s]})"
    check_weights(a, weights, ref_w, what)
    same_class(weights, ref_w, what + " weights")
    if z["kinds"][s] == "sum_order":
        check_sum_order(a, weights, ref_w, what)
    n = check_values(a, np.array([value_before]), g, np.array([value]), z["value"][s:s + 1], ref_w, what)
    n_ref = check_values(a, fixture_values_before(z)[s:s + 1], g, z["value"][s:s + 1], z["value"][s:s + 1],
                         ref_w, what + " reference")
    assert n == n_ref
    return n
