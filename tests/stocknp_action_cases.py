"""Action sets for the array-state stock step (VecStockTradingEnvNP / oracle.stocknp.StockNpOracle)
outside what every other test of it draws (uniform(-1, 1) at max_stock = 100, so scaled actions within
+-100), shared by tests/test_gpu_stocknp_action_domain.py (the HIP kernel vs the oracle),
tests/test_oracle_stocknp_action_domain.py (the oracle alone: every case must reach the events it exists
for) and tests/golden/make_golden.py (the oracle vs the unmodified reference, stocknp_actdom_*.npz).
Everything here is host-side NumPy plus the CPU oracle and checks its own constructions: a case that does
not hold what its name says raises instead of testing less.

The reference does not clip: `(actions * max_stock).astype(int)` is a float32 multiply, then truncation
toward zero into int64 (env_stocktrading_np.py:104); both compares against min_action are strict
(:112, :120) and both min() calls return their first, float32, operand at equality (:114, :124).  The
kernel saturates the float32 product at +-S (include/finenv.h, array-state section, "Action domain");
expectations for actions past S come from the oracle fed `saturated()` actions.  NaN and +-inf actions are
out of scope: the reference's own cast is undefined there.

The cases: `boundary` (k / max_stock and its float32 neighbours around 0, +-min_action, +-max_stock),
`ties` (sales of exactly the holdings, buys of exactly amount // price, on dyadic prices), `beyond`
(scaled magnitudes 2^8 .. S), `past` (products past S, -2^31 among them) and `quotient` (buys of S shares
that a float32 `amount // price` between 2^22 and S cuts short: NumPy's float32 floor division is not the
floor there, and only an action this large lets it bind -- the first run of `beyond` / `past` on the
device found the kernel buying the exact floor instead).

One run shape throughout: E = 130 envs (two full 64-env waves and a 2-lane tail), T = 8 panel rows,
16 steps (two episode ends).  Envs 0..63 start with a float64 amount (what an np.float64 initial_capital
gives the reference), so wave 0 is on the kernel's all-float64 trade loops on every step, the first of an
episode included; the others start on a Python-float or float32 amount and env 70 is fed zero actions, so
wave 1 stays on the tagged loops throughout.  Every event is booked under the form its wave takes
(`steady` / `mixed`, as panel_domain_cases.np_events does); the 2-lane tail is booked under neither."""
import collections
import functools

import numpy as np

F32 = np.float32
E, T = 130, 8
PAD = 3                             # further panel rows, for the windowed form (starts 0 .. PAD)
STEPS = 2 * (T - 1) + 2
IDLE, WAVE = 70, 64
K = 2                               # indicators per ticker
S = (1 << 31) - 128                 # the saturation value: the largest float32 an int32 holds
TURBULENT_ROW = 5                   # of the one case that has a turbulent day (inside every window)
KW = dict(gamma=0.98, buy_cost_pct=0.0012, sell_cost_pct=0.0008)
TAG_PY, TAG_F32, TAG_F64 = 0, 1, 2
assert float(F32(S)) == S and float(np.nextafter(F32(S), F32(np.inf))) == 2.0 ** 31

NS = (1, 5, 30, 32)
# (case, max_stock, min_stock_rate) of the plain form; every N
CONFIGS = [("boundary", 128, 0.1), ("boundary", 128, 0.0), ("boundary", 100, 0.1), ("boundary", 100, 0.0),
           ("boundary", 1e6, 0.1), ("boundary", 1e6, 0.0), ("ties", 128, 0.1), ("beyond", 128, 0.1),
           ("beyond", 1e6, 0.1), ("past", 128, 0.1), ("quotient", 128, 0.1)]
# the further launch forms (windows, history): these cases at max_stock 128, at these N
FORM_CASES, FORM_NS = ("beyond", "past", "ties"), (5, 30)

# Seeds: the first of 0, 1, 2, ... at which the oracle alone reaches every required event of the case
# (tests/test_oracle_stocknp_action_domain.py fails first when one stops doing so).
# key: (case, N, max_stock, min_stock_rate, windowed)
SEEDS = {("beyond", 1, 128, 0.1, False): 2}


def seed_of(case, N, max_stock, rate, windowed=False):
    return SEEDS.get((case, N, max_stock, rate, windowed), 0)


def min_action_of(max_stock, rate):
    return int(max_stock * rate)                                    # :111


def product(actions, max_stock):
    """f32(action) * f32(max_stock), the float32 product the cast sees (:104)."""
    x = np.asarray(actions, F32) * F32(max_stock)
    assert x.dtype == F32
    return x


def scaled(actions, max_stock):
    """trunc(product) as int64 (:104), for products an int64 holds."""
    x = product(actions, max_stock)
    assert (np.abs(x) < F32(2.0 ** 63)).all()
    return np.trunc(x).astype(np.int64)


def is_pow2(max_stock):
    return float(max_stock) == int(max_stock) and int(max_stock) & (int(max_stock) - 1) == 0


def effective(actions, max_stock):
    """The scaled integer the step trades on: the float32 product bounded to [-S, S], then truncated."""
    return np.trunc(np.clip(product(actions, max_stock), F32(-S), F32(S))).astype(np.int64)


def saturated(actions, max_stock):
    """The actions a step that saturates at +-S effectively sees, exact at a power-of-two max_stock."""
    assert is_pow2(max_stock), "exact only for a power-of-two max_stock"
    want = effective(actions, max_stock)
    out = (want / max_stock).astype(F32)
    np.testing.assert_array_equal(scaled(out, max_stock), want)
    return out


def below(v):
    """The largest float32 integer below v."""
    return int(np.nextafter(F32(v), F32(0)))


# ---------------------------------------------------------------- panel and start books
def panel(N, seed, dyadic=False, turbulent=False, rows=T + PAD, cheap0=True):
    """-> price [rows, N] (float32 values), tech [rows, N*K], turbulence [rows].  Price levels from 1e-3
    (ticker 0) to 1e5 (ticker 1) times a 2 % walk, or with `dyadic` powers of two from 2^-10 to 2^16
    that move by a factor of two; no turbulent day unless `turbulent` (then row TURBULENT_ROW).
    cheap0=False: ticker 0 at 10^U(0, 2.5) instead -- where a lone ticker lets 1e2 of cash cut a buy of
    256 shares short and 1e12 pay for S of them."""
    rng = np.random.default_rng(seed)
    if dyadic:
        k = rng.integers(-10, 17, N)
        k[:2] = (-10, 16)[:min(N, 2)]
        price = 2.0 ** (k[None, :] + rng.integers(-1, 2, (rows, N)))
    else:
        level = 10.0 ** rng.uniform(-3, 5, N)
        level[:2] = (1e-3 if cheap0 else 10.0 ** rng.uniform(0, 2.5), 1e5)[:min(N, 2)]
        price = level * np.exp(np.cumsum(rng.normal(0, 0.02, (rows, N)), axis=0))
    price = price.astype(F32).astype(np.float64)
    assert (price > 0).all() and np.isfinite(price).all()
    turb = np.abs(rng.normal(0, 40, rows)).clip(0, 90)
    if turbulent:
        turb[TURBULENT_ROW] = 150.0
    assert int((turb > 99).sum()) == int(turbulent)
    return price, rng.normal(0, 50, (rows, N * K)), turb


def books(N, seed, ties=False):
    """Per-env start state (stocks0 [E, N] f32, amount0 [E], amount0_tag [E]) in four kinds, e % 4:
    0 about 2^30 shares per ticker (float32 no longer holds every integer there; with `ties` about 2^22,
      so that a sale of exactly the holdings is an exact float32 action) and cash 1e12;
    1 a few shares and cash 10^U(2, 5) (env 1: 1e2) -- holdings bind the sells, cash the buys;
    2 about 2^20 shares and cash 10^U(4, 9);   3 up to 300 shares and cash 1e12.
    Tags: float64 in wave 0, Python float / float32 elsewhere (see the module docstring)."""
    rng = np.random.default_rng(seed)
    kind = (np.arange(E) % 4)[:, None]
    top = 22 if ties else 30
    stocks = np.choose(kind, [(1 << top) + rng.integers(0, 1 << 20, (E, N)), rng.integers(0, 40, (E, N)),
                              (1 << 20) + rng.integers(0, 1 << 10, (E, N)), rng.integers(0, 300, (E, N))])
    stocks = stocks.astype(F32)
    assert (stocks == np.round(stocks)).all()
    cash = np.choose(kind[:, 0], [np.full(E, 1e12), 10.0 ** rng.uniform(2, 5, E),
                                  10.0 ** rng.uniform(4, 9, E), np.full(E, 1e12)])
    cash[1] = 1e2
    tag = rng.integers(0, 2, E).astype(np.int32)
    tag[:WAVE] = TAG_F64
    assert tag[IDLE] in (TAG_PY, TAG_F32)
    amount = np.where(tag == TAG_F32, cash.astype(F32), cash).astype(np.float64)
    return stocks, amount, tag


# ---------------------------------------------------------------- (a) boundary
def boundary_values(max_stock, rate):
    """k / max_stock and its two float32 neighbours for k around 0, +-min_action and +-max_stock; +-0.0,
    the smallest normal, a denormal, and values with |a * max_stock| < 1.  At most 64 values: a wave of
    one-ticker envs holds them all."""
    m, M = min_action_of(max_stock, rate), int(max_stock)
    k = sorted({s * (c + d) for s in (1, -1) for c in (0, m, M) for d in (-1, 0, 1)})
    k = np.array(k, np.int64)
    base = (k / max_stock).astype(F32)
    if is_pow2(max_stock):                       # each asks for exactly its integer
        np.testing.assert_array_equal(scaled(base, max_stock), k)
        np.testing.assert_array_equal(product(base, max_stock), k.astype(F32))
    tiny, den = np.finfo(F32).tiny, F32(1e-42)
    sub = F32(1.0) / F32(max_stock)
    under = np.array([sub / 2, -sub / 2, F32(0.999) * sub, -F32(0.999) * sub], F32)
    x = product(under, max_stock)
    assert ((np.abs(x) < 1) & (x != 0)).all()
    extra = np.array([0.0, -0.0, tiny, -tiny, den, -den], F32)
    vals = np.concatenate([base, np.nextafter(base, F32(-np.inf)), np.nextafter(base, F32(np.inf)),
                           extra, under])
    assert len(vals) <= WAVE and np.isfinite(vals).all()
    return vals


def boundary_tiles(max_stock, rate, N, seed, steps=STEPS, envs=E):
    """[steps, envs, N] float32: every step a fresh permutation of boundary_values, repeated over the flat
    tile -- each full 64-env wave holds every value in every step, in other cells each time."""
    vals = boundary_values(max_stock, rate)
    rng = np.random.default_rng(seed)
    out = np.empty((steps, envs, N), F32)
    for s in range(steps):
        out[s] = np.resize(vals[rng.permutation(len(vals))], envs * N).reshape(envs, N)
        for w in range(0, envs - WAVE + 1, WAVE):
            assert np.isin(vals.view(np.uint32), out[s, w:w + WAVE].view(np.uint32)).all()
    return out


# ---------------------------------------------------------------- (c), (d) beyond [-1, 1], past S
def magnitudes_beyond():
    """Scaled magnitudes outside [-1, 1] * max_stock up to the saturation value."""
    return [1 << k for k in range(8, 31)] + [below(S), S]


def big_tiles(signed, max_stock, N, seed, steps=STEPS, envs=E):
    """[steps, envs, N] float32 mixing v / max_stock for v in `signed` (45 %), a few in-range values
    repeated all over the tile (30 %) and uniform(-1, 1) draws.  At a power-of-two max_stock each big
    action asks for exactly its integer; elsewhere the float32 chain rounds and what it asks for is
    `scaled()` of it, kept within +-S."""
    rng = np.random.default_rng(seed)
    signed = np.array(signed, np.float64)
    big = (signed / max_stock).astype(F32)
    if is_pow2(max_stock):
        np.testing.assert_array_equal(product(big, max_stock).astype(np.float64), signed)
    big = big[np.abs(product(big, max_stock)) <= F32(S)] if np.abs(signed).max() <= S else big
    m1 = min_action_of(max_stock, 0.1) + 1
    rep = np.array([-1.0, -0.5, -m1 / max_stock, 0.0, m1 / max_stock, 0.5, 1.0], F32)
    u = rng.random((steps, envs, N))
    out = rng.uniform(-1, 1, (steps, envs, N)).astype(F32)
    out = np.where(u < 0.75, rep[rng.integers(0, len(rep), u.shape)], out)
    out = np.where(u < 0.45, big[rng.integers(0, len(big), u.shape)], out)
    out = out.astype(F32)
    assert np.isfinite(product(out, max_stock)).all()
    return out


def signed_beyond():
    return [s * v for v in magnitudes_beyond() for s in (1, -1)]


def signed_past(max_stock):
    """Products past S: the float32 just above it (2^31: negative, int32's minimum exactly), 2 S, 2^40
    and 3e38."""
    return [s * v for v in (2.0 ** 31, 2.0 * S, 2.0 ** 40, float(F32(3e38))) for s in (1, -1)]


# ---------------------------------------------------------------- (b) ties, scripted on the oracle's state
def floordiv_as_numpy(amount, tag, price):
    """`self.amount // price[index]` as NumPy 2 evaluates it: in float32 unless the amount is a float64."""
    if tag == TAG_F64:
        return float(np.float64(amount) // F32(price))
    return float(F32(amount) // F32(price))


def ties_row(role, turn, amount, tag, stocks, price, draw, max_stock, m):
    """One env's actions [N] on a step of the `ties` script.  role 0: sell exactly the holdings of every
    ticker (-a == stocks[i], both exact float32 below 2^24); role 1: buy exactly amount // price on ticker
    `turn % N` and nothing else, so that no earlier trade of the step moves the cash; other roles: `draw`."""
    N = len(stocks)
    out = np.zeros(N, F32)
    if role == 0:
        ok = (stocks > m) & (stocks < 2 ** 24) & (stocks == np.round(stocks))
        out = np.where(ok, -stocks.astype(np.float64) / max_stock, 0.0).astype(F32)
        np.testing.assert_array_equal(scaled(out, max_stock), np.where(ok, -stocks, 0).astype(np.int64))
    elif role == 1:
        j = turn % N
        q = floordiv_as_numpy(amount, tag, price[j])
        if m < q <= S and float(F32(q)) == q:
            out[j] = F32(q / max_stock)
            assert scaled(out[j], max_stock) == q
    else:
        out = np.asarray(draw, F32).copy()
    return out


def quotient_row(s, e, amount, tag, stocks, price, draw, max_stock):
    """One env's actions [N] on a step of the `quotient` script, for an env whose amount is no float64.
    Even steps: one buy of S shares on ticker (e + s / 2) % N where the float32 `amount // price` lies in
    [2^22, S] -- cash binds, and what NumPy's float32 floor division returns there is bought, floor or not;
    nothing where it lies elsewhere.  Odd steps: sell S of everything held, which the holdings cut short.
    Both trade on float32 operands, so the amount stays a float32 and the next even step is another such
    buy.  Envs with a float64 amount (wave 0) play `draw`."""
    N = len(stocks)
    if tag == TAG_F64:
        return np.asarray(draw, F32).copy()
    out = np.zeros(N, F32)
    if s % 2 == 0:
        j = (e + s // 2) % N
        if 2.0 ** 22 <= floordiv_as_numpy(amount, tag, price[j]) <= S:
            out[j] = F32(S / max_stock)
    else:
        out[stocks > 0] = F32(-S / max_stock)
    assert set(scaled(out, max_stock).tolist()) <= {0, S, -S}
    return out


# ---------------------------------------------------------------- the cases
Case = collections.namedtuple("Case", "name N max_stock rate arrays starts acts signed sat")
# arrays: (price, tech, turb) of T + PAD rows; starts: (stocks0, amount0, tag0); acts [STEPS, E, N] f32 or
# None (scripted); signed: the scaled values the case exists for; sat: expectations on saturated actions


def build(name, N, max_stock=128, rate=0.1, seed=0):
    seed = 1000 * seed + 7 * N + len(name)
    if name == "boundary":
        acts, signed = boundary_tiles(max_stock, rate, N, seed), []
    elif name in ("ties", "quotient"):
        assert is_pow2(max_stock)
        acts, signed = None, []
    elif name == "beyond":
        signed = signed_beyond() if is_pow2(max_stock) else []
        acts = big_tiles(signed_beyond(), max_stock, N, seed)
        assert (np.abs(product(acts, max_stock)) <= F32(S)).all()
    elif name == "past":
        assert is_pow2(max_stock)
        signed = signed_past(max_stock)
        acts = big_tiles(signed, max_stock, N, seed)
        x = product(acts, max_stock)
        for v in signed:
            assert (x == F32(v)).any()
        assert (x == F32(-2.0 ** 31)).any() and np.isfinite(x).all()
    else:
        raise ValueError(name)
    if acts is not None:
        acts[:, IDLE, :] = 0.0
    arrays = panel(N, seed + 1, dyadic=name == "ties", turbulent=name == "beyond",
                   cheap0=N > 1 or name in ("past", "quotient"))
    return Case(name, N, max_stock, rate, arrays, books(N, seed + 2, ties=name == "ties"), acts, signed,
                name == "past")


def window_starts():
    """Per-env windows [s_e, s_e + T) of differing starts inside the T + PAD rows: the envs of a wave are
    on different panel rows at every step."""
    return np.arange(E) % (PAD + 1)


class Twins:
    """One StockNpOracle per distinct window start (every window has T rows, so all envs end together),
    gathered in env order; stepped without auto-reset so that the terminal state can be read."""

    def __init__(self, case, starts_at):
        from oracle.stocknp import StockNpOracle
        self.groups = []
        for s in np.unique(starts_at):
            ks = np.flatnonzero(starts_at == s)
            o = StockNpOracle(*(a[s:s + T] for a in case.arrays), n_envs=len(ks), max_stock=case.max_stock,
                              min_stock_rate=case.rate, **KW)
            o.set_initial(*(x[ks] for x in case.starts))
            self.groups.append((ks, o))
        self.price, self.turb_bool = np.empty((T + PAD, case.N), F32), np.empty(T + PAD, F32)
        for ks, o in self.groups:                  # the oracles' own derived float32 arrays, by panel row
            s = starts_at[ks[0]]
            self.price[s:s + T], self.turb_bool[s:s + T] = o.price, o.turb_bool

    def _gather(self, parts):
        out = np.empty((E,) + parts[0].shape[1:], parts[0].dtype)
        for (ks, _), x in zip(self.groups, parts):
            out[ks] = x
        return out

    def reset(self):
        return self._gather([o.reset() for _, o in self.groups])

    def step(self, a):
        outs = [o.step(a[ks]) for ks, o in self.groups]
        return tuple(self._gather([x[j] for x in outs]) for j in range(3))

    def state(self):
        sts = [o.state() for _, o in self.groups]
        return {k: self._gather([s[k] for s in sts]) for k in sts[0]}


Trace = collections.namedtuple("Trace", "case starts_at acts fed obs0 steps price turb_bool")
# acts: what the env is fed; fed: what the oracle was fed (saturated where case.sat); steps: per step a
# dict of obs / term / rew / done / state (after any reset) / pre / post (before it) / row [E] (panel row
# of the step's prices)


@functools.lru_cache(maxsize=None)
def trace(name, N, max_stock=128, rate=0.1, windowed=False):
    """The oracle's run of a case in the plain (rows [0, T) for every env) or the windowed form."""
    case = build(name, N, max_stock, rate, seed_of(name, N, max_stock, rate, windowed))
    starts_at = window_starts() if windowed else np.zeros(E, np.int64)
    tw = Twins(case, starts_at)
    rng = np.random.default_rng(N)
    m = min_action_of(max_stock, rate)
    obs0 = tw.reset()
    acts = np.zeros((STEPS, E, N), F32) if case.acts is None else case.acts
    steps = []
    for s in range(STEPS):
        pre = tw.state()
        row = starts_at + pre["day"] + 1
        if case.acts is None:
            draws = rng.uniform(-1, 1, (E, N)).astype(F32)
            for e in range(E):
                if e == IDLE:
                    continue
                state = pre["amount"][e], pre["amount_tag"][e], pre["stocks"][e], tw.price[row[e]], draws[e]
                if name == "ties":
                    acts[s, e] = ties_row((e + s) % 4, e + s, *state, max_stock, m)
                else:
                    acts[s, e] = quotient_row(s, e, *state, max_stock)
        fed = saturated(acts[s], max_stock) if case.sat else acts[s]
        obs, rew, done = tw.step(fed)
        assert done.all() or not done.any()
        post = tw.state()
        term = obs
        if done.all():
            obs = tw.reset()
        steps.append(dict(obs=obs, term=term, rew=rew, done=done, state=tw.state(), pre=pre, post=post,
                          row=row, fed=fed))
    assert sum(bool(st["done"].all()) for st in steps) == 2
    assert not acts[:, IDLE].any()
    fed = np.stack([st["fed"] for st in steps])
    return Trace(case, starts_at, acts, fed, obs0, steps, tw.price, tw.turb_bool)


# ---------------------------------------------------------------- event counter
def events(tr):
    """Event counts over a trace, read from the oracle's states alone.  Asserts on the way that the oracle
    trades exactly where the strict compares say (`traded`: the cool-down it zeroes)."""
    case = tr.case
    ms, m = case.max_stock, min_action_of(case.max_stock, case.rate)
    ev = collections.Counter()
    full = E // WAVE * WAVE
    for s, st in enumerate(tr.steps):
        pre, post, row = st["pre"], st["post"], st["row"]
        p = tr.price[row].astype(np.float64)
        calm = (tr.turb_bool[row] == 0.0)[:, None]
        x = product(tr.acts[s], ms).astype(np.float64)
        a = effective(tr.acts[s], ms)
        np.testing.assert_array_equal(scaled(st["fed"], ms), a)        # what the oracle was asked for
        f64 = pre["amount_tag"] == TAG_F64
        where = {"steady": np.zeros((E, 1), bool), "mixed": np.zeros((E, 1), bool)}
        for w in range(0, full, WAVE):
            where["steady"][w:w + WAVE] = f64[w:w + WAVE].all()
            where["mixed"][w:w + WAVE] = not f64[w:w + WAVE].all()
        s0, s1 = pre["stocks"].astype(np.float64), post["stocks"].astype(np.float64)
        held = s0 > 0
        sells, buys = calm & (a < -m), calm & (a > m)
        traded = post["cool_down"] == 0
        np.testing.assert_array_equal(traded, sells | buys | ~calm, err_msg=f"step {s}")
        assert (post["cool_down"][~traded] == pre["cool_down"][~traded] + 1).all()
        assert (s1[~traded] == s0[~traded]).all()
        assert (s1[~calm[:, 0]] == 0).all()
        # cash only falls during the buys, which follow the sells: it was at least the final amount
        rich = post["amount"][:, None] // p >= np.abs(a) + 1
        whole = x == np.trunc(x)
        frac = (np.abs(x) > m) & (np.abs(x) < m + 1)
        can_buy, can_sell = calm & rich, calm & held
        after_buy = (s0 + a).astype(F32).astype(np.float64)          # the holdings, were the action to bind
        after_sell = after_buy
        q32 = (pre["amount"].astype(F32)[:, None] // p.astype(F32)).astype(np.float64)
        q = np.where(f64[:, None], pre["amount"][:, None] // p, q32)
        alone = (tr.acts[s] != 0).sum(1, keepdims=True) == 1
        sell_tie = sells & (-a == s0) & held
        buy_tie = buys & (a == q) & alone
        assert (s1[sell_tie] == 0).all()
        np.testing.assert_array_equal(s1[buy_tie], after_buy[buy_tie])
        only_ties = sell_tie.any(1) & ~((sells | buys) & ~sell_tie).any(1)
        t0 = pre["amount_tag"]
        assert (post["amount_tag"][only_ties] == np.where(t0 == TAG_PY, TAG_F32, t0)[only_ties]).all()
        past = np.abs(x) > S
        # float32 `amount // price` from 2^22 on is no longer the floor (two float32 roundings in
        # npy_floor_dividef); where it binds, the reference buys that many.  Read on the env's first trade of
        # the step, where the amount is still the pre-step one.
        first = buys & ~sells.any(1, keepdims=True) & (np.cumsum(buys, axis=1) == 1)
        with np.errstate(over="ignore"):
            exact = np.floor_divide(pre["amount"].astype(F32).astype(np.float64)[:, None], p)
        odd = first & ~f64[:, None] & (q32 != exact) & (a >= np.minimum(q32, exact)) & (np.abs(exact) < 2.0 ** 40)
        np.testing.assert_array_equal(s1[odd], (s0 + q32).astype(F32).astype(np.float64)[odd])
        ev["float32_quotient_is_not_the_floor_mixed"] += int((odd & where["mixed"]).sum())
        for wname, wm in where.items():
            def add(key, mask):
                ev[f"{key}_{wname}"] += int((mask & wm).sum())
            ev[f"{wname}_wave_steps"] += int(wm[:full:WAVE].sum())
            add("at_plus_min", can_buy & (x == m) & ~traded)
            add("at_minus_min", can_sell & (x == -m) & ~traded)
            add("above_plus_min", can_buy & (x == m + 1) & traded)
            add("below_minus_min", can_sell & (x == -(m + 1)) & traded)
            add("fraction_truncated", np.where(x < 0, can_sell, can_buy) & frac & ~whole & ~traded)
            add("sell_tie", sell_tie)
            add("buy_tie", buy_tie)
            add("sell_tie_tag_checked", sell_tie & only_ties[:, None])
            add("sell_tie_stays_float32", sell_tie & only_ties[:, None] & (t0 != TAG_F64)[:, None])
            big = np.abs(a) > ms
            add("buy_action_binds", buys & big & (s1 == after_buy))
            add("buy_cash_binds", buys & big & (s1 < after_buy))
            add("sell_action_binds", sells & big & held & (s0 >= -a) & (s1 == after_sell))
            add("sell_holdings_bind", sells & big & held & (s0 < -a) & (s1 == 0))
            add("turbulent_env_steps", ~calm & held)
            add("past_buy_is_S", past & buys & (a == S) & (s1 == after_buy) & (s1 > s0))
            add("past_sell", past & sells & held & (a == -S))
            add("int_min_sell", (x == -2.0 ** 31) & sells & held)
            for v in case.signed:
                if abs(v) > S:
                    continue
                mv = (buys if v > 0 else sells & held) & (a == int(v))
                bound = (s1 == after_buy) if v > 0 else (s0 >= -a) & (s1 == after_sell)
                short = (s1 < after_buy) if v > 0 else (s0 < -a) & (s1 == 0)
                add(f"binds|{int(v)}", mv & bound)
                add(f"short|{int(v)}", mv & short)
    return ev


def _need(tr, ev, *keys, forms=("steady", "mixed")):
    c = tr.case
    for k in keys:
        for f in forms:
            assert ev[f"{k}_{f}"] > 0, (f"{c.name} N={c.N} max_stock={c.max_stock:g} rate={c.rate:g}: event "
                                        f"{k}_{f} never occurs")


def assert_both_bind(tr, ev):
    """For every scaled magnitude of the case: somewhere the trade is the action itself and somewhere
    holdings or cash cut it short (in a wave of either form).  Sells of more than the largest start
    book (2^30 + 2^20 shares) can only ever be cut short."""
    for v in tr.case.signed:
        if abs(v) > S:
            continue
        n = {k: ev[f"{k}|{int(v)}_steady"] + ev[f"{k}|{int(v)}_mixed"] for k in ("binds", "short")}
        assert n["short"] > 0, f"scaled action {v:g}: holdings / cash never bind"
        if v > 0 or -v <= 1 << 30:
            assert n["binds"] > 0, f"scaled action {v:g} never binds"


def require_boundary(tr, ev):
    _need(tr, ev, "at_plus_min", "at_minus_min", "above_plus_min", "below_minus_min", "fraction_truncated")


def require_ties(tr, ev):
    _need(tr, ev, "sell_tie", "buy_tie", "sell_tie_tag_checked")
    _need(tr, ev, "sell_tie_stays_float32", forms=("mixed",))


def require_beyond(tr, ev):
    _need(tr, ev, "buy_action_binds", "buy_cash_binds", "sell_action_binds", "sell_holdings_bind",
          "turbulent_env_steps")
    assert_both_bind(tr, ev)


def require_past(tr, ev):
    _need(tr, ev, "past_buy_is_S", "past_sell", "int_min_sell")


def require_quotient(tr, ev):
    """Only a wave on the tagged loops divides in float32: there is no steady form of this event."""
    _need(tr, ev, "float32_quotient_is_not_the_floor", forms=("mixed",))
    assert ev["float32_quotient_is_not_the_floor_mixed"] >= 8, dict(ev)


REQUIRE = dict(boundary=require_boundary, ties=require_ties, beyond=require_beyond, past=require_past,
               quotient=require_quotient)


def require_events(tr, ev=None):
    """What keeps a parametrised case from passing vacuously."""
    ev = events(tr) if ev is None else ev
    assert ev["steady_wave_steps"] >= STEPS and ev["mixed_wave_steps"] >= STEPS, dict(ev)
    REQUIRE[tr.case.name](tr, ev)
    return ev


# ---------------------------------------------------------------- one reference env (tests/golden/make_golden.py)
FIX_T, FIX_N, FIX_MAX_STOCK = 24, 5, 128
FIX_STEPS = 2 * (FIX_T - 1) + 2
FIXTURE_ENV = dict(boundary=3, ties=2, beyond=0)        # the env whose book the fixture's one env starts on


def fixture(name, seed):
    """One env of a case on a longer panel, for the unmodified reference: constructor arguments and
    script(step, amount, tag, stocks, price_row) -> [N] f32.  `beyond` asks for -+2^40 shares on step 1:
    int64 holds that product, the reference trades min(stocks, 2^40) and min(amount // price, 2^40) -- all
    the holdings and all the cash buys, both below S, so a step that saturates at S trades the same and
    the fixture also serves the tests that replay every stocknp_*.npz on the device."""
    N, ms, e = FIX_N, FIX_MAX_STOCK, FIXTURE_ENV[name]
    m = min_action_of(ms, 0.1)
    price, tech, turb = panel(N, seed, dyadic=name == "ties", turbulent=name == "beyond", rows=FIX_T)
    stocks0, amount0, _ = books(N, seed + 1, ties=name == "ties")
    rng = np.random.default_rng(seed + 2)
    if name == "boundary":
        acts = boundary_tiles(ms, 0.1, N, seed + 3, steps=1, envs=FIX_STEPS)[0]
    elif name == "beyond":
        acts = big_tiles(signed_beyond(), ms, N, seed + 3, steps=1, envs=FIX_STEPS)[0]
        every = np.array(signed_beyond(), np.float64)                # each magnitude at least once
        acts.reshape(-1)[rng.permutation(acts.size)[:len(every)]] = (every / ms).astype(F32)
        acts[1, :2] = F32(-2.0 ** 40 / ms), F32(2.0 ** 40 / ms)     # (ticker 1, at 1e5: 1e12 buys ~1e7 < S)
        assert scaled(acts[1, :2], ms).tolist() == [-(1 << 40), 1 << 40]
    else:
        acts = rng.uniform(-1, 1, (FIX_STEPS, N)).astype(F32)

    def script(s, amount, tag, stocks, price_row):
        if name != "ties":
            return acts[s].copy()
        return ties_row((e + s) % 4, e + s, amount, tag, np.asarray(stocks, F32), price_row, acts[s], ms, m)

    return dict(price=price, tech=tech, turb=turb, initial_capital=float(amount0[e]),
                initial_stocks=stocks0[e].copy(), max_stock=float(ms), script=script, T=FIX_T, N=N, K=K,
                S=FIX_STEPS, **KW)
