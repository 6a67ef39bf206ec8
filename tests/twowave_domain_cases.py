"""Market panels and action scripts for the cash-penalty and stop-loss envs outside what every other
test of them draws (closes 50 * exp(random walk), actions uniform(-1, 1): no compare of the trading rule
ever sees equality there, no close is zero, `np.floor_divide(a, close)` equals `floor(a / close)`, and no
price is far from 50).  Shared by tests/test_gpu_{cashpenalty,stoploss}_panel_domain.py (HIP kernels vs
the oracles) and tests/test_oracle_twowave_domain.py (the oracles alone).  Everything but the two
replay_* functions at the end is host-side NumPy.  Each builder comes with a counter that reads, from
oracle states and outputs alone, how often each event the case exists for occurred, and a
require_*_events() with the events a case must reach (include/finenv.h, "Panel domain" of the two envs):
a case that does not hold what its name says fails instead of testing less.

One run shape for every case: E envs (two full waves and a 2-lane tail: three blocks of the two-wave
kernels), T panel rows, STEPS steps, per-env starts in [0, T // 2) redrawn every step, auto-reset.

Out of scope: NaN / infinite prices, negative closes, actions outside [-1, 1]."""
import collections
import functools

import numpy as np

F32 = np.float32
E, T, STEPS = 130, 24, 36
# (N, C): D = 1 + N * (1 + C) columns.  D <= 64: one chunk; 64 < D <= 320: two chunks (at N = 17 the
# streamer's pass 3 holds exactly one asset); D > 320: the one-wave kernel
SHAPES = ((5, 2), (1, 0), (17, 3), (30, 5), (30, 10))
WINDOW_SHAPE = (17, 3)
KINDS = ("cashpenalty", "stoploss")

Case = collections.namedtuple("Case", "name close info turb kw sl_kw script")
# close [T, N] f64, info [T, N, C] f64, turb [T] f64; kw: the env arguments both kinds take, sl_kw: the
# stop-loss env's two more; script(s, first) -> actions [E, N] f32 of step s, `first` [E] bool being the
# envs on the first step of an episode (date_index == start).  A script draws from its own generator:
# call it once per step, in order.


def env_kwargs(kind, case):
    return dict(case.kw, **(case.sl_kw if kind == "stoploss" else {}))


def _info(rng, N, C):
    return rng.normal(0, 10, (T, N, C))


def _kw(hmax, initial_amount, discrete, inc, patient, thr, buy=0.002, sell=0.001, prop=0.15):
    return dict(hmax=hmax, initial_amount=initial_amount, discrete_actions=bool(discrete),
                shares_increment=int(inc), patient=bool(patient), turbulence_threshold=thr,
                buy_cost_pct=buy, sell_cost_pct=sell, cash_penalty_proportion=prop)


# ---------------------------------------------------------------- tick_prices
TICK_HMAX = 2 ** 15


def tick_prices(N, C, seed, *, inc=1, patient=False, turbulence=False):
    """Closes on a per-asset grid from {0.01, 0.05, 0.1, 0.25} (the double nearest to the decimal, as a
    price file parses), levels 0.05 .. 300; hmax 2^15 and actions j / 2^15, so every request is a whole
    number of dollars -- where a // close and floor(a / close) part ways (3.0 // 0.1 == 29).  Discrete
    actions only."""
    rng = np.random.default_rng(seed)
    grid = rng.choice([0.01, 0.05, 0.1, 0.25], N)
    level = np.exp(rng.uniform(np.log(0.05), np.log(300.0), N))
    level[:2] = (0.05, 300.0)[:min(N, 2)]
    walk = level * np.exp(np.cumsum(rng.normal(0, 0.03, (T, N)), axis=0))
    ticks = np.maximum(np.rint(np.clip(walk, 0.05, 300.0) / grid), 1.0)
    close = np.round(ticks * grid, 2)
    assert close.min() >= 0.05 - 1e-12 and close.max() <= 300.0 + 1e-9
    turb = rng.choice([0.0, 16.0, 32.0, 48.0], T, p=[0.4, 0.3, 0.15, 0.15])
    arng = np.random.default_rng(seed + 1)

    def script(s, first):
        j = arng.integers(-TICK_HMAX, TICK_HMAX + 1, (E, N))
        j[arng.random((E, N)) < 0.05] = 0
        j[::4] = np.abs(j[::4]) // 16            # every fourth env only buys, small: it keeps cash and shares
        j[1::4] //= 8                            # (and these trade small both ways: sells that are not clipped)
        return (j / float(TICK_HMAX)).astype(F32)

    kw = _kw(TICK_HMAX, 1e6, True, inc, patient, 32.0 if turbulence else None)
    return Case("tick_prices", close, _info(rng, N, C), turb, kw,
                dict(stoploss_penalty=0.93, profit_loss_ratio=1.5), script)


# ---------------------------------------------------------------- price_scales
def price_scales(N, C, seed, *, initial_amount=1e6, discrete=True, patient=False, turbulence=False):
    """Per-asset level 10^U(-8, 5.48) (both ends present) times a 2 % walk, fp64, strictly positive;
    hmax = max(initial_amount, 2^22); actions are scaled per asset so that |act * hmax / close| stays
    at about 2^49 on the cheapest row of the asset (the stated domain is 2^50) and spread over ten decades,
    so that small buys fill as asked and large ones run the env out of cash."""
    rng = np.random.default_rng(seed)
    hi = np.log10(3e5)
    level = 10.0 ** rng.uniform(-8.0, hi, N)
    level[:2] = (1e-8, 3e5)[:min(N, 2)]
    close = level * np.exp(np.cumsum(rng.normal(0, 0.02, (T, N)), axis=0))
    assert close.min() > 0.0
    hmax = float(max(initial_amount, 2 ** 22))
    cap = np.minimum(1.0, 2.0 ** 49 * close.min(0) / hmax)
    turb = rng.choice([0.0, 16.0, 32.0, 48.0], T, p=[0.4, 0.3, 0.15, 0.15])
    arng = np.random.default_rng(seed + 1)

    def script(s, first):
        mag = 10.0 ** arng.uniform(-3, 0, (E, N)) * 10.0 ** arng.uniform(-5, 0, (E, 1))
        mag[arng.random((E, N)) < 0.1] = 1.0
        mag[::4] = np.minimum(mag[::4], 10.0 ** arng.uniform(-8, -4, (len(mag[::4]), 1)))
        sign = np.where(arng.random((E, N)) < 0.5, -1.0, 1.0)
        a = (sign * mag * cap).astype(F32)
        return np.where(np.abs(a.astype(np.float64)) > cap, np.nextafter(a, F32(0)), a).astype(F32)

    kw = _kw(hmax, initial_amount, discrete, 1, patient, 32.0 if turbulence else None)
    return Case("price_scales", close, _info(rng, N, C), turb, kw,
                dict(stoploss_penalty=0.93, profit_loss_ratio=1.5), script)


# ---------------------------------------------------------------- dyadic_ties
DY_INIT = 2.0 ** 20
GROUPS = {"armed": 1, "short": 2, "quarter": 3}          # e % 16 of the scripted envs


def _dyadic_panel(rng, N):
    k = rng.integers(2, 9, N) + np.cumsum(rng.choice([-2, -1, 0, 1], (T, N), p=[0.1, 0.2, 0.3, 0.4]), axis=0)
    return 2.0 ** k, rng.choice([0.0, 16.0, 32.0, 48.0], T, p=[0.4, 0.3, 0.15, 0.15])


def dyadic_ties(N, C, seed, *, scripted=False, costs=False, discrete=False, patient=False,
                turbulence=True, _zero_frac=0.0):
    """Closes 2^k on a walk with steps in {-2, -1, 0, +1}; initial_amount 2^20, stoploss_penalty 0.5,
    profit_loss_ratio 2, cash_penalty_proportion 0.25, costs 0 or 2^-8, turbulence rows from
    {0, 16, 32, 48} against threshold 32, actions on the j / 16 grid (30 % zero, more of them from eight
    assets on; every fourth env buy-only): every product, sum and difference of the rule is exact, so its
    compares meet equality.
    scripted: hmax = initial_amount, zero costs, and three groups of envs (e % 16 == 1, 2, 3) whose first
    action of every episode is 0.5 / 1.0 / 0.75 on one asset and zero afterwards --
      armed:   cash becomes exactly stoploss_penalty * initial_amount, and stays: a later fall of the asset
               below half its buy price forces the sale only under `>=` (:353);
      short:   spend equals cash exactly; `>` (:372 / :333) lets the episode go on with cash 0.0;
      quarter: cash is a quarter of the total while the price holds: `total * proportion == cash` in the reward."""
    rng = np.random.default_rng(seed)
    close, turb = _dyadic_panel(rng, N)
    if _zero_frac:
        close = _with_zeros(rng, close, _zero_frac)
    assert _zero_frac or close.min() > 0.0
    hmax = DY_INIT if scripted else 2.0 ** 18
    cost = 2.0 ** -8 if (costs and not scripted) else 0.0
    arng = np.random.default_rng(seed + 1)
    active = min(0.7, 3.5 / N)                       # (so that a wide env does not run short on its first step)
    grp = np.arange(E) % 16
    asset = (np.arange(E) // 16) % N
    amount = {GROUPS["armed"]: 0.5, GROUPS["short"]: 1.0, GROUPS["quarter"]: 0.75}

    def script(s, first):
        j = arng.integers(-16, 17, (E, N))
        if scripted:
            j = np.where(arng.random((E, N)) < 0.5, j // 8, 0)       # (hmax is the whole cash here)
        j[arng.random((E, N)) >= active] = 0
        j[::4] = np.abs(j[::4])
        a = (j / 16.0).astype(F32)
        if scripted:
            for g, amt in amount.items():
                m = grp == g
                a[m] = 0.0
                mf = m & first
                a[mf, asset[mf]] = amt
        return a

    kw = _kw(hmax, DY_INIT, discrete, 1, patient, 32.0 if turbulence else None, buy=cost, sell=cost,
             prop=0.25)
    return Case("dyadic_ties", close, _info(rng, N, C), turb, kw,
                dict(stoploss_penalty=0.5, profit_loss_ratio=2), script)


# ---------------------------------------------------------------- zero_closes (stop-loss only)
def _with_zeros(rng, close, frac):
    close = close.copy()
    close[rng.random(close.shape) < frac] = 0.0
    close[0, 0] = 0.0                                # row 0 is no exception
    return close


def zero_closes(N, C, seed, *, dyadic=False, discrete=False, patient=False, turbulence=True):
    """A dyadic_ties panel or a 5 % random walk around 50 with ~8 % of the closes set to 0.0, the
    reference's "missing data" (:326, :335, :345), row 0 included.  Stop-loss only: the cash-penalty
    reference divides by such a close unguarded."""
    if dyadic:
        c = dyadic_ties(N, C, seed, costs=True, discrete=discrete, patient=patient,
                        turbulence=turbulence, _zero_frac=0.08)
        return c._replace(name="zero_closes")
    rng = np.random.default_rng(seed)
    close = _with_zeros(rng, 50 * np.exp(np.cumsum(rng.normal(0, 0.05, (T, N)), axis=0)), 0.08)
    turb = np.abs(rng.normal(0, 30, T))
    arng = np.random.default_rng(seed + 1)

    def script(s, first):
        a = arng.uniform(-1, 1, (E, N)).astype(F32)
        a[::4] *= F32(0.02)                          # every fourth env trades small and keeps its positions
        return a

    kw = _kw(60_000, 5e5, discrete, 3, patient, 40.0 if turbulence else None)
    return Case("zero_closes", close, _info(rng, N, C), turb, kw,
                dict(stoploss_penalty=0.93, profit_loss_ratio=1.5), script)


BUILDERS = {"tick_prices": tick_prices, "price_scales": price_scales, "dyadic_ties": dyadic_ties,
            "zero_closes": zero_closes}


# ---------------------------------------------------------------- the parametrised cases
def cases(kind):
    """[(id, builder name, (N, C), seed, builder arguments)]: every launch form for every builder, both
    action forms where the builder allows, patient and turbulence on and off."""
    out = []
    sl = kind == "stoploss"
    for i, (N, C) in enumerate(SHAPES):
        b = [bool(i >> k & 1) for k in range(3)]
        out.append(("tick_prices", (N, C), dict(inc=1 if i % 2 else 3, patient=b[1], turbulence=b[0])))
        if N in (5, 17):
            out.append(("tick_prices", (N, C), dict(inc=3 if i % 2 else 1, patient=not b[1],
                                                    turbulence=not b[0])))
        for disc in (True, False):
            # (one asset: it is the cheapest one, whose action cap keeps an env of 1e9 from ever running short)
            out.append(("price_scales", (N, C), dict(initial_amount=(1e2, 1e6, 1e9)[(i + disc) % (3 if N > 1 else 2)],
                                                     discrete=disc, patient=b[0] ^ disc,
                                                     turbulence=b[1] ^ disc)))
        out.append(("dyadic_ties", (N, C), dict(scripted=True, discrete=b[0], patient=False,
                                                turbulence=b[1])))
        if sl or N in (5, 30):
            out.append(("dyadic_ties", (N, C), dict(scripted=False, costs=b[0], discrete=not b[0],
                                                    patient=b[1], turbulence=True)))
        if sl:
            out.append(("zero_closes", (N, C), dict(dyadic=True, discrete=b[0], patient=b[1],
                                                    turbulence=True)))
            out.append(("zero_closes", (N, C), dict(dyadic=False, discrete=not b[0], patient=not b[1],
                                                    turbulence=not b[2])))
    return out


def case_id(name, shape, args):
    parts = [f"{name}-n{shape[0]}c{shape[1]}"]
    for k, v in sorted(args.items()):
        if v is True:
            parts.append(k)
        elif v is not False:
            parts.append(f"{k}{v:g}")
    return "-".join(parts)


def window_cases(kind):
    """One windowed run per kind and builder, at WINDOW_SHAPE."""
    out = [("tick_prices", WINDOW_SHAPE, dict(inc=3, turbulence=True)),
           ("price_scales", WINDOW_SHAPE, dict(initial_amount=1e6, discrete=True)),
           ("dyadic_ties", WINDOW_SHAPE, dict(scripted=True, turbulence=True))]
    if kind == "stoploss":
        out.append(("zero_closes", WINDOW_SHAPE, dict(dyadic=True, discrete=True)))
    return out


# Seeds: the first of 0, 1, 2, ... at which the oracle alone reaches every required event of the case
# (tests/test_oracle_twowave_domain.py fails first when one stops doing so).
SEEDS = {("stoploss", "zero_closes-n1c0-discrete-dyadic-turbulence", False): 1}


def seed_of(kind, name, shape, args, windowed=False):
    return SEEDS.get((kind, case_id(name, shape, args), windowed), 0)


def build(kind, name, shape, args, windowed=False):
    return BUILDERS[name](shape[0], shape[1], 1000 + seed_of(kind, name, shape, args, windowed), **args)


# ---------------------------------------------------------------- oracle trace
def classes(kind):
    from twowave_windows_cases import classes as c
    return c(kind)


def _copy(st):
    return {k: v.copy() for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def _trace(kind, name, shape, args_items):
    args = dict(args_items)
    case = build(kind, name, shape, args)
    orc = classes(kind)[2](case.close, case.info, case.turb, n_envs=E, **env_kwargs(kind, case))
    rng = np.random.default_rng(7)
    starts0 = rng.integers(0, T // 2, E).astype(np.int32)
    obs0 = orc.reset(starts0)
    steps = []
    for s in range(STEPS):
        pre = _copy(orc.state())
        a = case.script(s, pre["date_index"] == pre["start"])
        starts = rng.integers(0, T // 2, E).astype(np.int32)
        obs, rew, done, term = orc.vec_step(a, starts)
        steps.append(dict(a=a, starts=starts, obs=obs, rew=rew, done=done, term=term, pre=pre,
                          post=_copy(orc.state())))
    for st in steps:                                 # shared among tests: nobody writes to it
        for v in list(st.values()) + list(st["pre"].values()) + list(st["post"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return case, starts0, obs0, steps


def trace(kind, name, shape, args):
    """-> case, starts0 [E], obs0 [E, D], steps: per step the actions and starts fed, the oracle's
    outputs, and its state() before (`pre`) and after (`post`, after any auto-reset) the step.
    Computed once per case and process."""
    return _trace(kind, name, tuple(shape), tuple(sorted(args.items())))


# ---------------------------------------------------------------- event counters
def _increment(q, inc):
    """:338-343 on integer-valued float64."""
    q = np.asarray(q, np.float64)
    return np.where(q >= 0, np.floor_divide(q, inc) * inc, np.floor_divide(q + inc, inc) * inc)


def events(kind, case, steps, end=None):
    """Counts per event over `steps` (dicts with a, done, pre, post as trace() gives them; date_index in
    panel rows).  end [E]: the row after each env's episode window (default: the panel's).  Asserts on the
    way that the oracle treats each such cell as the panel domain says."""
    ev = collections.Counter()
    kw, sl = case.kw, kind == "stoploss"
    disc, inc, thr = kw["discrete_actions"], kw["shares_increment"], kw["turbulence_threshold"]
    slp = case.sl_kw["stoploss_penalty"]
    end = np.full(E, len(case.close)) if end is None else np.asarray(end)
    with np.errstate(all="ignore"):
        for s, st in enumerate(steps):
            pre, post, done = st["pre"], st["post"], st["done"]
            di = pre["date_index"]
            live = di < end - 1
            go = (live & ~done)[:, None]                        # the step was applied: post is its result
            cl = case.close[di]                                 # [E, N]
            h = pre["holdings"]
            new = post["holdings"]
            got = new - h
            coh = pre["coh"]
            a = (np.asarray(st["a"], F32) * F32(kw["hmax"])).astype(np.float64)
            turb = (pre["turbulence"] >= thr) & live if thr is not None else np.zeros(E, bool)
            calm = (live & ~turb)[:, None]
            pos, zero = cl > 0.0, cl == 0.0
            if sl:
                armed = coh >= slp * kw["initial_amount"]
                cd = cl - slp * pre["avg_buy_price"]
                forced = armed[:, None] & (cd < 0) & live[:, None]
            else:
                assert pos.all()
                armed, cd, forced = np.zeros(E, bool), np.ones_like(cl), np.zeros_like(pos)
            free = calm & ~forced & pos                          # the action decides the transaction
            q_np = np.floor_divide(a, np.where(pos, cl, 1.0))
            q_fl = np.floor(a / np.where(pos, cl, 1.0))
            want = _increment(q_np, inc) if disc else a / np.where(pos, cl, 1.0)
            assert (np.abs(a[pos & live[:, None]] / cl[pos & live[:, None]]) < 2.0 ** 50).all()
            # a cash shortage of a patient env cancels its buys: such a step leaves every buy unfilled
            cancelled = (go[:, 0] & ((want > 0) & free).any(1) & ~((got > 0).any(1)))[:, None] \
                if kw["patient"] else np.zeros((E, 1), bool)

            # ---- tick_prices: the two roundings give different transactions, and nothing clips them
            if disc:
                other = _increment(q_fl, inc)
                differ = free & go & (want != other) & (want >= -h) & (other >= -h)
                m = differ & (want > 0) & ~cancelled
                np.testing.assert_array_equal(new[m], (h + want)[m], err_msg=f"step {s}")
                ev["buy_roundings_differ"] += int(m.sum())
                m = differ & (want < 0) & (other < 0)
                np.testing.assert_array_equal(new[m], (h + want)[m], err_msg=f"step {s}")
                ev["sell_roundings_differ"] += int(m.sum())
                big = free & (np.abs(q_np) > 2.0 ** 40)
                ev["quotient_over_2p40"] += int(big.sum())
                ev["quotient_over_2p40_applied"] += int((big & go & ~cancelled & (want >= -h)).sum())
                ev["max_abs_quotient_log2"] = max(ev["max_abs_quotient_log2"], int(np.log2(
                    max(float(np.abs(q_np[free]).max()) if free.any() else 1.0, 1.0))))

            # ---- price_scales
            m = free & go & (want > 0) & ~cancelled
            np.testing.assert_array_equal(new[m], (h + want)[m], err_msg=f"step {s}")
            ev["buy_action_binds"] += int(m.sum())
            short = live & (done | cancelled[:, 0])
            ev["cash_shortage_steps"] += int(short.sum())
            m = free & go & (want < -h) & (h > 0)
            assert (post["holdings"][m] == 0).all()
            ev["sell_holdings_bind"] += int(m.sum())

            # ---- ties
            held = (h > 0).any(1)
            if thr is not None:
                at = (pre["turbulence"] == thr) & live & held
                ev["turbulence_at_threshold_with_holdings"] += int(at.sum())
            tie = live & (coh > 0) & ~done & (post["coh"] == 0.0) & (got > 0).any(1)
            ev["spend_equals_cash_goes_on"] += int(tie.sum())
            lt, lc = post["logged_total"], post["logged_cash"]
            ev["reward_cash_penalty_tie"] += int((live & held & (lt * kw["cash_penalty_proportion"] == lc)).sum())
            if sl:
                hl = (h > 0) & live[:, None] & pos
                arm = armed[:, None] & hl
                ev["armed_closing_diff_zero"] += int((arm & (cd == 0)).sum())
                m = arm & (cd == 0) & calm & go & ~((want < 0))
                assert (got[m] >= 0).all()                       # cd == 0 forces no sale
                ev["armed_closing_diff_negative"] += int((arm & (cd < 0)).sum())
                m = arm & (cd < 0) & go
                assert (new[m] == 0).all(), f"step {s}"
                at_arm = live & (coh == slp * kw["initial_amount"])
                ev["cash_at_arming_level"] += int(at_arm.sum())
                ev["cash_at_arming_level_forced_sale"] += int((at_arm[:, None] & hl & (cd < 0) & go).sum())
                sold = go & (got < 0) & pos
                abp = pre["avg_buy_price"]
                m = sold & (cl == abp)
                assert (post["profit_sell_diff_avg_buy"][m] == 0).all()      # no profit at the buy price
                ev["sale_at_avg_buy_price"] += int(m.sum())
                ev["sale_above_avg_buy_price"] += int((sold & (cl > abp)).sum())

                # ---- zero closes: 0 means missing; nothing trades there, nothing is counted
                # (but for the stop-loss of an armed env, which gives a held asset away at 0.0: :350-357 look at
                #  no price guard, and 0 - stoploss_penalty * avg_buy_price < 0)
                hz = zero & live[:, None]
                m = hz & go & forced & (h > 0)
                assert (new[m] == 0).all() and (post["avg_buy_price"][m] == 0).all()
                ev["stop_loss_sale_at_zero"] += int(m.sum())
                m = hz & go & ~forced
                assert (got[m] == 0).all()
                ev["buy_request_at_zero"] += int((m & calm & (a > 0)).sum())
                ev["sell_request_at_zero_held"] += int((m & calm & (a < 0) & (h > 0)).sum())
                ev["held_zero_priced_through_step"] += int((m & (h > 0)).sum())
                ev["turbulent_step_keeps_zero_priced"] += int(
                    (turb & go[:, 0] & (zero & (h > 0)).any(1) & (pos & (h > 0)).any(1)).sum())
                g1 = go[:, 0] & bool((case.close == 0).any())
                np.testing.assert_array_equal(post["actual_num_trades"][g1], (got[g1] != 0).sum(1),
                                              err_msg=f"step {s}")
    return ev


def _need(name, ev, keys):
    for k in keys:
        assert ev[k] > 0, f"{name}: event {k} never occurs ({dict(ev)})"


def require_tick_events(kind, case, ev):
    _need(case.name, ev, ("buy_roundings_differ", "sell_roundings_differ"))


def require_scale_events(kind, case, ev):
    _need(case.name, ev, ("buy_action_binds", "cash_shortage_steps", "sell_holdings_bind"))
    if case.kw["discrete_actions"]:
        _need(case.name, ev, ("quotient_over_2p40",))
        assert ev["max_abs_quotient_log2"] < 50
        if case.kw["initial_amount"] >= 1e6:      # (2^40 shares of the cheapest asset cost ~ $ 11 000)
            _need(case.name, ev, ("quotient_over_2p40_applied",))


def require_tie_events(kind, case, ev):
    scripted = case.kw["hmax"] == DY_INIT
    keys = []
    if case.kw["turbulence_threshold"] is not None:
        keys.append("turbulence_at_threshold_with_holdings")
    if scripted:
        keys += ["spend_equals_cash_goes_on", "reward_cash_penalty_tie"]
    if kind == "stoploss":
        keys += ["armed_closing_diff_zero", "armed_closing_diff_negative", "sale_at_avg_buy_price",
                 "sale_above_avg_buy_price"]
        if scripted:
            keys += ["cash_at_arming_level", "cash_at_arming_level_forced_sale"]
    _need(case.name, ev, keys)


def require_zero_events(kind, case, ev):
    assert kind == "stoploss" and (case.close == 0).any() and case.close[0, 0] == 0.0
    keys = ["buy_request_at_zero", "sell_request_at_zero_held", "held_zero_priced_through_step",
            "stop_loss_sale_at_zero"]
    if case.kw["turbulence_threshold"] is not None and case.close.shape[1] > 1:
        keys.append("turbulent_step_keeps_zero_priced")
    _need(case.name, ev, keys)


REQUIRE = {"tick_prices": require_tick_events, "price_scales": require_scale_events,
           "dyadic_ties": require_tie_events, "zero_closes": require_zero_events}


def require_events(kind, case, ev):
    REQUIRE[case.name](kind, case, ev)


# ---------------------------------------------------------------- windowed twins (one oracle per env)
def window_script(seed=11):
    """Per-env windows [s, t) of at least 8 rows inside the panel, and per-step offsets in [0, 4)."""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, 8, E).astype(np.int64)
    end = (start + rng.integers(8, T - 7 + 1, E)).astype(np.int64)
    assert (end <= T).all()
    return start, end, rng


def window_trace(kind, name, shape, args, on_step=None):
    """The case on per-env windows, driven through Twins (tests/twowave_windows_cases.py).  on_step(s, a,
    offsets, ref, twins), if given, is called after every step with the twins' outputs; offsets0 / obs0
    go to on_step(-1, None, offsets0, obs0, twins).  -> case, steps (for events()), end [E]."""
    from twowave_windows_cases import Twins
    case = build(kind, name, shape, args, windowed=True)
    start, end, rng = window_script()
    tw = Twins(kind, dict(E=E), case.close, case.info, case.turb, start, end, kw=env_kwargs(kind, case))
    off = rng.integers(0, 4, E).astype(np.int32)
    obs0 = tw.reset(off)
    if on_step:
        on_step(-1, None, off, obs0, tw)
    steps = []
    for s in range(STEPS):
        pre = _copy(tw.state())
        a = case.script(s, pre["date_index"] == pre["start"])
        off = rng.integers(0, 4, E).astype(np.int32)
        ref = tw.step(a, off, True)
        steps.append(dict(a=a, done=ref[2], pre=pre, post=_copy(tw.state())))
        if on_step:
            on_step(s, a, off, ref, tw)
    assert tw.episodes_done.min() >= 1 and sum(bool(st["done"].any()) for st in steps) >= 2
    return case, steps, end


# ---------------------------------------------------------------- device replay (the GPU tests)
def _state_keys(kind):
    from twowave_windows_cases import state_keys
    return state_keys(kind)


def _compare(kind, case, env, s, g, o_obs, o_rew, o_done, o_term, o_state):
    g_obs, g_rew, g_done = (t.cpu().numpy() for t in g[:3])
    np.testing.assert_array_equal(g_done.astype(bool), o_done, err_msg=f"done step {s}")
    np.testing.assert_array_equal(g_obs, o_obs.astype(F32), err_msg=f"obs step {s}")
    np.testing.assert_array_equal(g_rew, o_rew.astype(F32), err_msg=f"reward step {s}")
    st = env.state_numpy()
    for k in _state_keys(kind):
        if k == "turbulence" and case.kw["turbulence_threshold"] is None:
            continue
        np.testing.assert_array_equal(st[k], o_state[k], err_msg=f"{k} step {s}")
    if o_done.any():
        np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done], o_term[o_done].astype(F32),
                                      err_msg=f"term_obs step {s}")


def replay_on_device(kind, name, shape, args):
    """The batched HIP env of `kind` over the oracle trace of a case, at tolerance 0: obs, reward, done,
    terminal obs and every state field, every step, all E envs."""
    import torch
    case, starts0, obs0, steps = trace(kind, name, shape, args)
    require_events(kind, case, events(kind, case, steps))
    Panel, Env, _ = classes(kind)
    env = Env(Panel(case.close, case.info, case.turb), E, random_start=False, **env_kwargs(kind, case))
    env.enable_terminal_obs()
    env.set_next_start(starts0)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), obs0.astype(F32))
    nd = 0
    for s, st in enumerate(steps):
        env.set_next_start(st["starts"])
        g = env.step(torch.from_numpy(st["a"].copy()).cuda())
        _compare(kind, case, env, s, g, st["obs"], st["rew"], st["done"], st["term"], st["post"])
        nd += int(st["done"].any())
    assert nd >= 2


def replay_windowed(kind, name, shape, args):
    """The same through `windows=`: the WIN instantiations against one oracle per env on its slice."""
    import torch
    Panel, Env, _ = classes(kind)
    box = {}

    def on_step(s, a, off, ref, tw):
        if s < 0:
            env = box["env"] = Env(Panel(tw.close, tw.info, tw.turb), E, random_start=False,
                                   windows=(tw.pending[0].copy(), tw.pending[1].copy()), **tw.kw)
            env.enable_terminal_obs()
            env.set_next_start(off)
            np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.astype(F32))
            return
        env = box["env"]
        env.set_next_start(off)
        g = env.step(torch.from_numpy(a.copy()).cuda())
        _compare(kind, box["case"], env, s, g, *ref, tw.state())

    # (the case is needed by _compare before window_trace returns it)
    box["case"] = build(kind, name, shape, args, windowed=True)
    case, steps, end = window_trace(kind, name, shape, args, on_step)
    require_events(kind, case, events(kind, case, steps, end))
