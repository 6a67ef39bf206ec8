"""Market panels outside the value range every other test draws from (closes within a factor of three
of 50 or 100, no zero close, flags only at exactly 1.0 against continuous draws, thresholds that no
risk value equals), shared by the tests/test_gpu_*_panel_domain.py files (HIP kernels vs the oracles)
and tests/test_oracle_panel_domain.py (the stock oracle vs oracle/pandas_env.py).  Everything here is
host-side NumPy.  Each builder comes with a counter that reads, from oracle outputs alone (`realised`
and the state before and after a step), how often each event the case exists for occurred, and that
raises where the oracle does not treat such a cell as the panel domain says (include/finenv.h,
"Panel domain"): a case that does not hold what its name says fails instead of testing less.

Out of scope: NaN / infinite prices, indicators or risk values, and negative closes (rejected by
StockPanel.signed_close)."""
import collections

import numpy as np

F32 = np.float32
K = 2
FLAG_VALUES = (1.0, float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0)),
               float(np.float64(F32(1)) + 2.0 ** -30), -1.0)
# the fourth value rounds to 1.0 in the f32 observation and is still no flag
assert FLAG_VALUES[3] != 1.0 and F32(FLAG_VALUES[3]) == F32(1) and F32(FLAG_VALUES[1]) == F32(1)

Case = collections.namedtuple("Case", "close tech risk threshold cash0 shares0")
# close [T, N] f64, tech [T, K, N] f64, risk [T] f64, threshold (the value `turbulence_threshold` takes
# when turbulence is on), cash0 [E] f64, shares0 [E, N] int64


def scaled(actions, hmax):
    """trunc(f32(action) * f32(hmax)) as int64 (env_stocktrading.py:304-305)."""
    return np.trunc(np.asarray(actions, F32) * F32(hmax)).astype(np.int64)


def actions(E, N, steps, seed):
    """[steps, E, N] float32: uniform(-1, 1) with 5 % exact zeros -- every cell of a panel row is asked
    for buys and for sells by many envs on every step."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (steps, E, N)).astype(F32)
    a[rng.random(a.shape) < 0.05] = 0.0
    return a


def _base(rng, T, N):
    close = (50 + rng.uniform(0, 10, (T, N))).astype(F32).astype(np.float64)
    tech = rng.normal(0, 1, (T, K, N)).astype(F32).astype(np.float64)
    tech[tech == 1.0] = 0.5
    return close, tech


def _risk_with_ties(rng, T):
    """Continuous draws below a threshold that two rows (days 2 and 5) equal exactly: `>=` decides."""
    risk = rng.uniform(1, 30, T)
    thr = 41.7
    risk[[d for d in (2, 5) if d < T]] = thr
    return risk, thr


def _books(rng, E, N, cash=1e6):
    return np.full(E, float(cash)), rng.integers(0, 40, (E, N)).astype(np.int64)


# ---------------------------------------------------------------- builders
def zero_closes(N, T, E, seed, f32_prices=False, keep_day0=False):
    """Usual-scale panel with zero closes: ~15 % scattered cells, ticker 1 on every day, the whole of
    day 3 (never day 0); flags (tech_0 == 1.0) at ~15 % independent of the zeros, so flagged zeros
    (-0.0 on the device) exist; initial shares in [0, 40), so zero-priced tickers are held.
    keep_day0: no zero in row 0 at all (for envs that divide by the first row)."""
    rng = np.random.default_rng(seed)
    close, tech = _base(rng, T, N)
    zero = rng.random((T, N)) < 0.15
    if N > 1:
        zero[:, 1] = True
    if T > 3:
        zero[3, :] = True
    if keep_day0:
        zero[0, :] = False
    else:
        zero[0, 0] = False                       # (the begin asset of an episode stays positive)
    close[zero] = 0.0
    tech[:, 0, :][rng.random((T, N)) < 0.15] = 1.0
    risk, thr = _risk_with_ties(rng, T)
    cash0, shares0 = _books(rng, E, N)
    if f32_prices:
        close = close.astype(F32).astype(np.float64)
    return Case(close, tech, risk, thr, cash0, shares0)


def price_scales(N, T, E, seed, lo=-4.0, hi=5.5, f32_prices=False):
    """Per-ticker level 10^U(lo, hi) times a 2 % random walk, kept as fp64 (no float32 round trip
    unless the env's prices are f32); per-env initial cash 10^U(2, 9); flags at ~3 %."""
    rng = np.random.default_rng(seed)
    _, tech = _base(rng, T, N)
    level = 10.0 ** rng.uniform(lo, hi, N)
    level[:2] = 10.0 ** lo, 10.0 ** hi             # both ends are always there
    close = level * np.exp(np.cumsum(rng.normal(0, 0.02, (T, N)), axis=0))
    if f32_prices:
        close = close.astype(F32).astype(np.float64)
    tech[:, 0, :][rng.random((T, N)) < 0.03] = 1.0
    risk, thr = _risk_with_ties(rng, T)
    cash0 = 10.0 ** rng.uniform(2, 9, E)
    cash0[:2] = 1e2, 1e9                           # (so are these)
    shares0 = rng.integers(0, 40, (E, N)).astype(np.int64)
    return Case(close, tech, risk, thr, cash0, shares0)


def flag_neighbours(N, T, E, seed):
    """tech_0 takes each of FLAG_VALUES in ~12 % of the cells: only exact 1.0 may block a trade."""
    rng = np.random.default_rng(seed)
    close, tech = _base(rng, T, N)
    pick = rng.integers(0, 8, (T, N))
    for j, v in enumerate(FLAG_VALUES):
        tech[:, 0, :][pick == j] = v
    risk, thr = _risk_with_ties(rng, T)
    cash0, shares0 = _books(rng, E, N)
    return Case(close, tech, risk, thr, cash0, shares0)


def threshold_ties(N, T, E, seed, zero=False):
    """`turbulence >= threshold` at the threshold and its fp64 neighbours.  Rows alternate between a
    value below the threshold (the envs buy) and one to be told apart (then everything held is sold
    or not): [., lo, thr, lo, hi, lo, thr, lo] with lo / hi = nextafter(thr, 0 / inf).
    zero: threshold 0.0 and rows [., -1, 0.0, -1, -0.0, -1, 0.0, -1] -- 0.0 >= 0.0 and -0.0 >= 0.0
    liquidate, as does the 0.0 a reset leaves in `turbulence`; -1 rows are there only so that shares
    are bought back before the next 0.0 row."""
    assert T >= 8
    rng = np.random.default_rng(seed)
    close, tech = _base(rng, T, N)
    if zero:
        thr, row = 0.0, [5.0, -1.0, 0.0, -1.0, -0.0, -1.0, 0.0, -1.0]
    else:
        thr = 37.3
        lo, hi = float(np.nextafter(thr, 0.0)), float(np.nextafter(thr, np.inf))
        row = [1.0, lo, thr, lo, hi, lo, thr, lo]
    risk = np.resize(np.array(row), T)
    cash0, shares0 = _books(rng, E, N)
    return Case(close, tech, risk, thr, cash0, shares0)


STOCK_CASES = {
    "zero_closes": zero_closes,
    "price_scales": price_scales,
    "flag_neighbours": flag_neighbours,
    "threshold_ties": threshold_ties,
    "threshold_zero": lambda N, T, E, seed: threshold_ties(N, T, E, seed, zero=True),
}


# ---------------------------------------------------------------- event counter (stock oracle)
def stock_events(case, hmax, use_turbulence, acts, pre, real, post, buy_cost_pct=1e-3):
    """Counts per event over a trace of oracle.stock.StockOracle.  acts [S, E, N] f32 as fed; pre / post
    [S] state() dicts around each step (post taken before any reset); real [S, E, N] `realised`.
    Asserts on the way that the oracle applies the panel-domain rules to every such cell and that
    every step's trade count is the one those rules give."""
    ev = collections.Counter()
    T = case.close.shape[0]
    thr = case.threshold
    for s in range(len(acts)):
        st, en, r = pre[s], post[s], real[s]
        live = st["day"] < T - 1                                # a terminal step trades nothing
        assert (r[~live] == 0).all()
        p = case.close[st["price_day"]]                         # the row the env holds: [E, N]
        t0 = case.tech[st["price_day"], 0, :]
        flag = t0 == 1.0
        h = st["shares"]
        turb = (st["turbulence"] >= thr) & live if use_turbulence else np.zeros(len(live), bool)
        calm = (live & ~turb)[:, None]
        turb = turb[:, None]
        want = scaled(acts[s], hmax)
        zero, pos = p == 0.0, p > 0.0
        buy, sell = calm & (want > 0), calm & (want < 0) & (h > 0)

        n_trades = (sell & ~flag).sum(1) + (buy & ~flag & pos).sum(1) + (turb & (h > 0) & pos).sum(1)
        np.testing.assert_array_equal(en["trades"] - st["trades"], n_trades, err_msg=f"step {s}")

        m = buy & ~flag & zero                                  # fills 0 shares and is no trade
        assert (r[m] == 0).all()
        ev["buy_at_zero"] += int(m.sum())
        m = sell & ~flag & zero                                 # removes shares, is a trade, adds +0.0
        np.testing.assert_array_equal(r[m], -np.minimum(-want[m], h[m]))
        ev["sell_at_zero"] += int(m.sum())
        only = m.any(1) & (((r != 0) & ~zero).sum(1) == 0)       # ... and cash stays what it was
        assert (en["cash"][only] == st["cash"][only]).all()
        ev["only_zero_trades"] += int(only.sum())
        m = buy & flag & zero
        assert (r[m] == 0).all()
        ev["buy_at_flagged_zero"] += int(m.sum())
        m = sell & flag & zero
        assert (r[m] == 0).all()
        ev["sell_at_flagged_zero"] += int(m.sum())

        kept, sold = turb & (h > 0) & zero, turb & (h > 0) & pos & flag
        assert (r[kept] == 0).all() and (en["shares"][kept] == h[kept]).all()
        np.testing.assert_array_equal(r[sold], -h[sold])
        ev["turbulent_zero_kept"] += int(kept.sum())
        ev["turbulent_flagged_sold"] += int(sold.sum())
        ev["turbulent_step_with_both"] += int((kept.any(1) & sold.any(1)).sum())

        m = buy & ~flag & pos
        ev["buy_action_binds"] += int((r[m] == want[m]).sum())
        ev["buy_cash_binds"] += int((r[m] < want[m]).sum())
        unit = np.where(pos, p * (1 + buy_cost_pct), 1.0)
        ev["buy_quotient_over_2p40"] += int(
            (m & (np.minimum(st["cash"], en["cash"])[:, None] / unit > 2.0 ** 40)).sum())

        for j, v in enumerate(FLAG_VALUES):                     # what trades at each value of tech_0
            m = (buy | sell) & (t0 == v) & pos
            ev[f"tech0_value{j}_requests"] += int(m.sum())
            ev[f"tech0_value{j}_trades"] += int((r[m] != 0).sum())

        if use_turbulence:                                      # from `realised` alone: who liquidated
            full = ((r == -h) | ~pos).all(1) & ((h > 0) & pos).any(1) & live
            bought = (r > 0).any(1)
            below = -1.0 if thr == 0.0 else np.nextafter(thr, -np.inf)
            for name, v in (("at_threshold", thr), ("below_threshold", below),
                            ("above_threshold", np.nextafter(thr, np.inf))):
                at = st["turbulence"] == v
                if name == "at_threshold" and thr == 0.0:
                    ev["minus_zero_liquidates"] += int((at & full & np.signbit(st["turbulence"])).sum())
                ev[f"{name}_liquidates"] += int((at & full).sum())
                ev[f"{name}_buys"] += int((at & bought).sum())
    return ev


def require_stock_events(name, ev, use_turbulence):
    """What keeps a parametrised case from passing vacuously."""
    def need(*keys):
        for k in keys:
            assert ev[k] > 0, f"{name}: event {k} never occurs ({dict(ev)})"
    if name == "zero_closes":
        need("buy_at_zero", "sell_at_zero", "only_zero_trades", "buy_at_flagged_zero", "sell_at_flagged_zero")
        if use_turbulence:
            need("turbulent_step_with_both", "at_threshold_liquidates")
    elif name == "price_scales":
        need("buy_action_binds", "buy_cash_binds", "buy_quotient_over_2p40")
    elif name == "flag_neighbours":
        assert ev["tech0_value0_requests"] > 0 and ev["tech0_value0_trades"] == 0, dict(ev)
        need(*[f"tech0_value{j}_trades" for j in range(1, len(FLAG_VALUES))])
    elif name == "threshold_ties" and use_turbulence:
        need("at_threshold_liquidates", "above_threshold_liquidates", "below_threshold_buys")
        assert ev["at_threshold_buys"] == 0 and ev["above_threshold_buys"] == 0, dict(ev)
    elif name == "threshold_zero" and use_turbulence:
        need("at_threshold_liquidates", "minus_zero_liquidates", "below_threshold_buys")
        assert ev["at_threshold_buys"] == 0, dict(ev)


def stock_trace(case, hmax, use_turbulence, acts, make_oracle):
    """Drive one lock-step StockOracle batch over acts [S, E, N], resetting it when every env is done
    (what the batched env's auto-reset does).  -> obs0, trace: per step a dict of the outputs the GPU
    tests compare plus `pre` / `post` state for stock_events()."""
    orc = make_oracle()
    obs0 = orc.reset()
    trace = []
    keys = ("cash", "shares", "cost", "trades", "day", "price_day", "turbulence")
    for s in range(len(acts)):
        pre = {k: v.copy() for k, v in orc.state().items() if k in keys}
        obs, rew, done, real = orc.step(acts[s], want_realised=True)
        assert done.all() or not done.any()
        post = {k: v.copy() for k, v in orc.state().items() if k in keys}
        term = obs
        if done.all():
            obs = orc.reset()
        fin = orc.state()
        trace.append(dict(obs=obs, term=term, rew=rew, done=done, real=real, pre=pre, post=post,
                          stats=orc.episode_stats(), cash=fin["cash"], shares=fin["shares"],
                          cost=fin["cost"], trades=fin["trades"]))
    return obs0, trace


# ---------------------------------------------------------------- array-state env (oracle.stocknp)
NP_THRESH = 99                      # the env's default turbulence_thresh; `>` there, so 99.0 is calm


def np_case(name, N, T, E, seed):
    """-> (config arrays, stocks0 [E, N] f32, amount0 [E], amount0_tag [E]) for VecStockTradingEnvNP /
    StockNpOracle.  Prices are float32 there, so `price_scales` uses levels 10^U(-3, 5); no zero in
    row 0 (reset values the start holdings on it and the episode return divides by that).  Day 6 is
    turbulent (late, so that start holdings of zero-priced tickers are still there once a wave has
    reached its all-float64 state), day 4 sits exactly on the threshold (calm).  Start amounts are a mix of
    Python-float and float32 tags, as eval and train mode produce."""
    rng = np.random.default_rng(seed)
    if name == "zero_closes":
        c = zero_closes(N, T, E, seed, f32_prices=True, keep_day0=True)
        amount0 = 1e6 * rng.uniform(0.9, 1.1, E)
    else:
        c = price_scales(N, T, E, seed, lo=-3.0, hi=5.0, f32_prices=True)
        amount0 = c.cash0
    turb = np.abs(rng.normal(0, 40, T)).clip(0, 90)
    turb[6] = 150.0
    turb[4] = float(NP_THRESH)
    tag = rng.integers(0, 2, E).astype(np.int32)
    amount0 = np.where(tag == 1, amount0.astype(F32), amount0).astype(np.float64)
    arrays = {"price_array": c.close, "tech_array": rng.normal(0, 50, (T, N * K)),
              "turbulence_array": turb, "if_train": False}
    return arrays, rng.integers(0, 40, (E, N)).astype(F32), amount0, tag


def np_events(price, turb_bool, max_stock, min_action, acts, pre, post, wave=64):
    """Event counts over a StockNpOracle trace (price / turb_bool: the oracle's derived f32 arrays; pre /
    post: state() around each step, post before any reset).  A request at a zero price must leave the
    holdings alone and the cool-down counting (`price > 0` guards sells and buys alike); each is
    booked under the path its wave takes: `steady` when all 64 envs carry a float64 cash, `mixed` else."""
    ev = collections.Counter()
    for s in range(len(acts)):
        st, en = pre[s], post[s]
        row = st["day"] + 1
        p = price[row]
        calm = (turb_bool[row] == 0.0)[:, None]
        a = np.trunc(np.asarray(acts[s], F32) * F32(max_stock)).astype(np.int64)
        f64 = st["amount_tag"] == 2
        full = len(f64) // wave * wave                          # (a partial wave is booked under neither)
        steady = np.zeros((len(f64), 1), bool)
        mixed = np.zeros((len(f64), 1), bool)
        for w in range(0, full, wave):
            steady[w:w + wave] = f64[w:w + wave].all()
            mixed[w:w + wave] = not f64[w:w + wave].all()
        sell = calm & (a < -min_action) & (st["stocks"] > 0)
        buy = calm & (a > min_action)
        for kind, m in (("sell", sell & (p == 0)), ("buy", buy & (p == 0))):
            assert (en["stocks"][m] == st["stocks"][m]).all()
            assert (en["cool_down"][m] == st["cool_down"][m] + 1).all()
            ev[f"{kind}_at_zero_steady"] += int((m & steady).sum())
            ev[f"{kind}_at_zero_mixed"] += int((m & mixed).sum())
        m = ~calm & (st["stocks"] > 0) & (p == 0)
        assert (en["stocks"][~calm[:, 0]] == 0).all()
        ev["turbulent_zero_liquidated"] += int(m.sum())
        m = buy & (p > 0)
        got = en["stocks"] - st["stocks"]
        ev["buy_action_binds"] += int((got[m] == a[m]).sum())
        ev["buy_cash_binds"] += int((got[m] < a[m]).sum())
        ev["steady_wave_steps"] += int(steady[:full:wave].sum())
        ev["mixed_wave_steps"] += int(mixed[:full:wave].sum())
    return ev


# ---------------------------------------------------------------- crypto env (oracle.crypto)
def crypto_case(name, N, T, W, seed):
    """-> price [T, N] f64, tech [T, W] f64.  `zero_closes`: usual scale, ~15 % zero cells, asset 1 zero
    from row 1 on, one whole row zero -- none in row 0, which action_norm_vector takes logarithms of.
    `price_scales`: levels 10^U(-8, 5) (both ends present) times a 0.4 % walk."""
    rng = np.random.default_rng(seed)
    if name == "zero_closes":
        price = zero_closes(N, T, 1, seed, keep_day0=True).close
    else:
        level = 10.0 ** rng.uniform(-8, 5, N)
        level[:2] = (2e-8, 9e4)[:min(N, 2)]
        price = level * np.exp(np.cumsum(rng.normal(0, 0.004, (T, N)), axis=0))
    return price, rng.normal(0, 3000, (T, W))


def crypto_events(price, norm, acts, pre, post):
    """Event counts over a CryptoOracle trace (pre / post: state() around each step, post before any
    reset): requests at a zero price leave the holdings alone; buys whose `cash // price` exceeds 2^40."""
    ev = collections.Counter()
    for s in range(len(acts)):
        st, en = pre[s], post[s]
        assert (en["time"] == st["time"] + 1).all()
        p = price[en["time"]]
        a = (np.asarray(acts[s], np.float64) * norm).astype(F32)
        for kind, m in (("sell", (a < 0) & (st["stocks"] > 0) & (p == 0)), ("buy", (a > 0) & (p == 0))):
            assert (en["stocks"][m] == st["stocks"][m]).all()
            ev[f"{kind}_at_zero"] += int(m.sum())
        m = (a > 0) & (p > 0)
        got = en["stocks"].astype(np.float64) - st["stocks"]
        ev["buy_action_binds"] += int((got[m] > 0.75 * a[m]).sum())
        ev["buy_cash_binds"] += int((got[m] < 0.25 * a[m]).sum())
        cash = np.minimum(st["cash"], en["cash"])[:, None]
        ev["buy_quotient_over_2p40"] += int((m & (cash / np.where(p > 0, p, 1.0) > 2.0 ** 40)).sum())
        ev["steps_with_mixed_time"] += int(len(np.unique(st["time"])) > 1)
    return ev
