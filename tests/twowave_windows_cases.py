"""Scenarios shared by the window tests of the cash-penalty and stop-loss envs: panels, windows,
actions, starting offsets and pending-window redraws, and `Twins` -- one CPU oracle per env, built on
the slice of the panel its ACTIVE window names -- which is what `windows=` promises of the batched env.
tests/test_twowave_windows_scenarios.py runs the twins alone and asserts that every scenario reaches
the paths the GPU tests rely on; tests/test_gpu_twowave_windows.py compares the HIP env with them."""
import numpy as np

KINDS = ("cashpenalty", "stoploss")
COMMON = dict(shares_increment=3, initial_amount=5e5, buy_cost_pct=0.002, sell_cost_pct=0.001,
              cash_penalty_proportion=0.15)
T_ROWS = 48

# every launch form (D <= 64: NCH 1; 64 < D <= 320: NCH 2; D > 320: NCH 0), both action forms, patient,
# turbulence on / off, auto_reset on / off; E: a full wave, a 1-lane tail, a 6-lane tail, four blocks
SCENARIOS = [
    dict(name="d16-disc", E=70, N=5, C=2, steps=36, hmax=300_000, thr=45.0, patient=False, disc=True,
         auto=True),
    # nearly every env runs out of cash within a few steps: more re-decided rows per block than kFix
    dict(name="d181-broke", E=200, N=30, C=5, steps=30, hmax=400_000, thr=None, patient=False,
         disc=False, auto=True),
    dict(name="d241-disc-manual", E=65, N=30, C=7, steps=30, hmax=60_000, thr=40.0, patient=False,
         disc=True, auto=False),
    dict(name="d331-patient", E=70, N=30, C=10, steps=30, hmax=60_000, thr=40.0, patient=True,
         disc=False, auto=True),
    dict(name="d331-manual", E=70, N=30, C=10, steps=24, hmax=60_000, thr=None, patient=False,
         disc=True, auto=False),
    dict(name="d2-one-asset", E=64, N=1, C=0, steps=30, hmax=700_000, thr=30.0, patient=False,
         disc=False, auto=True),
    dict(name="d65-n32", E=65, N=32, C=1, steps=30, hmax=40_000, thr=None, patient=False, disc=True,
         auto=False),
]
SCENARIO_IDS = [sc["name"] for sc in SCENARIOS]


def classes(kind):
    """(panel class, batched env class, oracle class) of a kind."""
    from finrl_amd.vec_cashpenalty import CashPenaltyPanel, VecCashPenaltyEnv, VecStopLossEnv
    if kind == "cashpenalty":
        from oracle.cashpenalty import CashPenaltyOracle
        return CashPenaltyPanel, VecCashPenaltyEnv, CashPenaltyOracle
    from oracle.stoploss import StopLossOracle
    return CashPenaltyPanel, VecStopLossEnv, StopLossOracle


def env_kwargs(sc):
    return dict(hmax=sc["hmax"], turbulence_threshold=sc["thr"], patient=sc["patient"],
                discrete_actions=sc["disc"], **COMMON)


def make_panel(N, C, T=T_ROWS, seed=0):
    """close [T, N] on a path rough enough for stop-loss sales (a 10 % drop below the average buy
    price within a few rows), info [T, N, C], turb [T]."""
    rng = np.random.default_rng(1000 + 31 * N + C + seed)
    close = 50 * np.exp(np.cumsum(rng.normal(0, 0.07, (T, N)), axis=0))
    return close, rng.normal(0, 10, (T, N, C)), np.abs(rng.normal(0, 30, T))


def draw_windows(rng, T, E, one_row=()):
    """Random windows of 1..12 rows inside [0, T); the envs in `one_row` get one-row windows."""
    length = rng.integers(2, 13, E)
    length[list(one_row)] = 1
    s = rng.integers(0, T - length + 1)
    return s.astype(np.int64), (s + length).astype(np.int64)


class Script:
    """What a scenario feeds the env, step by step, from one seed: actions [E, N] f32 (small ones for
    every eighth env, so that not all of them are out of cash within a few steps), NEXT_START
    offsets [E] (some past the end of a short window: the kernel clamps them), and every third step
    a redraw of the pending windows of a random third of the envs."""

    def __init__(self, sc, seed=0):
        self.sc, self.rng = sc, np.random.default_rng(7 + seed + sc["E"] + sc["N"])
        self.start, self.end = draw_windows(self.rng, T_ROWS, sc["E"], one_row=(1, sc["E"] - 1))
        self.offsets0 = self.rng.integers(0, 6, sc["E"]).astype(np.int32)

    def step(self, s):
        """-> (actions, offsets, redraw) with redraw = None or (mask [E] bool, start [E], end [E])."""
        sc, rng = self.sc, self.rng
        a = rng.uniform(-1, 1, (sc["E"], sc["N"])).astype(np.float32)
        a[::8] *= np.float32(0.004)      # every eighth env trades small: it keeps positions for a while
        off = rng.integers(0, 6, sc["E"]).astype(np.int32)
        redraw = None
        if s % 3 == 1:
            m = rng.random(sc["E"]) < 0.35
            ns, nt = draw_windows(rng, T_ROWS, sc["E"], one_row=(2,) if s % 2 else ())
            redraw = (m, ns, nt)
        return a, off, redraw


class Twins:
    """One oracle per env on panel[s_e:t_e] of its ACTIVE window.  A reset of env e first takes the
    PENDING window (a new oracle on that slice when it differs) and starts on
    clamp(offset, 0, t - s - 1) of it.  State fields are reported as the batched env holds them:
    date_index / start as PANEL rows, episode counted over the env's resets, and logged_total /
    logged_cash surviving a reset until the new episode's first trading step (the reference's reset
    leaves them alone)."""

    def __init__(self, kind, sc, close, info, turb, start, end, kw=None):
        self.kind, self.sc = kind, sc
        self.kw = env_kwargs(sc) if kw is None else kw          # the env arguments of every oracle
        self.Oracle = classes(kind)[2]
        self.close, self.info, self.turb = close, info, turb
        E = sc["E"]
        self.E, self.N, self.D = E, close.shape[1], 1 + close.shape[1] * (1 + info.shape[2])
        self.pending = np.stack([np.asarray(start, np.int64), np.asarray(end, np.int64)])
        self.active = np.stack([np.zeros(E, np.int64), np.full(E, close.shape[0], np.int64)])
        self.orc = [None] * E
        self.episode = np.full(E, -1, np.int32)
        self.carry = np.zeros((2, E))                 # logged_total, logged_cash across a reset
        self.fresh = np.zeros(E, bool)
        # coverage counters (tests/test_twowave_windows_scenarios.py)
        self.episodes_done = np.zeros(E, np.int64)
        self.n_cash_end_inside = self.n_last_date_end = self.n_reset_on_new_window = 0
        self.n_forced_sales = 0
        self.one_row_episodes = 0

    def set_pending(self, mask, start, end):
        self.pending[0][mask], self.pending[1][mask] = start[mask], end[mask]

    def _reset_env(self, e, offset):
        s, t = self.pending[:, e]
        if self.orc[e] is not None:
            st = self.orc[e].state()
            if not self.fresh[e]:
                self.carry[:, e] = st["logged_total"][0], st["logged_cash"][0]
        if self.orc[e] is None or (s, t) != tuple(self.active[:, e]):
            if self.orc[e] is not None:
                self.n_reset_on_new_window += 1
            self.orc[e] = self.Oracle(self.close[s:t], self.info[s:t], self.turb[s:t], n_envs=1,
                                      **self.kw)
            self.fresh[e] = True
        self.active[:, e] = s, t
        self.one_row_episodes += int(t - s == 1)
        self.episode[e] += 1
        return self.orc[e].reset(int(min(max(int(offset), 0), t - s - 1)))[0]

    def reset(self, offsets, mask=None):
        """-> obs [E, D] f64 (rows of envs outside the mask are NaN)."""
        obs = np.full((self.E, self.D), np.nan)
        for e in range(self.E):
            if mask is None or mask[e]:
                obs[e] = self._reset_env(e, offsets[e])
        return obs

    def _forced_sale(self, e, st):
        if self.kind != "stoploss":
            return False
        s, t = self.active[:, e]
        di = int(st["date_index"][0])
        if di == t - s - 1:
            return False
        c = COMMON
        armed = st["coh"][0] >= 0.9 * c["initial_amount"]
        cd = self.close[s + di] - 0.9 * st["avg_buy_price"][0]
        return bool(armed and ((cd < 0) & (st["holdings"][0] > 0)).any())

    def step(self, actions, offsets, auto_reset):
        """-> obs, reward, done, term_obs as the batched env reports them (f64, term rows of envs that
        did not finish are zero)."""
        E = self.E
        obs, term = np.empty((E, self.D)), np.zeros((E, self.D))
        rew, done = np.empty(E), np.zeros(E, bool)
        for e in range(E):
            o = self.orc[e]
            s, t = self.active[:, e]
            before = o.state()
            di = int(before["date_index"][0])
            self.n_forced_sales += int(self._forced_sale(e, before))
            ob, r, d = o.step(actions[e:e + 1])
            obs[e], rew[e], done[e] = ob[0], r[0], d[0]
            if di < t - s - 1:
                self.fresh[e] = False
            if d[0]:
                self.episodes_done[e] += 1
                if di == t - s - 1:
                    self.n_last_date_end += 1
                else:
                    self.n_cash_end_inside += 1
                if auto_reset:
                    term[e] = ob[0]
                    obs[e] = self._reset_env(e, offsets[e])
        return obs, rew, done, term

    def state(self):
        """Every state field of the oracles, [E] / [E, N], in the batched env's terms."""
        per = [o.state() for o in self.orc]
        out = {k: np.concatenate([p[k] for p in per]) for k in per[0]}
        out["date_index"] = (out["date_index"] + self.active[0]).astype(np.int32)
        out["start"] = (out["start"] + self.active[0]).astype(np.int32)
        out["episode"] = self.episode.copy()
        out["logged_total"] = np.where(self.fresh, self.carry[0], out["logged_total"])
        out["logged_cash"] = np.where(self.fresh, self.carry[1], out["logged_cash"])
        return out


def state_keys(kind):
    from oracle.stoploss import SCALARS, VECTORS
    if kind == "stoploss":
        return SCALARS + VECTORS + ("date_index", "start", "episode")
    return ("coh", "holdings", "date_index", "start", "turbulence", "sum_trades", "logged_total",
            "logged_cash", "episode")


def nan_padded(blocks, pad, N, C):
    """[pad NaN rows, block, pad NaN rows, block, ..., pad NaN rows] of (close, info, turb) blocks ->
    (close, info, turb, offsets of the blocks)."""
    closes, infos, turbs, offs, row = [], [], [], [], 0
    nan = (np.full((pad, N), np.nan), np.full((pad, N, C), np.nan), np.full(pad, np.nan))
    for close, info, turb in blocks:
        for lst, x in zip((closes, infos, turbs), nan):
            lst.append(x)
        row += pad
        offs.append(row)
        closes.append(close), infos.append(np.asarray(info).reshape(len(close), N, C)), turbs.append(turb)
        row += len(close)
    for lst, x in zip((closes, infos, turbs), nan):
        lst.append(x)
    return np.concatenate(closes), np.concatenate(infos), np.concatenate(turbs), offs
