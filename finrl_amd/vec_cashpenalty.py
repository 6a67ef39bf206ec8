"""Device-resident batch of the reference's StockTradingEnvCashpenalty
(finrl/meta/env_stock_trading/env_stocktrading_cashpenalty.py:19-409), one HIP launch per step
through the C ABI (finenv_cashpenalty_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat
from .spaces import Box
from .vec_base import WindowedEnv


class CashPenaltyPanel:
    """close [T,N] f64, info [T,N,C] f64 (daily_information_cols per asset, ticker-major as
    get_date_vector builds them, :159-171), turb [T]."""

    def __init__(self, close, info, turb=None, dates=None, assets=None):
        self.close = np.ascontiguousarray(close, dtype=np.float64)
        T, N = self.close.shape
        self.info = np.ascontiguousarray(info, dtype=np.float64).reshape(T, N, -1)
        self.turb = np.ascontiguousarray(np.zeros(T) if turb is None else turb, np.float64)
        self.T, self.N, self.C = T, N, self.info.shape[2]
        self.D = 1 + N + N * self.C
        self.dates = list(dates) if dates is not None else list(range(T))
        self.assets = list(assets) if assets is not None else [f"A{i}" for i in range(N)]

    @classmethod
    def from_dataframe(cls, df, daily_information_cols, date_col_name="date"):
        """assets = df.tic.unique() (order of appearance), dates = sorted unique (:70-71)."""
        assets = list(dict.fromkeys(df["tic"].tolist()))
        dates = sorted(df[date_col_name].unique().tolist())
        T, N = len(dates), len(assets)
        piv = df.set_index([date_col_name, "tic"]).sort_index()
        idx = [(d, a) for d in dates for a in assets]
        sub = piv.loc[idx]
        close = sub["close"].to_numpy(np.float64).reshape(T, N)
        info = sub[list(daily_information_cols)].to_numpy(np.float64).reshape(T, N, -1)
        turb = sub["turbulence"].to_numpy(np.float64).reshape(T, N)[:, 0] \
            if "turbulence" in sub.columns else None
        return cls(close, info, turb, dates, assets)


class VecCashPenaltyEnv(WindowedEnv):
    """``windows=(start, end)`` gives every env its own episode window of panel rows ``[start, end)``
    (one value or ``[E]`` each): env ``e`` then equals the reference env built on the frame restricted
    to ``dates[start_e:end_e]`` -- a train env and a trade env, ensemble validation windows or random
    training windows, in ONE batch over one panel.  ``state["date_index"]`` and ``state["start"]`` stay
    panel rows; ``window_day()`` is the reference's ``self.date_index``.  See ``set_windows``."""
    env_name = "StockTradingEnvCashpenalty-MI355X"
    if_discrete = False
    _kind = "cashpenalty"
    _cfg_cls, _panel_cls, _state_cls = nat.CashPenaltyConfig, nat.CashPenaltyPanelPtrs, \
        nat.CashPenaltyStatePtrs
    # holdings: an [N][E] f64 book after the scalar rows
    _layout = {"f64": (nat.CASHPENALTY_F64_FIELDS, ("holdings",)),
               "i32": (nat.CASHPENALTY_I32_FIELDS, ())}

    def _extra_cfg(self, **kw):
        if kw:
            raise TypeError(f"unexpected arguments {sorted(kw)}")
        return ()

    def __init__(self, panel: CashPenaltyPanel, num_envs, *, buy_cost_pct=3e-3, sell_cost_pct=3e-3,
                 hmax=10, discrete_actions=False, shares_increment=1, turbulence_threshold=None,
                 initial_amount=1e6, cash_penalty_proportion=0.1, random_start=True, patient=False,
                 auto_reset=True, device="cuda", seed=0, windows=None, **extra):
        import torch
        self._set_device(device)
        self.panel = panel
        E, N, Cc, T = int(num_envs), panel.N, panel.C, panel.T
        self.num_envs = self.env_num = E
        self.action_dim = N
        self.state_dim = self.state_space = panel.D
        self.random_start = bool(random_start)
        self.auto_reset = bool(auto_reset)
        self.max_step = T - 1
        self.observation_space = Box(-np.inf, np.inf, (panel.D,), np.float32)
        self.action_space = Box(-1, 1, (N,), np.float32)
        self._seed, self._rs_on_device = int(seed) & (2 ** 63 - 1), False
        self._open(self._cfg_cls(
            E, N, Cc, T, int(discrete_actions), int(shares_increment),
            int(turbulence_threshold is not None), int(patient), float(hmax), float(buy_cost_pct),
            float(sell_cost_pct), float(initial_amount), float(cash_penalty_proportion),
            float(turbulence_threshold if turbulence_threshold is not None else 0.0),
            *self._extra_cfg(**extra)))
        dev = self.device
        self._close = torch.from_numpy(panel.close).to(dev)
        self._info = torch.from_numpy(panel.info.reshape(T, N * Cc).astype(np.float32)).to(dev)
        self._turb = torch.from_numpy(panel.turb).to(dev)
        self._alloc_state(E, N)
        self.state["episode"].fill_(-1)                                         # :98
        self._bind(self._close, self._info, self._turb)
        self._alloc_outputs(E, panel.D)
        self.audit = None
        if windows is not None:                       # attached before the first reset(), which puts
            self.set_windows(*self._check_windows(*windows))          # every env on its window

    # ------------------------------------------------------------------ episode windows
    _window_active = True                             # pending / active rows, as the crypto env
    _window_min = 1                                   # the n_days rule of finenv_<kind>_create

    def set_windows(self, start, end=None, mask=None):
        """Per-env episode windows [start, end) of panel rows (finenv_<kind>_set_windows), with the
        arguments, validation and device-tensor rules of ``WindowedEnv.set_windows``; a one-row
        window is legal (its first step ends at the last date).  ``set_windows(None)`` detaches.

        ``self.windows`` holds the PENDING windows: an env takes its pair at its next reset
        (``reset()`` for the envs it selects, or the auto-reset inside ``step``), whatever is
        written here meanwhile; the running episodes' windows are in ``self.active_windows``
        (kernel-owned, read-only for the caller).  So windows can be redrawn for the envs that just
        reported ``done`` with no reset launch, also inside a captured graph::

            obs, rew, done, _ = env.step(actions)          # auto-reset: took the pending windows
            env.set_windows(*random_windows(T, E, L, device=dev), mask=done)   # for the one after

        A reset starts env ``e`` inside its new window ``[s, t)``: with ``random_start`` on
        ``s + draw`` in ``[s, s + max(1, (t - s) // 2))``, else on ``s + next_start`` (see
        ``set_next_start``).  Attaching windows to a running batch leaves every env on the whole
        panel until its next reset.  ``max_step`` is that of the longest pending window."""
        return super().set_windows(start, end, mask)

    def window_day(self):
        """The reference's ``self.date_index`` of every env (int32 [E], device): the panel row
        minus the start row of the window its episode runs on."""
        if self.active_windows is None:
            return self.state["date_index"]
        return self.state["date_index"] - self.active_windows[0]

    def enable_audit(self):
        """Per-step harness log rows [E, AUDIT_HEAD + N] f64 (begin cash, asset value, reward,
        reason flags, applied transactions): what the single-env facade appends to the reference's
        account_information / transaction_memory lists.  Off by default (no extra traffic)."""
        import torch
        if getattr(self, "audit", None) is None:
            self.audit = torch.zeros(self.num_envs, nat.AUDIT_HEAD + self.action_dim,
                                     dtype=torch.float64, device=self.device)
            self._call("set_audit", C.c_void_p(self.audit.data_ptr()))
        return self.audit

    history = None              # enable_history()

    def enable_history(self, capacity=None, transactions=True, actions=True):
        """Record every env's episode on the device: the reference's ``account_information``,
        ``actions_memory`` (with ``actions``) and ``transaction_memory`` (with ``transactions``), copied
        from the audit row by one small kernel behind every step (finenv_<kind>_set_history) -- no
        device-to-host copy per step, no host loop, it sits in a captured graph, and under
        ``auto_reset`` the finished episode stays readable.  Calls ``enable_audit()`` first: the record
        is a copy of the audit row.  Returns the ``finrl_amd.history.TwoWaveEpisodeHistory`` (also
        ``self.history``) with ``save_asset_memory(e)`` / ``save_action_memory(e)``, the frames of the
        reference's methods for a whole batch of back-test windows; idempotent: a second call returns the
        same object whatever its arguments.

        ``capacity``: entries per env, by default the longest episode (``max_step + 1``: the rows of
        the longest pending window, ``T`` without windows) AS IT IS AT THIS CALL: windows made longer
        by a later ``set_windows`` do not grow the record, an episode that outruns it sets ``overflow``
        and keeps its first ``capacity`` entries.  Memory: ``E * (28 * capacity + 20)`` bytes plus
        ``8 * E * N * capacity`` for the transactions and ``4 * E * N * capacity`` for the actions.
        Every env is armed at its current date with an empty record; ``reset(mask)`` arms the envs it
        resets, the auto-reset inside ``step`` does not.  Enable it before capturing a graph."""
        if self.history is None:
            from .history import TwoWaveEpisodeHistory
            self.enable_audit()
            self.history = TwoWaveEpisodeHistory(
                self, self.max_step + 1 if capacity is None else capacity, transactions, actions)
        return self.history

    def set_next_start(self, starts):
        """Starting points the next reset of each env will use (the reference draws
        random.choice(range(int(len(dates) * 0.5))), :134-138).  Panel rows; with windows attached
        OFFSETS from the first row of each env's pending window (the reference's starting point on
        the env's own slice), clamped into the window by the kernel."""
        import torch
        self.state["next_start"].copy_(torch.as_tensor(
            np.broadcast_to(np.asarray(starts, np.int32), (self.num_envs,)).copy()))

    def _draw_starts(self):
        """random_start: resets draw their starting point on the device (set once; no host work
        per step).  `set_next_start()` + random_start=False pins them for reproducible runs.
        With windows attached the `hi` passed here only switches the draw on: env e then draws in
        [0, max(1, (t_e - s_e) // 2)) of the window it is reset onto -- int(len(dates) * 0.5) of
        its own slice -- and starts on s_e + draw."""
        if not self._rs_on_device:
            hi = max(1, int(self.panel.T * 0.5))                                   # :134-138
            self._call("set_random_start", hi, int(self._seed))
            self._rs_on_device = True

    def _before_reset(self):
        if self.random_start:
            self._draw_starts()

    def step(self, actions, out=None):
        if self.random_start and self.auto_reset:
            self._draw_starts()          # fresh starting points for envs that end this step
        return super().step(actions, out)

    def episode_return(self):
        """last logged total assets / initial amount per env (the GainLoss figure, :176), f32."""
        import torch
        return (self.state["logged_total"] / float(self._cfg.initial_amount)).to(torch.float32)


class VecStopLossEnv(VecCashPenaltyEnv):
    """Device-resident batch of the reference's StockTradingEnvStopLoss
    (finrl/meta/env_stock_trading/env_stocktrading_stoploss.py:19-459); extra kwargs
    stoploss_penalty (:73) and profit_loss_ratio (:74)."""
    env_name = "StockTradingEnvStopLoss-MI355X"
    _kind = "stoploss"
    _cfg_cls, _panel_cls, _state_cls = nat.StopLossConfig, nat.StopLossPanelPtrs, \
        nat.StopLossStatePtrs
    _layout = {"f64": (nat.STOPLOSS_F64_FIELDS, nat.STOPLOSS_BOOKS),
               "i32": (nat.STOPLOSS_I32_FIELDS, ())}

    def _extra_cfg(self, stoploss_penalty=0.9, profit_loss_ratio=2):
        min_profit_penalty = 1 + profit_loss_ratio * (1 - stoploss_penalty)      # :101
        return float(stoploss_penalty), float(min_profit_penalty)
