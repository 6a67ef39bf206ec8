"""Device-resident batch of StockTradingEnv instances (one HIP launch per step).

``VecStockTradingEnv`` is tensor-in / tensor-out (the ElegantRL vectorised-env shape:
``env_num, state_dim, action_dim, max_step, if_discrete, target_return``);
``SB3VecEnvAdapter`` presents the same batch through the stable-baselines3 ``VecEnv``
protocol (numpy in / numpy out, auto-reset with ``info["terminal_observation"]``), which is
what the reference builds with ``DummyVecEnv([lambda: env])`` (env_stocktrading.py:549-552).

All arithmetic happens in finrl_amd/csrc/finenv_stock.hip through the C ABI; this module
only owns the torch tensors that back the state and hands their pointers over.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat
from .panel import StockPanel
from .spaces import Box
from .vec_base import BatchedEnv, WindowedEnv


def _torch():
    import torch
    return torch


def _indices(env, indices):
    """SB3 ``VecEnv._get_indices`` over ``env.num_envs``: None -> all envs, int -> [int], else the
    iterable."""
    if indices is None:
        return list(range(env.num_envs))
    if isinstance(indices, (int, np.integer)):
        return [int(indices)]
    return [int(i) for i in indices]


class _EpisodeWindows(WindowedEnv):
    """Per-env episode windows (vec_base.WindowedEnv) and the last-episode latch of a panel-driven
    batch: the host side shared by VecStockTradingEnv and VecStockPortfolioEnv (``num_envs``,
    ``panel.T`` and ``max_step`` are theirs).  ``_last_fields`` is the kind's last-episode block
    layout, ``_last_ratio`` its (begin, end) fields and ``last_episode_keys`` the
    last_episode_stats() columns."""

    history = None              # enable_history() of the subclass
    _last = _last_stats = last_episode = None
    _last_fields, _last_ratio, last_episode_keys = (), ("", ""), ()

    def _history(self, what):
        """The episode history (enable_history() of the subclass), or FinenvError."""
        if self.history is None:
            raise nat.FinenvError(f"{what}: call enable_history() first")
        return self.history

    def save_asset_memory(self, indices=None):
        """The reference's save_asset_memory() frames (env_stocktrading.py:517-525; for the portfolio env
        ``{date, daily_return}``, env_portfolio.py:231-239), one per selected env (all by default).
        Always a list, also for a single index (``self.history.save_asset_memory(e)`` gives the bare
        frame).  Needs enable_history()."""
        return self._history("save_asset_memory").save_asset_memory(_indices(self, indices))

    def save_action_memory(self, indices=None):
        """The reference's save_action_memory() frames (env_stocktrading.py:527-543,
        env_portfolio.py:241-252), one per selected env (all by default; always a list).  Needs
        enable_history() with actions / weights."""
        return self._history("save_action_memory").save_action_memory(_indices(self, indices))

    def _init_last(self, last):
        """Hook: edit a new last-episode block before it is attached."""

    def enable_last_episode(self):
        """Attach a last-episode block (finenv_<kind>_set_last_episode): from now on the step that
        reports done latches the finished episode's summary -- before an auto-reset replaces the
        state -- into a caller-owned f64 [_last_fields, E] device tensor, returned here and viewed
        by name in ``self.last_episode``.  ``count`` starts at 0 and every other field at NaN.
        Idempotent: a second call returns the same tensor.  The block's pointer is a step-kernel
        argument, so a step captured into a graph writes the block only if it was enabled before
        the capture."""
        torch = _torch()
        if self._last is None:
            last = torch.full((len(self._last_fields), self.num_envs), float("nan"),
                              dtype=torch.float64, device=self.device)
            last[0].zero_()
            self._init_last(last)
            self._call("set_last_episode", C.c_void_p(last.data_ptr()))
            self._last = last
            self.last_episode = {k: last[j] for j, k in enumerate(self._last_fields)}
        return self._last

    def last_episode_stats(self):
        """``last_episode_keys`` of each env's last FINISHED episode -> f64 [E, len(keys)] device
        tensor (rows of envs that have not finished one yet are NaN).  Needs enable_last_episode()."""
        torch = _torch()
        if self._last is None:
            raise nat.FinenvError("last_episode_stats: call enable_last_episode() first")
        if self._last_stats is None:
            self._last_stats = torch.zeros(self.num_envs, len(self.last_episode_keys),
                                           dtype=torch.float64, device=self.device)
        self._call("last_episode_stats", C.c_void_p(self._last_stats.data_ptr()), self._stream())
        return self._last_stats

    def last_episode_return(self):
        """end / begin total asset of each env's last finished episode, f32 [E] (NaN where none has
        finished): what episode_return() reports for the current episode, for the one an auto-reset
        has already replaced -- the quantity to gather across ranks."""
        if self._last is None:
            raise nat.FinenvError("last_episode_return: call enable_last_episode() first")
        begin, end = self._last_ratio
        return (self.last_episode[end] / self.last_episode[begin]).to(_torch().float32)


class VecStockTradingEnv(_EpisodeWindows):
    """E parallel copies of the reference ``StockTradingEnv`` (env_stocktrading.py:19-552).

    Constructor keywords keep the reference's names (``hmax, initial_amount,
    num_stock_shares, buy_cost_pct, sell_cost_pct, reward_scaling, turbulence_threshold,
    day, initial``).  ``initial_amount`` / ``num_stock_shares`` may be per-env
    ([E] / [E, N]) which also covers the ``previous_state`` carry-over (:423-450).
    Costs are scalars, as in this fork (:118, :179).

    ``windows=(start, end)`` gives every env its own episode window of panel rows ``[start, end)``
    (one pair for all envs, or [E] arrays / tensors): env e then behaves like the reference env
    built on ``data_split(df, dates[start[e]], dates[end[e]])`` -- K ensemble windows or random
    training windows in ONE batch over one panel.  ``day`` counts from each window's start.
    ``state["day"]`` stays the panel row; ``window_day()`` is the reference's ``self.day``.
    See ``set_windows``.
    """

    if_discrete = False
    env_name = "StockTradingEnv-MI355X"
    target_return = 10.0
    # names of the last_episode_stats() columns, as the reference prints them (:257-264)
    last_episode_keys = ("begin_total_asset", "end_total_asset", "total_reward", "total_cost",
                         "total_trades", "sharpe")

    _kind = "stock"
    _panel_cls, _state_cls = nat.StockPanelPtrs, nat.StockStatePtrs
    # two [field][E] blocks (include/finenv.h); holdings and shares0 are [N][E] books of the i32 one
    _layout = {"f64": (nat.STOCK_F64_FIELDS, ()),
               "i32": (nat.STOCK_I32_FIELDS, ("holdings", "shares0"))}
    _step_extras = ("term_obs", "realised")
    _pitched = True
    _last_fields, _last_ratio = nat.STOCK_LAST_FIELDS, ("begin_asset", "end_asset")
    _stats = None
    # the stock env's own names of its two state blocks, kept for code that reads them
    _state_f64 = property(lambda self: self._f64)
    _state_i32 = property(lambda self: self._i32)

    def __init__(self, panel: StockPanel, num_envs: int, *, hmax=100,
                 initial_amount=1_000_000, num_stock_shares=None, buy_cost_pct=1e-3,
                 sell_cost_pct=1e-3, reward_scaling=1e-4, turbulence_threshold=None,
                 day=0, initial=True, reset_quirk=True, track_stats=True, auto_reset=True,
                 device="cuda", obs_pitch=None, windows=None):
        torch = _torch()
        if not isinstance(buy_cost_pct, (int, float)) or not isinstance(sell_cost_pct, (int, float)):
            # the fork's own env raises TypeError on list costs
            raise TypeError("buy_cost_pct / sell_cost_pct must be scalars in this fork")
        self.panel = panel
        self._set_device(device)
        E, N, K, T = int(num_envs), panel.N, panel.K, panel.T
        self.num_envs = self.env_num = E
        self.stock_dim = self.action_dim = N
        self.state_dim = self.state_space = panel.D
        self.max_step = T - 1
        self.hmax = int(hmax)
        self.reward_scaling = float(reward_scaling)
        self.turbulence_threshold = turbulence_threshold
        self.auto_reset = bool(auto_reset)
        self.observation_space = Box(-np.inf, np.inf, (panel.D,), np.float32)
        self.action_space = Box(-1.0, 1.0, (N,), np.float32)

        self._open(nat.StockConfig(
            E, N, K, T, self.hmax, int(turbulence_threshold is not None), int(bool(reset_quirk)),
            int(bool(initial)), int(bool(track_stats)),
            int(N == 1),      # one ticker in the frame: the reference's single-stock branches (:415-422)
            float(buy_cost_pct),
            float(sell_cost_pct), float(reward_scaling),
            float(turbulence_threshold) if turbulence_threshold is not None else 0.0))
        cash0 = np.broadcast_to(np.asarray(initial_amount, dtype=np.float64), (E,))
        if num_stock_shares is None:
            num_stock_shares = np.zeros(N, dtype=np.int64)
        sh0 = np.broadcast_to(np.asarray(num_stock_shares, dtype=np.int64), (E, N))
        self._alloc_state(E, N)
        self.state["cash0"].copy_(torch.from_numpy(np.array(cash0, dtype=np.float64)))
        self.state["shares0"].copy_(torch.from_numpy(np.ascontiguousarray(sh0.T).astype(np.int32)))
        self._panel_t = panel.to_device(self.device)
        self._bind(*(self._panel_t[k] for k in ("close", "obs_tmpl", "risk")))
        # obs rows start on 64-byte boundaries unless obs_pitch="packed" / an explicit pitch is
        # given (vec_base.obs_pitch_for)
        self._alloc_outputs(E, panel.D, obs_pitch)
        self._day0 = int(day)
        if windows is not None:
            start, end = windows
            s_np, t_np = self._check_windows(start, end)
            if not 0 <= self._day0 < int((t_np - s_np).min()):
                raise ValueError(f"day={day} does not fit the shortest window "
                                 f"({int((t_np - s_np).min())} days)")
            self.set_windows(s_np, t_np)
        self._call("init", int(day), self._stream())

    close = BatchedEnv.__del__

    def window_day(self):
        """The reference's ``self.day`` of every env (int32 [E] device tensor): ``state["day"]`` minus
        the panel row its window started on when the episode began.  A reset sets ``start_day`` to
        that row; the constructor's episode began ``day`` rows later.  Without windows it equals
        ``state["day"]``."""
        st = self.state
        return st["day"] - st["start_day"] + self._day0 * (st["episode"] == 0).to(st["day"].dtype)

    def hint_desynchronised(self, on=True):
        """Performance hint (results never depend on it): the envs of this batch sit on different
        days -- per-env start days, staggered episode ends, windows with different starts.  Selects
        the step-kernel instantiation tuned for per-env panel rows (finenv_stock_set_desync_hint)."""
        self._call("set_desync_hint", int(bool(on)))

    def enable_realised(self):
        return self._enable_output("realised", self.stock_dim, _torch().int32)

    def enable_history(self, capacity=None, actions=True):
        """Record every env's episode on the device: the reference's ``asset_memory``,
        ``date_memory`` and (with ``actions``) ``actions_memory`` (:85-97, :332, :348-349), written by
        one small kernel behind each step -- no ``state_numpy()`` per step, no host loop, and it sits
        in a captured graph.  Returns the ``finrl_amd.history.EpisodeHistory`` (also
        ``self.history``); idempotent like ``enable_last_episode``: a second call returns the same
        object whatever its arguments.

        ``capacity``: entries per env, by default the longest episode in panel rows (``T``, or the
        longest window).  Every env is armed from its current state; ``reset(mask)`` re-arms the envs
        it resets, an auto-reset does not (the finished record stays readable), see EpisodeHistory.
        With ``actions`` the ``realised`` step output is enabled too.

        Memory: ``E * (12 * capacity + 8) + 4 * E * N * (capacity - 1)`` bytes.  63-day windows at
        65,536 x DOW30 are 0.05 GB without and 0.54 GB with actions; a full 2,893-day episode at that
        batch is 2.3 GB without and 25 GB with, which is why ``actions`` is optional.

        Enable it before capturing a graph (the tensors' addresses are launch arguments).  A
        ``GraphedSegment`` restores only the env's state blocks after its warm-up steps, so a history
        enabled before the segment is built has recorded the warm-up: build the segment, then
        ``history.arm()``."""
        if self.history is None:
            from .history import EpisodeHistory
            self.history = EpisodeHistory(
                self, self.max_step + 1 if capacity is None else capacity, actions)
        return self.history

    # ------------------------------------------------------------------ env protocol
    # reset() (:359-393) and step() (:220-357) are BatchedEnv's
    def refresh(self):
        """Call after editing ``state["cash"]`` / ``state["holdings"]`` / ``state["price_day"]`` in
        place: re-evaluates the carried begin asset (``state["begin_asset"]``) that ``step`` uses
        for the next reward instead of recomputing it (finenv_stock_refresh)."""
        self._call("refresh", self._stream())

    def observe(self):
        """render() (:395-396): current observation without stepping."""
        self._use_pitch(self._pitch)
        self._call("observe", C.c_void_p(self.obs.data_ptr()), self._stream())
        return self.obs

    # ------------------------------------------------------------------ introspection
    def episode_stats(self):
        """Terminal-branch summary (:226-264) -> f64 [E, 6] device tensor:
        begin_total_asset, end_total_asset, total_reward, total_cost, total_trades, sharpe."""
        torch = _torch()
        if self._stats is None:
            self._stats = torch.zeros(self.num_envs, 6, dtype=torch.float64, device=self.device)
        self._call("episode_stats", C.c_void_p(self._stats.data_ptr()), self._stream(), what="stats")
        return self._stats

    def total_asset(self):
        return self.episode_stats()[:, 1]

    def episode_return(self):
        """end_total_asset / begin_total_asset per env (the quantity gathered across ranks)."""
        st = self.episode_stats()
        return (st[:, 1] / st[:, 0]).to(_torch().float32)

    def state_numpy(self):
        """Host copy of the per-env state (synchronises)."""
        out = super().state_numpy()
        out["window_day"] = self.window_day().cpu().numpy()
        out["shares"] = out.pop("holdings")
        return out


class SB3VecEnvAdapter:
    """stable-baselines3 ``VecEnv``-shaped view of a VecStockTradingEnv.

    SB3 itself is not vendored in the reference (setup.py:34-36) nor installed here, so this
    follows its documented public behaviour: ``reset() -> float32 [E, D]``;
    ``step_wait() -> (obs f32 [E, D], rewards f32 [E], dones bool [E], infos list[dict])``
    with auto-reset and ``infos[i]["terminal_observation"]``.
    """

    def __init__(self, env):
        """env: any of the batched envs of this package (they share the tensor protocol:
        ``reset()``, ``step(a) -> (obs, reward, done, _)``, ``enable_terminal_obs()``).  Envs with
        a last-episode block (stock, portfolio) get it enabled here, and every done env's info then
        carries ``"episode_summary"``: the reference's terminal printout (begin / end total asset,
        total reward, cost, trades, Sharpe; NaN where it prints none) under its names.  (SB3's own
        ``"episode"`` key is Monitor's sum of the scaled rewards, a different quantity.)"""
        self.env = env
        env.auto_reset = True
        env.enable_terminal_obs()
        self._summary_keys = None
        if hasattr(env, "enable_last_episode"):
            env.enable_last_episode()
            self._summary_keys = env.last_episode_keys
        self.num_envs = env.num_envs
        self.observation_space = env.observation_space
        self.action_space = env.action_space
        self._actions = None
        self.render_mode = None

    def reset(self):
        return self.env.reset().cpu().numpy()

    def step_async(self, actions):
        self._actions = actions

    def step_wait(self):
        torch = _torch()
        a = self._actions
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        a = a.to(self.env.device, non_blocking=True)
        obs, rew, done, _ = self.env.step(a)
        obs_h = obs.cpu().numpy()
        rew_h = rew.cpu().numpy()
        done_h = done.cpu().numpy().astype(bool)
        infos = [{} for _ in range(self.num_envs)]
        if done_h.any():
            idx = np.nonzero(done_h)[0]
            idx_t = torch.from_numpy(idx).to(self.env.device)
            term = self.env.term_obs[idx_t].cpu().numpy()
            for j, i in enumerate(idx):
                infos[i]["terminal_observation"] = term[j]
            if self._summary_keys is not None:
                summ = self.env.last_episode_stats()[idx_t].cpu().numpy()
                for j, i in enumerate(idx):
                    infos[i]["episode_summary"] = {k: float(v) for k, v in
                                                   zip(self._summary_keys, summ[j])}
        return obs_h, rew_h, done_h, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        pass

    def seed(self, seed=None):
        return [seed] * self.num_envs

    def render(self, mode="human"):
        obs = self.env.observe() if hasattr(self.env, "observe") else self.env.obs
        return obs.cpu().numpy()

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(_indices(self, indices))

    def get_attr(self, attr_name, indices=None):
        v = getattr(self.env, attr_name)
        return [v] * len(_indices(self, indices))

    def set_attr(self, attr_name, value, indices=None):
        setattr(self.env, attr_name, value)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        """SB3's public signature (the reference calls ``env_method(method_name=...)``,
        agents/stablebaselines3/models.py:120-121).  The batch is one object, so the method
        runs once and its result is repeated per selected env."""
        r = getattr(self.env, method_name)(*method_args, **method_kwargs)
        return [r] * len(_indices(self, indices))


class SingleEnvVecAdapter:
    """``DummyVecEnv([lambda: env])``-shaped wrapper around one of the single-env facades
    (what the reference's ``get_sb_env`` returns, env_stocktrading.py:549-552): SB3's documented
    VecEnv behaviour -- observation / reward buffers in the spaces' dtype (float32), auto-reset
    on done with ``infos[0]["terminal_observation"]``, ``env_method(method_name, ...)``,
    ``get_attr / set_attr(..., indices)``, ``seed``, ``env_is_wrapped``.  SB3 is not vendored
    in the reference (setup.py:34-36), so this boundary is parity unpinned upstream; the tests
    drive it with the reference's own caller loop (agents/stablebaselines3/models.py:110-129)."""

    def __init__(self, env):
        self.env = env
        self.envs = [env]
        self.num_envs = 1
        self.observation_space = env.observation_space
        self.action_space = env.action_space
        self._actions = None
        self.render_mode = None
        self._obs_dtype = np.dtype(getattr(env.observation_space, "dtype", np.float32))

    def _obs(self, obs):
        return np.asarray(obs, dtype=self._obs_dtype)[None].copy()

    def reset(self):
        return self._obs(self.env.reset())

    def step_async(self, actions):
        self._actions = np.asarray(actions)

    def step_wait(self):
        obs, rew, done, info = self.env.step(self._actions[0])
        info = dict(info) if isinstance(info, dict) else {}
        if done:
            info["terminal_observation"] = np.asarray(obs, dtype=self._obs_dtype)
            obs = self.env.reset()
        return (self._obs(obs), np.asarray([rew], dtype=np.float32),
                np.asarray([done], dtype=bool), [info])

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def _indices(self, indices):
        if indices is None:
            return [0]
        if isinstance(indices, (int, np.integer)):
            indices = [indices]
        idx = [int(i) for i in indices]
        if any(i != 0 for i in idx):
            raise IndexError(f"indices {idx}: this VecEnv holds one env")
        return idx

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        return [getattr(self.env, method_name)(*method_args, **method_kwargs)
                for _ in self._indices(indices)]

    def get_attr(self, attr_name, indices=None):
        return [getattr(self.env, attr_name) for _ in self._indices(indices)]

    def set_attr(self, attr_name, value, indices=None):
        for _ in self._indices(indices):
            setattr(self.env, attr_name, value)

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False for _ in self._indices(indices)]

    def seed(self, seed=None):
        fn = getattr(self.env, "seed", None) or getattr(self.env, "_seed", None)
        return [fn(seed) if fn is not None else None]

    def render(self, mode="human"):
        return self.env.render(mode) if hasattr(self.env, "render") else None

    def close(self):
        pass
