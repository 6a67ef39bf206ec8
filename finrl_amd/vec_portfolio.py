"""Device-resident batch of StockPortfolioEnv instances (env_portfolio.py:15-261 in the
reference tree), one HIP launch per step through the C ABI (finenv_portfolio_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat
from .panel import PortfolioPanel
from .spaces import Box
from .vec_env import _EpisodeWindows


class VecStockPortfolioEnv(_EpisodeWindows):
    """E parallel StockPortfolioEnv.  step(actions f32 [E,N]) -> (obs f32 [E, N+K, N] flattened
    to [E, D], reward f32 [E] = new portfolio value (:196), done u8 [E], None).

    ``windows=(start, end)`` gives every env its own episode window of panel rows ``[start, end)``
    (one pair for all envs, or [E] arrays / tensors): env e then behaves like the reference env
    built on ``data_split(df, dates[start[e]], dates[end[e]])`` -- the tutorial's train and trade
    slices, or random training windows, in ONE batch over one panel.  ``state["day"]`` stays the
    panel row; ``window_day()`` is the reference's ``self.day``.  See ``set_windows``: as in
    VecStockTradingEnv an edited start applies at the env's next reset.  The portfolio state keeps
    no start day, so ``window_day()`` and the last-episode latch count from the start in
    ``self.windows``: an episode whose start was edited before it ended, and that was not reset
    since, is out of contract (``set_windows(s, t, mask=done)`` then ``reset(done)`` is exact).
    """

    _kind = "portfolio"

    if_discrete = False
    env_name = "StockPortfolioEnv-MI355X"
    # names of the last_episode_stats() columns, as the reference prints them (:141-153)
    last_episode_keys = ("begin_total_asset", "end_total_asset", "sharpe")

    def __init__(self, panel: PortfolioPanel, num_envs: int, *, initial_amount=1_000_000,
                 auto_reset=True, device="cuda", windows=None):
        import torch
        self.panel = panel
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.FinenvError("finrl_amd has no CPU path: device must be a HIP GPU")
        E, N, K, T = int(num_envs), panel.N, panel.K, panel.T
        self.num_envs = self.env_num = E
        self.stock_dim = self.action_dim = N
        self.state_dim = panel.D
        self.max_step = T - 1
        self.auto_reset = bool(auto_reset)
        self.observation_space = Box(-np.inf, np.inf, (N + K, N), np.float32)   # :99-103
        self.action_space = Box(0.0, 1.0, (N,), np.float32)                      # :96
        L = nat.lib()
        self._cfg = nat.PortfolioConfig(E, N, K, T, float(initial_amount))
        self._h = C.c_void_p()
        nat.check(L.finenv_portfolio_create(C.byref(self._cfg), C.byref(self._h)), None,
                  "finenv_portfolio_create")
        dev = self.device
        self._f64 = torch.zeros(len(nat.PORTFOLIO_F64_FIELDS), E, dtype=torch.float64, device=dev)
        self._i32 = torch.zeros(len(nat.PORTFOLIO_I32_FIELDS), E, dtype=torch.int32, device=dev)
        self.state = {k: self._f64[j] for j, k in enumerate(nat.PORTFOLIO_F64_FIELDS)}
        self.state.update({k: self._i32[j] for j, k in enumerate(nat.PORTFOLIO_I32_FIELDS)})
        self.state["value"].fill_(float(initial_amount))
        self._panel_t = panel.to_device(dev)
        pp = nat.PortfolioPanelPtrs(self._panel_t["gross_ret"].data_ptr(),
                                    self._panel_t["obs_tmpl"].data_ptr())
        sp = nat.PortfolioStatePtrs(self._f64.data_ptr(), self._i32.data_ptr())
        nat.check(L.finenv_portfolio_bind(self._h, C.byref(pp), C.byref(sp)), self._h, "bind",
                  "portfolio")
        self.obs = torch.zeros(E, panel.D, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(E, dtype=torch.float32, device=dev)
        self.done = torch.zeros(E, dtype=torch.uint8, device=dev)
        self.term_obs = None
        self.weights = None
        self._last = None
        self._last_stats = None
        self.last_episode = None
        self.windows = None
        if windows is not None:
            self.set_windows(*self._check_windows(*windows))
            self.state["day"].copy_(self.windows[0])       # the constructor's episode: day 0 of each window

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                nat.lib().finenv_portfolio_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def enable_terminal_obs(self):
        import torch
        if self.term_obs is None:
            self.term_obs = torch.zeros_like(self.obs)
        return self.term_obs

    def enable_weights(self):
        import torch
        if self.weights is None:
            self.weights = torch.zeros(self.num_envs, self.stock_dim, dtype=torch.float32,
                                       device=self.device)
        return self.weights

    def enable_last_episode(self):
        """Attach a last-episode block (finenv_portfolio_set_last_episode), f64
        [FINENV_PORTFOLIO_LAST_FIELDS, E] on the device, viewed by name in ``self.last_episode``:
        the terminal step latches begin / end value and the daily-return sums of the finished
        episode before an auto-reset.  While attached, every step also keeps running return sums
        (``run_sum`` / ``run_sumsq``); they start at 0 for envs on day 0 and at NaN for envs in mid
        episode (whose earlier returns were not kept: that episode's Sharpe reads NaN).
        Idempotent; as for the stock env, a captured step sees the block only if it was enabled
        before the capture."""
        import torch
        if self._last is None:
            last = torch.full((len(nat.PORTFOLIO_LAST_FIELDS), self.num_envs), float("nan"),
                              dtype=torch.float64, device=self.device)
            last[0].zero_()
            fresh = self.window_day() == 0
            for k in ("run_sum", "run_sumsq"):
                j = nat.PORTFOLIO_LAST_FIELDS.index(k)
                last[j] = torch.where(fresh, torch.zeros_like(last[j]), last[j])
            nat.check(nat.lib().finenv_portfolio_set_last_episode(self._h, C.c_void_p(last.data_ptr())),
                      self._h, "set_last_episode", "portfolio")
            self._last = last
            self.last_episode = {k: last[j] for j, k in enumerate(nat.PORTFOLIO_LAST_FIELDS)}
        return self._last

    def last_episode_stats(self):
        """{begin_total_asset, end_total_asset, sharpe} of each env's last finished episode -> f64
        [E, 3] device tensor (NaN rows where none has finished).  Needs enable_last_episode()."""
        import torch
        if self._last is None:
            raise nat.FinenvError("last_episode_stats: call enable_last_episode() first")
        if self._last_stats is None:
            self._last_stats = torch.zeros(self.num_envs, 3, dtype=torch.float64, device=self.device)
        nat.check(nat.lib().finenv_portfolio_last_episode_stats(
            self._h, C.c_void_p(self._last_stats.data_ptr()), self._stream()), self._h,
            "last_episode_stats", "portfolio")
        return self._last_stats

    def last_episode_return(self):
        """end / begin value of each env's last finished episode, f32 [E] (NaN where none has
        finished); same shape and dtype as episode_return()."""
        import torch
        if self._last is None:
            raise nat.FinenvError("last_episode_return: call enable_last_episode() first")
        le = self.last_episode
        return (le["end_value"] / le["begin_value"]).to(torch.float32)

    def window_day(self):
        """The reference's ``self.day`` of every env (int32 [E] device tensor): ``state["day"]`` minus
        the env's window start in ``self.windows`` (``state["day"]`` without windows)."""
        if self.windows is None:
            return self.state["day"].clone()
        return self.state["day"] - self.windows[0]

    def reset(self, mask=None):
        import torch
        mptr = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mptr = C.c_void_p(mask.data_ptr())
        nat.check(nat.lib().finenv_portfolio_reset(self._h, mptr, C.c_void_p(self.obs.data_ptr()),
                                                   self._stream()), self._h, "reset", "portfolio")
        return self.obs

    def step(self, actions, out=None):
        import torch
        if actions.dtype != torch.float32 or not actions.is_contiguous() or \
                actions.device != self.obs.device:
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        obs, rew, done = out if out is not None else (self.obs, self.reward, self.done)
        nat.check(nat.lib().finenv_portfolio_step(
            self._h, C.c_void_p(actions.data_ptr()), C.c_void_p(obs.data_ptr()),
            C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()),
            C.c_void_p(self.term_obs.data_ptr()) if self.term_obs is not None else None,
            C.c_void_p(self.weights.data_ptr()) if self.weights is not None else None,
            int(self.auto_reset), self._stream()), self._h, "step", "portfolio")
        return obs, rew, done, None

    def as_sb3_vec_env(self):
        """stable-baselines3 VecEnv-shaped view (numpy in / out, auto-reset, terminal_observation)."""
        from .vec_env import SB3VecEnvAdapter
        return SB3VecEnvAdapter(self)

    def episode_return(self):
        """portfolio value / initial amount per env, f32 (the quantity gathered across ranks)."""
        import torch
        return (self.state["value"] / float(self._cfg.initial_amount)).to(torch.float32)

    def state_numpy(self):
        out = {k: v.detach().cpu().numpy() for k, v in self.state.items()}
        out["window_day"] = self.window_day().cpu().numpy()
        return out
