"""Device-resident batch of StockPortfolioEnv instances (env_portfolio.py:15-261 in the
reference tree), one HIP launch per step through the C ABI (finenv_portfolio_*)."""
from __future__ import annotations

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
    _panel_cls, _state_cls = nat.PortfolioPanelPtrs, nat.PortfolioStatePtrs
    _layout = {"f64": (nat.PORTFOLIO_F64_FIELDS, ()), "i32": (nat.PORTFOLIO_I32_FIELDS, ())}
    _step_extras = ("term_obs", "weights")
    _last_fields, _last_ratio = nat.PORTFOLIO_LAST_FIELDS, ("begin_value", "end_value")

    if_discrete = False
    env_name = "StockPortfolioEnv-MI355X"
    # names of the last_episode_stats() columns, as the reference prints them (:141-153)
    last_episode_keys = ("begin_total_asset", "end_total_asset", "sharpe")

    def __init__(self, panel: PortfolioPanel, num_envs: int, *, initial_amount=1_000_000,
                 auto_reset=True, device="cuda", windows=None):
        self.panel = panel
        self._set_device(device)
        E, N, K, T = int(num_envs), panel.N, panel.K, panel.T
        self.num_envs = self.env_num = E
        self.stock_dim = self.action_dim = N
        self.state_dim = panel.D
        self.max_step = T - 1
        self.auto_reset = bool(auto_reset)
        self.observation_space = Box(-np.inf, np.inf, (N + K, N), np.float32)   # :99-103
        self.action_space = Box(0.0, 1.0, (N,), np.float32)                      # :96
        self._open(nat.PortfolioConfig(E, N, K, T, float(initial_amount)))
        self._alloc_state(E, N)
        self.state["value"].fill_(float(initial_amount))
        self._panel_t = panel.to_device(self.device)
        self._bind(self._panel_t["gross_ret"], self._panel_t["obs_tmpl"])
        self._alloc_outputs(E, panel.D)
        if windows is not None:
            self.set_windows(*self._check_windows(*windows))
            self.state["day"].copy_(self.windows[0])       # the constructor's episode: day 0 of each window

    def enable_weights(self):
        import torch
        return self._enable_output("weights", self.stock_dim, torch.float32)

    def enable_history(self, capacity=None, weights=True):
        """Record every env's episode on the device: the reference's ``asset_memory``,
        ``portfolio_return_memory``, ``date_memory`` and (with ``weights``) ``actions_memory``
        (:118-123, :168, :190-193), written by the step kernel itself -- no ``state_numpy()`` /
        ``weights.cpu()`` per step, no host loop, and it sits in a captured graph.  Returns the
        ``finrl_amd.history.PortfolioEpisodeHistory`` (also ``self.history``); idempotent: a second call
        returns the same object whatever its arguments.

        ``capacity``: entries per env, by default the longest episode in panel rows (``max_step + 1``:
        ``T``, or the longest window) AS IT IS AT THIS CALL: windows made longer (or detached) by a
        later ``set_windows`` do not grow the tensors, and the longer episodes then end with
        ``overflow`` set and their first ``capacity`` days recorded -- pass ``capacity`` for the longest
        window to come.  Every env is armed from its current state; ``reset(mask)`` re-arms the envs
        it resets, an auto-reset does not (the finished record stays readable).

        Memory: ``E * (20 * capacity + 8) + 4 * E * N * capacity`` bytes.  63-day windows at
        65,536 x DOW30 are 0.08 GB without and 0.58 GB with weights; a full 2,893-day episode at that
        batch is 3.8 GB without and 26.5 GB with, which is why ``weights`` is optional.

        Enable it before capturing a graph (the tensors' addresses are launch arguments)."""
        if self.history is None:
            from .history import PortfolioEpisodeHistory
            self.history = PortfolioEpisodeHistory(
                self, self.max_step + 1 if capacity is None else capacity, weights)
        return self.history

    def _init_last(self, last):
        """While a last-episode block is attached, every step also keeps running return sums
        (``run_sum`` / ``run_sumsq``); they start at 0 for envs on day 0 and at NaN for envs in mid
        episode (whose earlier returns were not kept: that episode's Sharpe reads NaN)."""
        import torch
        fresh = self.window_day() == 0
        for k in ("run_sum", "run_sumsq"):
            j = nat.PORTFOLIO_LAST_FIELDS.index(k)
            last[j] = torch.where(fresh, torch.zeros_like(last[j]), last[j])

    def window_day(self):
        """The reference's ``self.day`` of every env (int32 [E] device tensor): ``state["day"]`` minus
        the env's window start in ``self.windows`` (``state["day"]`` without windows)."""
        if self.windows is None:
            return self.state["day"].clone()
        return self.state["day"] - self.windows[0]

    def episode_return(self):
        """portfolio value / initial amount per env, f32 (the quantity gathered across ranks)."""
        import torch
        return (self.state["value"] / float(self._cfg.initial_amount)).to(torch.float32)

    def state_numpy(self):
        out = super().state_numpy()
        out["window_day"] = self.window_day().cpu().numpy()
        return out
