"""Episode history of the batched stock env: the reference's ``asset_memory`` / ``date_memory`` /
``actions_memory`` (env_stocktrading.py:85-97, :332, :348-349) of every env's current episode,
recorded on the device by one small kernel behind each step (finenv_stock_set_history,
include/finenv.h), and the frames everything downstream of the reference env reads, built from ONE
device-to-host copy per tensor.

The frame builders at the top work on host arrays (time-major, as the device holds them) and need
no GPU; ``EpisodeHistory`` owns the device tensors and is what
``VecStockTradingEnv.enable_history()`` returns.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat

METRIC_KEYS = nat.STOCK_HISTORY_METRICS
PORTFOLIO_METRIC_KEYS = nat.PORTFOLIO_HISTORY_METRICS


def _torch():
    import torch
    return torch


# ---------------------------------------------------------------------- frames from host arrays
def _dates(dates, row, length):
    return [dates[int(r)] for r in np.asarray(row)[:int(length)]]


def asset_memory_frame(dates, asset, row, length):
    """save_asset_memory() (:517-525): ``{date, account_value}`` from one env's recorded columns
    (``asset`` / ``row``: at least ``length`` entries; ``dates``: the panel's dates by row)."""
    import pandas as pd
    n = int(length)
    return pd.DataFrame({"date": _dates(dates, row, n),
                         "account_value": np.asarray(asset, dtype=np.float64)[:n].tolist()})


def action_memory_frame(dates, tickers, actions, row, length):
    """save_action_memory() (:527-543) from one env's recorded columns (``actions``: [>= length - 1, N]):
    one column per ticker and the dates as index named ``date`` for N > 1; ``{date, actions}`` with one
    [1] array per day for a single ticker."""
    import pandas as pd
    n = max(int(length) - 1, 0)
    date_list = _dates(dates, row, n)
    acts = np.asarray(actions)[:n].astype(np.int64)
    if acts.shape[1] > 1:
        df_actions = pd.DataFrame(acts)
        df_actions.columns = list(tickers)
        df_actions.index = pd.Index(date_list, name="date")
        return df_actions
    return pd.DataFrame({"date": date_list, "actions": list(acts)})


def account_value_frame(dates, asset, row, length):
    """The frame the terminal branch builds and writes to account_value_*.csv (:230-242):
    ``account_value``, ``date``, ``daily_return = account_value.pct_change(1)``."""
    import pandas as pd
    n = int(length)
    df = pd.DataFrame(np.asarray(asset, dtype=np.float64)[:n].tolist())
    df.columns = ["account_value"]
    df["date"] = _dates(dates, row, n)
    df["daily_return"] = df["account_value"].pct_change(1)
    return df


def validation_sharpe_from(mean, std):
    """get_validation_sharpe (agents/stablebaselines3/models.py:214-230) from the mean and std of the
    daily returns: ``inf`` / ``0.0`` when their variance is 0, else ``4 ** 0.5 * mean / std``."""
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (4 ** 0.5) * mean / std
    return np.where(std * std == 0, np.where(mean > 0, np.inf, 0.0), out)


def portfolio_asset_memory_frame(dates, ret, row, length):
    """StockPortfolioEnv.save_asset_memory() (env_portfolio.py:231-239): ``{date, daily_return}`` from
    one env's recorded columns.  The memory's first entry is the integer 0 of :121, as the reference's
    list holds it."""
    import pandas as pd
    n = int(length)
    r = np.asarray(ret, dtype=np.float64)[:n].tolist()
    if n and r[0] == 0:
        r[0] = 0
    return pd.DataFrame({"date": _dates(dates, row, n), "daily_return": r})


def portfolio_action_memory_frame(dates, tickers, weights, row, length):
    """StockPortfolioEnv.save_action_memory() (:241-252) from one env's recorded columns (``weights``:
    [>= length, N] f32): one float64 column per ticker, the dates as index named ``date``.  Row 0 is
    ``1 / N`` in fp64, as the reference's list holds it (:122), whenever the recorded row is the
    ``float32(1 / N)`` an armed record starts with; later rows are the f32 weights widened."""
    import pandas as pd
    n = int(length)
    w32 = np.asarray(weights, dtype=np.float32)[:n]
    w = w32.astype(np.float64)
    N = w.shape[1]
    if n and (w32[0] == np.float32(1 / N)).all():
        w[0] = 1 / N
    df_actions = pd.DataFrame(w)
    df_actions.columns = list(tickers)
    df_actions.index = pd.Index(_dates(dates, row, n), name="date")
    return df_actions


# ---------------------------------------------------------------------- the device side
def _env_list(e):
    """(single?, [env, ...]) of an env selection: one index, or a sequence of them."""
    one = isinstance(e, (int, np.integer))
    return one, ([int(e)] if one else [int(x) for x in e])


class _Record:
    """What the two device-resident records share: the flag views and the masked arm call (``env``,
    ``flags`` are the subclass's)."""

    @property
    def complete(self):
        """bool [E]: the recorded episode has reported done; the record is final."""
        return (self.flags & nat.HIST_COMPLETE) != 0

    @property
    def overflow(self):
        """bool [E]: the episode outran ``capacity``; the entries below it are right, later days are
        missing."""
        return (self.flags & nat.HIST_OVERFLOW) != 0

    def _arm(self, mask):
        mptr = None
        if mask is not None:
            torch = _torch()
            if not torch.is_tensor(mask):
                mask = torch.from_numpy(np.asarray(mask).astype(np.uint8))
            mask = mask.to(device=self.env.device, dtype=torch.uint8).contiguous()
            mptr = C.c_void_p(mask.data_ptr())
        self.env._call("history_arm", mptr, self.env._stream())


class EpisodeHistory(_Record):
    """Device-resident episode record of a ``VecStockTradingEnv`` (``env.enable_history()``).

    Tensors (time-major; entries at or past ``length[e]`` are unspecified):
      ``asset``    f64 [capacity, E]       asset_memory
      ``row``      i32 [capacity, E]       panel row of each date_memory entry
      ``actions``  i32 [capacity-1, E, N]  actions_memory (realised trades), or None
      ``length``   i32 [E]                 entries recorded; 0 = not armed
      ``flags``    i32 [E]                 bit 0 complete, bit 1 overflow (``complete`` / ``overflow``)

    A record starts when its env is armed -- by the constructor's init, by ``env.reset(mask)`` for the
    envs it resets, or by ``arm(mask)`` from the env's current state -- and ends on the step that
    reports ``done`` (``complete``).  An auto-reset inside ``step`` does not arm: the finished
    episode stays readable until the next host reset or ``arm``.  The pointers are launch arguments, so
    a captured graph records only if the history was enabled before the capture.
    """

    def __init__(self, env, capacity, actions=True):
        torch = _torch()
        E, N = env.num_envs, env.stock_dim
        capacity = int(capacity)
        if capacity < 2:
            raise ValueError("history capacity must be >= 2")
        self.env, self.capacity = env, capacity
        dev = env.device
        self.asset = torch.zeros(capacity, E, dtype=torch.float64, device=dev)
        self.row = torch.zeros(capacity, E, dtype=torch.int32, device=dev)
        self.actions = torch.zeros(capacity - 1, E, N, dtype=torch.int32, device=dev) if actions else None
        self.length = torch.zeros(E, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(E, dtype=torch.int32, device=dev)
        self._metrics = None
        if actions:
            env.enable_realised()
        self._ptrs = nat.StockHistoryPtrs(
            self.asset.data_ptr(), self.row.data_ptr(),
            self.actions.data_ptr() if actions else None,
            self.length.data_ptr(), self.flags.data_ptr(), capacity)
        env._call("set_history", C.byref(self._ptrs))
        self.arm()

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in
                   (self.asset, self.row, self.actions, self.length, self.flags) if t is not None)

    def arm(self, mask=None):
        """Start a new record for every env, or those with mask[e] != 0, from its CURRENT state: one
        entry (asset_memory[0] at the start of an episode, else the current total asset; the current
        date), flags cleared (finenv_stock_history_arm).  No host synchronisation."""
        self._arm(mask)

    def metrics(self, annualization=252 ** 0.5):
        """Backtest figures of the recorded series -> f64 [E, 6] device tensor, columns ``METRIC_KEYS``
        (n_returns, cumulative_return, mean, std, sharpe, max_drawdown); finenv_stock_history_metrics.
        ``252 ** 0.5`` gives the env's terminal printout (:243-251), ``4 ** 0.5``
        get_validation_sharpe's figure.  Sharpe is NaN with fewer than two returns or zero std; rows of
        unarmed envs are NaN.  The tensor is reused by the next call."""
        torch = _torch()
        if self._metrics is None:
            self._metrics = torch.zeros(self.env.num_envs, len(METRIC_KEYS), dtype=torch.float64,
                                        device=self.env.device)
        self.env._call("history_metrics", float(annualization), C.c_void_p(self._metrics.data_ptr()),
                       self.env._stream())
        return self._metrics

    def metrics_dict(self, annualization=252 ** 0.5):
        """``metrics()`` as ``{name: f64 [E] device tensor}``."""
        m = self.metrics(annualization)
        return {k: m[:, j] for j, k in enumerate(METRIC_KEYS)}

    def validation_sharpe(self):
        """get_validation_sharpe (models.py:214-230) of every env's record -> host f64 [E]: ``inf`` /
        ``0.0`` when the variance of the daily returns is 0 (``models.py:220-224``)."""
        m = self.metrics(4 ** 0.5).cpu().numpy()
        return validation_sharpe_from(m[:, METRIC_KEYS.index("mean")], m[:, METRIC_KEYS.index("std")])

    # ------------------------------------------------------------------ frames
    def _host(self, envs, with_actions):
        """Host copies of the selected envs' columns: one device-to-host copy per tensor."""
        torch = _torch()
        idx = torch.as_tensor(envs, dtype=torch.int64, device=self.env.device)
        length = self.length.index_select(0, idx).cpu().numpy()
        asset = self.asset.index_select(1, idx).cpu().numpy()
        row = self.row.index_select(1, idx).cpu().numpy()
        acts = None
        if with_actions:
            if self.actions is None:
                raise nat.FinenvError("this history was enabled with actions=False")
            acts = self.actions.index_select(1, idx).cpu().numpy()
        return length, asset, row, acts

    def _frames(self, e, build, with_actions=False):
        one, envs = _env_list(e)
        length, asset, row, acts = self._host(envs, with_actions)
        out = [build(j, int(length[j]), asset, row, acts) for j in range(len(envs))]
        return out[0] if one else out

    def save_asset_memory(self, e):
        """The reference's save_asset_memory() frame of env ``e`` (a list of frames for a list of
        envs)."""
        dates = self.env.panel.dates
        return self._frames(e, lambda j, n, a, r, _: asset_memory_frame(dates, a[:, j], r[:, j], n))

    def save_action_memory(self, e):
        """The reference's save_action_memory() frame of env ``e`` (a list for a list of envs)."""
        dates, tickers = self.env.panel.dates, self.env.panel.tickers
        return self._frames(
            e, lambda j, n, a, r, acts: action_memory_frame(dates, tickers, acts[:, j], r[:, j], n),
            with_actions=True)

    def account_value_frame(self, e):
        """The frame behind account_value_*.csv of env ``e`` (a list for a list of envs)."""
        dates = self.env.panel.dates
        return self._frames(e, lambda j, n, a, r, _: account_value_frame(dates, a[:, j], r[:, j], n))


class PortfolioEpisodeHistory(_Record):
    """Device-resident episode record of a ``VecStockPortfolioEnv`` (``env.enable_history()``): the
    reference's ``asset_memory`` / ``portfolio_return_memory`` / ``date_memory`` / ``actions_memory``
    (env_portfolio.py:118-123, :168, :190-193), written by the step kernel itself
    (finenv_portfolio_set_history, include/finenv.h).

    Tensors (time-major; entries at or past ``length[e]`` are unspecified), all of the same length:
      ``value``    f64 [capacity, E]     asset_memory
      ``ret``      f64 [capacity, E]     portfolio_return_memory (entry 0 is its leading 0)
      ``row``      i32 [capacity, E]     panel row of each date_memory entry
      ``weights``  f32 [capacity, E, N]  actions_memory (softmax weights; entry 0 is 1/N), or None
      ``length``   i32 [E]               entries recorded; 0 = not armed
      ``flags``    i32 [E]               bit 0 complete, bit 1 overflow (``complete`` / ``overflow``)

    Armed by the constructor (from the env's current state), by ``env.reset(mask)`` for the envs it
    resets and by ``arm(mask)``; final on the step that reports ``done``.  An auto-reset inside ``step``
    does not arm.  The pointers are launch arguments: enable the history before capturing a graph.
    """

    def __init__(self, env, capacity, weights=True):
        torch = _torch()
        E, N = env.num_envs, env.stock_dim
        capacity = int(capacity)
        if capacity < 2:
            raise ValueError("history capacity must be >= 2")
        self.env, self.capacity = env, capacity
        dev = env.device
        self.value = torch.zeros(capacity, E, dtype=torch.float64, device=dev)
        self.ret = torch.zeros(capacity, E, dtype=torch.float64, device=dev)
        self.row = torch.zeros(capacity, E, dtype=torch.int32, device=dev)
        self.weights = torch.zeros(capacity, E, N, dtype=torch.float32, device=dev) if weights else None
        self.length = torch.zeros(E, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(E, dtype=torch.int32, device=dev)
        self._metrics = None
        self._ptrs = nat.PortfolioHistoryPtrs(
            self.value.data_ptr(), self.ret.data_ptr(), self.row.data_ptr(),
            self.weights.data_ptr() if weights else None,
            self.length.data_ptr(), self.flags.data_ptr(), capacity)
        env._call("set_history", C.byref(self._ptrs))
        self.arm()

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in
                   (self.value, self.ret, self.row, self.weights, self.length, self.flags)
                   if t is not None)

    def arm(self, mask=None):
        """Start a new record for every env, or those with mask[e] != 0, from its CURRENT state: one
        entry (the current portfolio value, return 0, the current date, weights 1/N), flags cleared
        (finenv_portfolio_history_arm).  No host synchronisation."""
        self._arm(mask)

    def metrics(self, annualization=252 ** 0.5):
        """Backtest figures of the recorded series -> f64 [E, 6] device tensor, columns
        ``PORTFOLIO_METRIC_KEYS`` (finenv_portfolio_history_metrics): mean / std / Sharpe over the
        recorded returns with their leading 0, as the env's terminal printout takes them (:145-152),
        so ``n_returns`` is ``length`` (one more than the stock env's convention).  Sharpe is NaN with
        fewer than two entries or zero std; rows of unarmed envs are NaN.  Reused by the next call."""
        torch = _torch()
        if self._metrics is None:
            self._metrics = torch.zeros(self.env.num_envs, len(PORTFOLIO_METRIC_KEYS),
                                        dtype=torch.float64, device=self.env.device)
        self.env._call("history_metrics", float(annualization), C.c_void_p(self._metrics.data_ptr()),
                       self.env._stream())
        return self._metrics

    def metrics_dict(self, annualization=252 ** 0.5):
        """``metrics()`` as ``{name: f64 [E] device tensor}``."""
        m = self.metrics(annualization)
        return {k: m[:, j] for j, k in enumerate(PORTFOLIO_METRIC_KEYS)}

    # ------------------------------------------------------------------ frames
    def _host(self, envs, names):
        """Host copies of the selected envs' columns: one device-to-host copy per tensor."""
        torch = _torch()
        idx = torch.as_tensor(envs, dtype=torch.int64, device=self.env.device)
        out = {"length": self.length.index_select(0, idx).cpu().numpy()}
        for k in names:
            t = getattr(self, k)
            if t is None:
                raise nat.FinenvError("this history was enabled with weights=False")
            out[k] = t.index_select(1, idx).cpu().numpy()
        return out

    def save_asset_memory(self, e):
        """The reference's save_asset_memory() frame ``{date, daily_return}`` of env ``e`` (a list of
        frames for a list of envs)."""
        one, envs = _env_list(e)
        h, dates = self._host(envs, ("ret", "row")), self.env.panel.dates
        out = [portfolio_asset_memory_frame(dates, h["ret"][:, j], h["row"][:, j], h["length"][j])
               for j in range(len(envs))]
        return out[0] if one else out

    def save_action_memory(self, e):
        """The reference's save_action_memory() frame of env ``e`` (a list for a list of envs)."""
        one, envs = _env_list(e)
        h = self._host(envs, ("weights", "row"))
        dates, tickers = self.env.panel.dates, self.env.panel.tickers
        out = [portfolio_action_memory_frame(dates, tickers, h["weights"][:, j], h["row"][:, j],
                                             h["length"][j]) for j in range(len(envs))]
        return out[0] if one else out
