"""Episode history of the batched stock env: the reference's ``asset_memory`` / ``date_memory`` /
``actions_memory`` (env_stocktrading.py:85-97, :332, :348-349) of every env's current episode,
recorded on the device by one small kernel behind each step (finenv_stock_set_history,
include/finenv.h), and the frames everything downstream of the reference env reads, built from ONE
device-to-host copy per tensor.

The frame builders at the top work on host arrays (time-major, as the device holds them) and need
no GPU; ``EpisodeHistory`` owns the device tensors and is what
``VecStockTradingEnv.enable_history()`` returns.  ``PortfolioEpisodeHistory``,
``CryptoEpisodeHistory`` and ``StockNpEpisodeHistory`` are the same for the portfolio, the crypto and
the array-state stock env, whose step kernels write the record themselves; ``TwoWaveEpisodeHistory``
is the record of the cash-penalty and stop-loss envs, a copy of their audit rows taken by one small
kernel behind each step.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat

METRIC_KEYS = nat.STOCK_HISTORY_METRICS
PORTFOLIO_METRIC_KEYS = nat.PORTFOLIO_HISTORY_METRICS
CRYPTO_METRIC_KEYS = nat.CRYPTO_HISTORY_METRICS
STOCKNP_METRIC_KEYS = nat.STOCKNP_HISTORY_METRICS
TWOWAVE_METRIC_KEYS = nat.TWOWAVE_HISTORY_METRICS


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


def crypto_account_values(asset, length):
    """The true account value of one crypto env's recorded episode: ``total_asset`` after every step
    (env_multiple_crypto.py:82-84), entry 0 the value the episode started with -> f64 [length]."""
    return np.array(np.asarray(asset, dtype=np.float64)[:int(length)])


def crypto_episode_total_assets(holdings, length, initial_total_asset):
    """The list DRLAgent.DRL_prediction_load_from_file returns (agents/stablebaselines3/models.py:146-156)
    from one env's recorded ``holdings`` column, as Python floats: ``[initial_total_asset]`` and then
    ``initial_total_asset + holdings[k]`` per step.  The reference adds the value of the holdings to
    ``initial_total_asset`` where the remaining cash belongs (models.py:152-155), so this is not the
    account value (``crypto_account_values``) once anything was bought; it is reproduced as it is."""
    init = float(initial_total_asset)
    h = np.asarray(holdings, dtype=np.float64)[1:max(int(length), 1)]
    return [init] + [init + float(x) for x in h]


def crypto_positions(stocks, length):
    """One crypto env's holdings after every recorded entry -> f32 [length, N] (``stocks``: [>= length, N])."""
    return np.array(np.asarray(stocks, dtype=np.float32)[:int(length)])


def crypto_rows(start, length):
    """The panel row of every recorded entry of one crypto env: ``start + arange(length)`` (the env
    moves one row per step), for indexing the caller's own timestamps."""
    return int(start) + np.arange(int(length), dtype=np.int64)


# the scalar type behind each FINENV_NT_* tag of the array-state env (include/finenv.h)
_STOCKNP_SCALARS = (float, np.float32, np.float64)


def stocknp_account_values(asset, length):
    """One array-state env's recorded account curve: ``total_asset`` after every step
    (env_stocktrading_np.py:137), entry 0 the value the record was armed on -> f64 [length]."""
    return np.array(np.asarray(asset, dtype=np.float64)[:int(length)])


def stocknp_episode_total_assets(asset, tag, length):
    """The list DRLAgent.DRL_prediction returns (agents/elegantrl/models.py:107-131) from one env's
    recorded ``asset`` and ``tag`` columns: element k is the scalar the reference's list holds there
    under NumPy >= 2 -- ``float``, ``np.float32`` or ``np.float64`` by its FINENV_NT_* tag (a float32
    total_asset is recorded widened, so the conversion back is exact).  ``tag`` None (not recorded):
    Python floats."""
    n = int(length)
    a = np.asarray(asset, dtype=np.float64)[:n].tolist()
    if tag is None:
        return a
    return [_STOCKNP_SCALARS[t](x) for x, t in zip(a, np.asarray(tag)[:n].tolist())]


def stocknp_episode_returns(asset, tag, length):
    """``episode_returns`` of the same loop (models.py:124): ``total_asset / initial_total_asset`` for
    every entry k >= 1 over entry 0, each quotient in the dtype NumPy >= 2 promotes the two scalars to
    (a Python float defers to a NumPy scalar, float64 beats float32) -- the reference's list when the
    record was armed at the episode's start.  ``tag`` None: float64 quotients as Python floats."""
    vals = stocknp_episode_total_assets(asset, tag, length)
    if not vals:
        return []
    first, out = vals[0], []
    for x in vals[1:]:
        kinds = {type(x), type(first)}
        kind = np.float64 if np.float64 in kinds else (np.float32 if np.float32 in kinds else float)
        out.append(kind(kind(x) / kind(first)))
    return out


def _own_dates(dates, end, length):
    """The ``date`` column of the cash-penalty / stop-loss frames: ``self.dates[-len(cash):]``
    (env_stocktrading_cashpenalty.py:395, :405) -- the LAST ``length`` dates of the env's own frame,
    ``dates[end - length:end]`` of the panel's, whatever dates the entries were recorded on."""
    return list(dates[int(end) - int(length):int(end)])


def dollar_asset_memory_frame(dates, cash, asset_value, reward, end, length):
    """save_asset_memory() of the cash-penalty and stop-loss envs (env_stocktrading_cashpenalty.py:390-397,
    env_stocktrading_stoploss.py:444-451) from one env's recorded columns: ``account_information`` with
    ``total_assets = cash + asset_value`` as the reference forms it (:314) and the ``date`` column of
    ``_own_dates``; None for an empty record (``current_step == 0``)."""
    import pandas as pd
    n = int(length)
    if n == 0:
        return None
    cash = np.asarray(cash, dtype=np.float64)[:n]
    asset_value = np.asarray(asset_value, dtype=np.float64)[:n]
    info = {"cash": cash.tolist(), "asset_value": asset_value.tolist(),
            "total_assets": (cash + asset_value).tolist(),
            "reward": np.asarray(reward, dtype=np.float64)[:n].tolist()}
    info["date"] = _own_dates(dates, end, n)
    return pd.DataFrame(info)


def stoploss_actions_memory(raw, hmax, close_rows):
    """What the stop-loss env appends to ``actions_memory`` (env_stocktrading_stoploss.py:321-324):
    ``(actions * hmax) * closings`` from the raw float32 action rows [n, N] and the close rows [n, N]
    of the entries' dates -- the product with ``hmax`` in float32, as the caller's array makes it, the
    one with the float64 closings in float64."""
    return (np.asarray(raw, dtype=np.float32) * hmax) * np.asarray(close_rows, dtype=np.float64)


def dollar_action_memory_frame(dates, actions, transactions, end, length, ntx):
    """save_action_memory() of the two envs (:399-409, :453-459): ``{date, actions, transactions}``,
    one array per day in both list columns.  ``actions``: [>= length, N] as the env's ``actions_memory``
    holds them (the raw rows; ``stoploss_actions_memory`` for the stop-loss env); ``transactions``:
    [>= ntx, N].  The lists have the reference's lengths: an episode that ended on a cash shortage holds
    one transaction row fewer (``ntx == length - 1``, :341-344 returns before the append), and pandas
    raises its ValueError here as it does in the reference's call.  None for an empty record."""
    import pandas as pd
    n = int(length)
    if n == 0:
        return None
    return pd.DataFrame({"date": _own_dates(dates, end, n),
                         "actions": list(np.asarray(actions)[:n]),
                         "transactions": list(np.asarray(transactions, dtype=np.float64)[:int(ntx)])})


# ---------------------------------------------------------------------- the device side
class _Record:
    """A device-resident episode record: what ``EpisodeHistory``, ``PortfolioEpisodeHistory``,
    ``CryptoEpisodeHistory``, ``StockNpEpisodeHistory`` and ``TwoWaveEpisodeHistory`` are made of.  A
    subclass declares its data:
      ``_ptrs_cls``    the ctypes struct of finenv_<kind>_set_history (one pointer per tensor, capacity)
      ``_series``      ((name, dtype), ...): the time-major tensors [capacity, E]; those named in the
                       constructor's ``without`` are not recorded (None)
      ``_per_ticker``  (name, dtype, rows short of capacity): the optional tensor [capacity - short, E, N],
                       or a tuple of such triples (the constructor's ``per_ticker`` is then one switch
                       for all of them or a tuple of switches)
      ``_env_last``    those tensors are [capacity - short, N, E] instead (the env is the fastest index)
      ``_per_env``     ((name, dtype), ...): the tensors [E] beside ``length`` and ``flags``
      ``_attr``        {struct field: attribute} where the tensor's attribute has another name
      ``_assets``      the env attribute that holds N
      ``_min_capacity`` 2 where arming writes entry 0, 1 where an armed record is empty
      ``metric_keys``  the columns of ``metrics()``
    """

    _env_last, _per_env, _assets, _min_capacity = False, (), "stock_dim", 2
    _attr = {"len": "length"}

    @classmethod
    def _tickers(cls):
        """``_per_ticker`` as a tuple of (name, dtype, short) triples."""
        pt = cls._per_ticker
        return (pt,) if isinstance(pt[0], str) else tuple(pt)

    def __init__(self, env, capacity, per_ticker=True, without=()):
        torch = _torch()
        E, N, dev = env.num_envs, getattr(env, self._assets), env.device
        capacity = int(capacity)
        if capacity < self._min_capacity:
            raise ValueError(f"history capacity must be >= {self._min_capacity}")
        self.env, self.capacity = env, capacity
        for name, dtype in self._series:
            setattr(self, name, None if name in without else
                    torch.zeros(capacity, E, dtype=getattr(torch, dtype), device=dev))
        specs = self._tickers()
        wanted = per_ticker if isinstance(per_ticker, tuple) else (per_ticker,) * len(specs)
        for (name, dtype, short), on in zip(specs, wanted):
            shape = (capacity - short, N, E) if self._env_last else (capacity - short, E, N)
            setattr(self, name, torch.zeros(*shape, dtype=getattr(torch, dtype), device=dev)
                    if on else None)
        for name, dtype in self._per_env:
            setattr(self, name, torch.zeros(E, dtype=getattr(torch, dtype), device=dev))
        self.length = torch.zeros(E, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(E, dtype=torch.int32, device=dev)
        self._metrics = None
        self._ptrs = self._ptrs_cls(*(None if t is None else t.data_ptr() for t in self._tensors()),
                                    capacity)
        env._call("set_history", C.byref(self._ptrs))
        self.arm()

    def _tensors(self):
        """The tensors in the pointer struct's field order (None: a per-ticker one, disabled)."""
        return [getattr(self, self._attr.get(f, f)) for f, _ in self._ptrs_cls._fields_[:-1]]

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._tensors() if t is not None)

    @property
    def complete(self):
        """bool [E]: the recorded episode has reported done; the record is final."""
        return (self.flags & nat.HIST_COMPLETE) != 0

    @property
    def overflow(self):
        """bool [E]: the episode outran ``capacity``; the entries below it are right, later days are
        missing."""
        return (self.flags & nat.HIST_OVERFLOW) != 0

    def arm(self, mask=None):
        """Start a new record for every env, or those with mask[e] != 0, from its CURRENT state: one
        entry (the class docstring says what it holds), flags cleared (finenv_<kind>_history_arm).  No
        host synchronisation."""
        mptr = None
        if mask is not None:
            torch = _torch()
            if not torch.is_tensor(mask):
                mask = torch.from_numpy(np.asarray(mask).astype(np.uint8))
            mask = mask.to(device=self.env.device, dtype=torch.uint8).contiguous()
            mptr = C.c_void_p(mask.data_ptr())
        self.env._call("history_arm", mptr, self.env._stream())

    def metrics(self, annualization=252 ** 0.5):
        """Backtest figures of the recorded series -> f64 [E, 6] device tensor, columns ``metric_keys``
        (n_returns, cumulative_return, mean, std, sharpe, max_drawdown); finenv_<kind>_history_metrics.
        ``252 ** 0.5`` gives the env's terminal printout (env_stocktrading.py:243-251,
        env_portfolio.py:145-152), ``4 ** 0.5`` get_validation_sharpe's figure.  The stock env's returns
        are ``asset.pct_change()``, so ``n_returns`` is ``length - 1``; the portfolio env's are the
        recorded ones with their leading 0, so it is ``length``.  Sharpe is NaN with fewer than two
        returns or zero std; rows of unarmed envs are NaN.  The tensor is reused by the next call."""
        if self._metrics is None:
            self._metrics = _torch().zeros(self.env.num_envs, len(self.metric_keys),
                                           dtype=_torch().float64, device=self.env.device)
        self.env._call("history_metrics", float(annualization), C.c_void_p(self._metrics.data_ptr()),
                       self.env._stream())
        return self._metrics

    def metrics_dict(self, annualization=252 ** 0.5):
        """``metrics()`` as ``{name: f64 [E] device tensor}``."""
        m = self.metrics(annualization)
        return {k: m[:, j] for j, k in enumerate(self.metric_keys)}

    # ------------------------------------------------------------------ frames
    def _host(self, envs, names):
        """Host copies of the selected envs' columns, ``{"length": ..., name: ...}``: one device-to-host
        copy per tensor.  Time-major with the env second ([entries, n] and [entries, n, N]), whatever
        the device layout is; the per-env tensors are [n]."""
        torch = _torch()
        idx = torch.as_tensor(envs, dtype=torch.int64, device=self.env.device)
        out = {"length": self.length.index_select(0, idx).cpu().numpy()}
        per_env = [name for name, _ in self._per_env]
        switch = {a: f for f, a in self._attr.items()}
        for k in names:
            t = getattr(self, k)
            if t is None:
                raise nat.FinenvError(f"this history was enabled with {switch.get(k, k)}=False")
            if k in per_env:
                out[k] = t.index_select(0, idx).cpu().numpy()
            elif self._env_last and k in [name for name, _, _ in self._tickers()]:
                out[k] = t.index_select(2, idx).cpu().numpy().transpose(0, 2, 1)
            else:
                out[k] = t.index_select(1, idx).cpu().numpy()
        return out

    def _frames(self, e, build, *names, tickers=False, dates=True):
        """``e`` -> host columns -> frame(s): ``build([dates, [tickers,]] *columns, length)`` for one env
        index (a frame) or a sequence of them (a list of frames)."""
        one = isinstance(e, (int, np.integer))
        envs = [int(e)] if one else [int(x) for x in e]
        h = self._host(envs, names)
        head = ()
        if dates:
            panel = self.env.panel
            head = (panel.dates, panel.tickers) if tickers else (panel.dates,)
        per_env = [name for name, _ in self._per_env]
        out = [build(*head, *(h[k][j] if k in per_env else h[k][:, j] for k in names), h["length"][j])
               for j in range(len(envs))]
        return out[0] if one else out


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
    reports ``done`` (``complete``).  Its first entry is asset_memory[0] at the start of an episode,
    else the current total asset, and the current date.  An auto-reset inside ``step`` does not arm: the
    finished episode stays readable until the next host reset or ``arm``.  The pointers are launch
    arguments, so a captured graph records only if the history was enabled before the capture.
    """

    _ptrs_cls, metric_keys = nat.StockHistoryPtrs, METRIC_KEYS
    _series, _per_ticker = (("asset", "float64"), ("row", "int32")), ("actions", "int32", 1)

    def __init__(self, env, capacity, actions=True):
        super().__init__(env, capacity, actions)
        if actions:
            env.enable_realised()

    def validation_sharpe(self):
        """get_validation_sharpe (models.py:214-230) of every env's record -> host f64 [E]: ``inf`` /
        ``0.0`` when the variance of the daily returns is 0 (``models.py:220-224``)."""
        m = self.metrics(4 ** 0.5).cpu().numpy()
        return validation_sharpe_from(m[:, METRIC_KEYS.index("mean")], m[:, METRIC_KEYS.index("std")])

    def save_asset_memory(self, e):
        """The reference's save_asset_memory() frame of env ``e`` (a list of frames for a list of
        envs)."""
        return self._frames(e, asset_memory_frame, "asset", "row")

    def save_action_memory(self, e):
        """The reference's save_action_memory() frame of env ``e`` (a list for a list of envs)."""
        return self._frames(e, action_memory_frame, "actions", "row", tickers=True)

    def account_value_frame(self, e):
        """The frame behind account_value_*.csv of env ``e`` (a list for a list of envs)."""
        return self._frames(e, account_value_frame, "asset", "row")


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
    resets and by ``arm(mask)``; final on the step that reports ``done``.  The first entry is the current
    portfolio value, return 0, the current date and weights 1/N.  An auto-reset inside ``step`` does not
    arm.  The pointers are launch arguments: enable the history before capturing a graph.
    """

    _ptrs_cls, metric_keys = nat.PortfolioHistoryPtrs, PORTFOLIO_METRIC_KEYS
    _series = (("value", "float64"), ("ret", "float64"), ("row", "int32"))
    _per_ticker = ("weights", "float32", 0)

    def __init__(self, env, capacity, weights=True):
        super().__init__(env, capacity, weights)

    def save_asset_memory(self, e):
        """The reference's save_asset_memory() frame ``{date, daily_return}`` of env ``e`` (a list of
        frames for a list of envs)."""
        return self._frames(e, portfolio_asset_memory_frame, "ret", "row")

    def save_action_memory(self, e):
        """The reference's save_action_memory() frame of env ``e`` (a list for a list of envs)."""
        return self._frames(e, portfolio_action_memory_frame, "weights", "row", tickers=True)


class CryptoEpisodeHistory(_Record):
    """Device-resident episode record of a ``VecCryptoEnv`` (``env.enable_history()``): the account value
    of every env's episode, one entry per step, written by the step kernel itself
    (finenv_crypto_set_history, include/finenv.h) -- what DRLAgent.DRL_prediction_load_from_file
    (agents/stablebaselines3/models.py:144-162) returns for the one env it runs.

    Tensors (time-major; entries at or past ``length[e]`` are unspecified):
      ``asset``     f64 [capacity, E]     total_asset after the step (env_multiple_crypto.py:82-84)
      ``holdings``  f64 [capacity, E]     np.sum(stocks * price_array[time]) of that step (:82)
      ``stocks``    f32 [capacity, N, E]  holdings after the step (the state's [N, E] layout), or None
      ``start``     i32 [E]               panel row of entry 0; entry k is panel row ``start + k``
      ``length``    i32 [E]               entries recorded; 0 = not armed
      ``flags``     i32 [E]               bit 0 complete, bit 1 overflow (``complete`` / ``overflow``)

    Armed by the constructor (from the env's current state), by ``env.reset(mask)`` for the envs it
    resets and by ``arm(mask)``; entry 0 is the current total asset, the value of the current holdings
    (``initial_cash`` and 0.0 at the start of an episode) and the current holdings.  The terminal step is
    recorded -- this env trades on it -- and makes the record final.  An auto-reset inside ``step`` does
    not arm: the finished episode stays readable until the next host reset or ``arm``.  The pointers are
    launch arguments: enable the history before capturing a graph.
    """

    _ptrs_cls, metric_keys = nat.CryptoHistoryPtrs, CRYPTO_METRIC_KEYS
    _series = (("asset", "float64"), ("holdings", "float64"))
    _per_ticker, _env_last = ("stocks", "float32", 0), True
    _per_env, _assets = (("start", "int32"),), "crypto_num"

    def __init__(self, env, capacity, stocks=True):
        super().__init__(env, capacity, stocks)

    def account_values(self, e):
        """The true account value of env ``e``'s recorded episode, ``asset[:length]`` -> f64 array (a list
        of arrays for a sequence of envs)."""
        return self._frames(e, crypto_account_values, "asset", dates=False)

    def episode_total_assets(self, e, initial_total_asset=None):
        """The list DRL_prediction_load_from_file returns for env ``e`` (a list of lists for a sequence of
        envs), as Python floats: ``[initial_total_asset] + [initial_total_asset + holdings[k]]``.  The
        reference adds the holdings' value to ``initial_total_asset`` where the cash belongs
        (models.py:152-155); this reproduces its list, ``account_values`` gives the true curve.
        ``initial_total_asset`` defaults to the env's ``initial_cash``."""
        init = self.env.initial_cash if initial_total_asset is None else initial_total_asset
        return self._frames(e, lambda holdings, n: crypto_episode_total_assets(holdings, n, init),
                            "holdings", dates=False)

    def positions(self, e):
        """The holdings after every recorded entry of env ``e`` -> f32 [length, N] (a list for a sequence
        of envs); needs ``stocks=True``."""
        return self._frames(e, crypto_positions, "stocks", dates=False)

    def rows(self, e):
        """The panel rows of env ``e``'s entries, ``start + arange(length)`` (a list for a sequence of
        envs): index your own timestamps with them."""
        return self._frames(e, crypto_rows, "start", dates=False)


class StockNpEpisodeHistory(_Record):
    """Device-resident episode record of a ``VecStockTradingEnvNP`` (``env.enable_history()``): the
    account curve of every env's episode, one entry per step, written by the step kernel itself
    (finenv_stocknp_set_history, include/finenv.h) -- what DRLAgent.DRL_prediction
    (agents/elegantrl/models.py:105-131) returns for the one env it runs.

    Tensors (time-major; entries at or past ``length[e]`` are unspecified):
      ``asset``   f64 [capacity, E]     total_asset after the step (env_stocktrading_np.py:137)
      ``tag``     u8  [capacity, E]     its NumPy-2 scalar type (0 float, 1 float32, 2 float64), or None
      ``stocks``  f32 [capacity, N, E]  holdings after the step (the state's [N, E] layout), or None
      ``start``   i32 [E]               panel row of entry 0; entry k is panel row ``start + k``
      ``length``  i32 [E]               entries recorded; 0 = not armed
      ``flags``   i32 [E]               bit 0 complete, bit 1 overflow (``complete`` / ``overflow``)

    Armed by the constructor (from the env's current state), by ``env.reset(mask)`` for the envs it
    resets and by ``arm(mask)``; entry 0 is the current total asset (``initial_total_asset`` at the start
    of an episode), its tag and the current holdings.  The terminal step is recorded -- this env trades
    on it -- from the values before an auto-reset replaces them, and makes the record final.  An
    auto-reset inside ``step`` does not arm: the finished episode stays readable until the next host
    reset or ``arm``.  The pointers are launch arguments: enable the history before capturing a graph.
    """

    _ptrs_cls, metric_keys = nat.StockNpHistoryPtrs, STOCKNP_METRIC_KEYS
    _series = (("asset", "float64"), ("tag", "uint8"))
    _per_ticker, _env_last = ("stocks", "float32", 0), True
    _per_env, _assets = (("start", "int32"),), "action_dim"

    def __init__(self, env, capacity, stocks=True, tags=True):
        super().__init__(env, capacity, stocks, without=() if tags else ("tag",))

    def _typed(self, e, build):
        """``build(asset, tag, length)`` per env, with ``tag`` None where it is not recorded."""
        if self.tag is None:
            return self._frames(e, lambda asset, n: build(asset, None, n), "asset", dates=False)
        return self._frames(e, build, "asset", "tag", dates=False)

    def account_values(self, e):
        """The account curve of env ``e``'s recorded episode, ``asset[:length]`` -> f64 array (a list of
        arrays for a sequence of envs)."""
        return self._frames(e, stocknp_account_values, "asset", dates=False)

    def episode_total_assets(self, e):
        """The list DRL_prediction returns for env ``e`` (a list of lists for a sequence of envs); with
        ``tags`` recorded every element is the scalar type the reference's list holds (``float`` /
        ``np.float32`` / ``np.float64``), else a Python float."""
        return self._typed(e, stocknp_episode_total_assets)

    def episode_returns(self, e):
        """``total_asset / initial_total_asset`` after every step of env ``e``'s record (models.py:124),
        in the dtype NumPy promotes to; the reference's ``episode_returns`` when the record was armed at
        the episode's start (a list of lists for a sequence of envs)."""
        return self._typed(e, stocknp_episode_returns)

    def positions(self, e):
        """The holdings after every recorded entry of env ``e`` -> f32 [length, N] (a list for a sequence
        of envs); needs ``stocks=True``."""
        return self._frames(e, crypto_positions, "stocks", dates=False)

    def rows(self, e):
        """The panel rows of env ``e``'s entries, ``start + arange(length)`` (a list for a sequence of
        envs): index your own dates with them."""
        return self._frames(e, crypto_rows, "start", dates=False)


class TwoWaveEpisodeHistory(_Record):
    """Device-resident episode record of a ``VecCashPenaltyEnv`` / ``VecStopLossEnv``
    (``env.enable_history()``): the reference's ``account_information``, ``actions_memory`` and
    ``transaction_memory`` (env_stocktrading_cashpenalty.py:308-355, env_stocktrading_stoploss.py:315-385)
    of every env's current episode -- the audit row of every step, copied by one small kernel behind the
    step kernel (finenv_<kind>_set_history, include/finenv.h), with no host work per step.

    Tensors (time-major; entries at or past ``length[e]`` are unspecified):
      ``cash``         f64 [capacity, E]     begin cash of the step (:312)
      ``asset_value``  f64 [capacity, E]     asset value (:310); total assets are ``cash + asset_value``
      ``reward``       f64 [capacity, E]     the f64 reward (:317)
      ``reason``       i32 [capacity, E]     the step's reason flags (``nat.AUDIT_F_*``)
      ``tx``           f64 [capacity, E, N]  transaction_memory, or None (``transactions=False``)
      ``actions``      f32 [capacity, E, N]  the raw action rows ``step`` was given, or None
      ``start``        i32 [E]               panel row of entry 0; entry k is panel row ``start + k``
      ``end``          i32 [E]               end of the window the record was armed on
      ``ntx``          i32 [E]               rows of transaction_memory: ``length``, or one fewer when the
                                             episode ended on a cash shortage
      ``length``       i32 [E]               entries recorded (0: armed and empty, or not armed)
      ``flags``        i32 [E]               bit 2 armed, bit 0 complete, bit 1 overflow

    Armed by the constructor (at the env's current date), by ``env.reset(mask)`` for the envs it resets
    and by ``arm(mask)``; an armed record is EMPTY, as the reference's lists are after ``reset()``.  The
    step that ends at the last date appends nothing (:299-301); either ending makes the record final.
    An auto-reset inside ``step`` does not arm: the finished episode stays readable until the next host
    reset or ``arm``.  The pointers are launch arguments: enable the history before capturing a graph.
    """

    _ptrs_cls, metric_keys = nat.TwoWaveHistoryPtrs, TWOWAVE_METRIC_KEYS
    _series = (("cash", "float64"), ("asset_value", "float64"), ("reward", "float64"), ("reason", "int32"))
    _per_ticker = (("tx", "float64", 0), ("actions", "float32", 0))
    _per_env = (("start", "int32"), ("end", "int32"), ("ntx", "int32"))
    _attr = {"len": "length", "transactions": "tx"}
    _assets, _min_capacity = "action_dim", 1

    def __init__(self, env, capacity, transactions=True, actions=True):
        super().__init__(env, capacity, (transactions, actions))

    @property
    def armed(self):
        """bool [E]: the env has a record (possibly empty)."""
        return (self.flags & nat.HIST_ARMED) != 0

    def _actions_memory(self, raw, start, n):
        """The env's ``actions_memory`` rows from the raw ones: themselves (:264), or for the stop-loss
        env ``(actions * hmax) * closings`` with the panel's close rows of the entries."""
        if self.env._kind != "stoploss":
            return raw
        lo = int(start)
        return stoploss_actions_memory(raw[:int(n)], float(self.env._cfg.hmax),
                                       self.env.panel.close[lo:lo + int(n)])

    def save_asset_memory(self, e):
        """The reference's save_asset_memory() frame of env ``e`` -- ``cash, asset_value, total_assets,
        reward, date`` -- or None for an empty record (a list for a sequence of envs)."""
        return self._frames(e, dollar_asset_memory_frame, "cash", "asset_value", "reward", "end")

    def save_action_memory(self, e):
        """The reference's save_action_memory() frame ``{date, actions, transactions}`` of env ``e``, or
        None for an empty record (a list for a sequence of envs); needs both optional tensors.  For an
        episode that ended on a cash shortage it raises the ValueError the reference's call raises."""
        return self._frames(
            e, lambda dates, actions, tx, start, end, ntx, n: dollar_action_memory_frame(
                dates, self._actions_memory(actions, start, n), tx, end, n, ntx),
            "actions", "tx", "start", "end", "ntx")

    def account_values(self, e):
        """Total assets ``cash + asset_value`` of env ``e``'s entries -> f64 [length] (a list for a
        sequence of envs)."""
        return self._frames(e, lambda cash, av, n: np.asarray(cash[:int(n)] + av[:int(n)], np.float64),
                            "cash", "asset_value", dates=False)

    def transactions(self, e):
        """transaction_memory of env ``e`` -> f64 [ntx, N]; needs ``transactions=True``."""
        return self._frames(e, lambda tx, ntx, n: np.array(tx[:int(ntx)]), "tx", "ntx", dates=False)

    def raw_actions(self, e):
        """The action rows ``step`` was given on env ``e``'s entries -> f32 [length, N]; needs
        ``actions=True``."""
        return self._frames(e, lambda a, n: np.array(a[:int(n)]), "actions", dates=False)

    def reasons(self, e):
        """The reason flag words (``nat.AUDIT_F_*``) of env ``e``'s entries -> i32 [length]."""
        return self._frames(e, lambda r, n: np.array(r[:int(n)]), "reason", dates=False)

    def rows(self, e):
        """The panel rows of env ``e``'s entries, ``start + arange(length)``: the dates the steps were
        taken on (the frames' ``date`` column is the reference's, see ``dollar_asset_memory_frame``)."""
        return self._frames(e, crypto_rows, "start", dates=False)
