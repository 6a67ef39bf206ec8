"""The data formats on either side of the env path: the DataFrame index
contract the DataFrame-backed envs rely on and the array layout the array-state env consumes.
Vectorised restatements -- same results as the reference helpers, no network, no stockstats.

  data_split   <- finrl/meta/preprocessor/preprocessors.py:24-33
  df_to_array  <- finrl/meta/data_processors/processor_yahoofinance.py:293-318 plus the
                  NaN / inf -> 0 clean-up of finrl/meta/data_processor.py:74-84
  clean_data   <- finrl/meta/preprocessor/preprocessors.py:107-131 (FeatureEngineer.clean_data:
                  keep only tickers with a close on every date -- what makes the panel complete
                  before add_turbulence / the envs see it)
"""
from __future__ import annotations

import numpy as np


def data_split(df, start, end, target_date_col="date"):
    """Rows with start <= date < end, sorted by (date, tic), index = day ordinal."""
    data = df[(df[target_date_col] >= start) & (df[target_date_col] < end)]
    data = data.sort_values([target_date_col, "tic"], ignore_index=True)
    data.index = data[target_date_col].factorize()[0]
    return data


def clean_data(data):
    """Rows sorted by (date, tic), index = day ordinal, tickers with a missing close on any
    date dropped (delisted / not yet listed)."""
    df = data.copy()
    df = df.sort_values(["date", "tic"], ignore_index=True)
    df.index = df.date.factorize()[0]
    closes = df.pivot_table(index="date", columns="tic", values="close")
    keep = closes.columns[closes.notna().all(axis=0)]
    return df[df.tic.isin(keep)]


def df_to_array(df, tech_indicator_list, if_vix, price_col="adjcp"):
    """-> price_array [T, N], tech_array [T, N*K] (ticker-major: all indicators of ticker 0,
    then ticker 1, ...), turbulence_array [T] -- the config of env_stocktrading_np.

    The reference hstacks one ticker at a time in `df.tic.unique()` order, each ticker's rows
    in frame order; this does the same with one stable sort."""
    tics = df["tic"].to_numpy()
    uniq, first = np.unique(tics, return_index=True)
    uniq = uniq[np.argsort(first)]                      # order of first appearance
    code = {t: i for i, t in enumerate(uniq)}
    tic_code = np.fromiter((code[t] for t in tics), dtype=np.int64, count=len(tics))
    order = np.argsort(tic_code, kind="stable")         # ticker-major, frame order within
    N = len(uniq)
    if len(df) % N:
        raise ValueError("every ticker must have the same number of rows")
    T = len(df) // N
    price = df[price_col].to_numpy(dtype=np.float64)[order].reshape(N, T).T
    tech = df[list(tech_indicator_list)].to_numpy(dtype=np.float64)[order]
    K = len(tech_indicator_list)
    tech = tech.reshape(N, T, K).transpose(1, 0, 2).reshape(T, N * K)
    risk_col = "vix" if if_vix else "turbulence"
    turb = df[risk_col].to_numpy()[order][:T]           # the reference takes the FIRST ticker's
    tech = np.array(tech)                               # rows (:304-307)
    tech[np.isnan(tech)] = 0
    tech[np.isinf(tech)] = 0
    return np.ascontiguousarray(price), tech, np.array(turb)


def windows_from_dates(dates, starts, ends):
    """Panel rows of ``data_split(df, start, end)`` for each (start, end) date pair -> (start, end)
    int64 arrays, end exclusive: the rows whose date satisfies ``start <= date < end`` (the
    ``windows=`` / ``set_windows`` argument of VecStockTradingEnv).  ``dates``: the panel's dates
    (e.g. ``df.date``; sorted and deduplicated here, i.e. the factorize order of ``data_split``
    over the full frame).  Dates compare as they do in the frame: strings lexically, numbers
    numerically.  Raises ValueError on a pair that selects no row."""
    days = np.unique(np.asarray(dates))
    lo = np.searchsorted(days, np.asarray(starts), side="left")
    hi = np.searchsorted(days, np.asarray(ends), side="left")
    lo, hi = np.broadcast_arrays(np.atleast_1d(lo), np.atleast_1d(hi))
    empty = hi <= lo
    if empty.any():
        k = int(np.argmax(empty))
        raise ValueError(f"window {k} selects no panel day (start={np.ravel(starts)[k % np.size(starts)]!r}, "
                         f"end={np.ravel(ends)[k % np.size(ends)]!r})")
    return lo.astype(np.int64), hi.astype(np.int64)


def random_windows(T, E, length, generator=None, device="cuda"):
    """E random windows of ``length`` panel days (an int, or [E] lengths) in a panel of T days ->
    (start, end) int32 [E] tensors on ``device``, start uniform over the positions the window fits
    in (the cash-penalty env's random start, env_stocktrading_cashpenalty.py:135).  Only torch ops:
    usable inside a captured graph, e.g. ``env.set_windows(*random_windows(...), mask=done)``.
    ``generator``: a torch.Generator on ``device``."""
    import torch
    dev, E, T = torch.device(device), int(E), int(T)
    if torch.is_tensor(length):
        length = length.to(device=dev, dtype=torch.int64).expand(E)
    else:
        n = np.asarray(length, dtype=np.int64)
        if ((n < 1) | (n > T)).any():
            raise ValueError(f"window length must be in [1, {T}]")
        length = torch.full((E,), int(n), dtype=torch.int64, device=dev) if n.ndim == 0 else \
            torch.from_numpy(np.broadcast_to(n, (E,)).copy()).to(dev)
    span = T - length + 1                              # start positions the window fits in
    u = torch.rand(E, generator=generator, device=dev, dtype=torch.float64)
    start = torch.minimum((u * span).to(torch.int64), span - 1)
    return start.to(torch.int32), (start + length).to(torch.int32)
