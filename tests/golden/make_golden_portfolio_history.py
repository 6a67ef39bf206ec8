#!/usr/bin/env python3
"""Golden-vector generator for the portfolio env's episode history (run ONLY in the build container,
where the reference tree exists).

    python tests/golden/make_golden_portfolio_history.py [name ...]

Runs the *unmodified* reference StockPortfolioEnv (imported through oracle/ref_harness.py) through the
restated DRL_prediction loop of tests/harness_loops.py on small seeded synthetic frames and stores, as
harness_portfolio_<name>.npz next to this file: the panel, the float32 actions fed, the env's four
memories as they stand on the second-to-last day (where DRL_prediction pulls its frames; all T entries
are there), the two frames DRL_prediction returned and the terminal branch's printout.  Data only: no
reference source is stored."""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import harness_loops as hl  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402


class TableModel:
    """Stands in for a trained SB3 model: ``predict`` returns row ``step`` of a float32 table.  Right
    before the terminal step (after DRL_prediction has pulled its frames, before the VecEnv's reset wipes
    them) it copies the env's four memories."""

    def __init__(self, actions, env, n_days):
        self.actions, self.env, self.n_days = np.asarray(actions, np.float32), env, n_days
        self.step, self.memories = 0, None

    def predict(self, obs, deterministic=True):
        o = np.asarray(obs)
        assert o.ndim == 3 and o.shape[0] == 1 and o.dtype == np.float32, (o.shape, o.dtype)
        if self.step == self.n_days - 1:
            e = self.env
            self.memories = (list(e.asset_memory), list(e.portfolio_return_memory),
                             [np.asarray(w) for w in e.actions_memory], list(e.date_memory))
        a = self.actions[self.step % len(self.actions)]
        self.step += 1
        return a[None].copy(), None


def panel(seed, T, N, K, lookback=8, constant=False):
    """close [T,N], cov [T,N,N], tech [T,K,N]: the construction of make_golden.py's portfolio frames;
    `constant`: every close of the episode equals day 0's (every return is exactly 0)."""
    rng = np.random.default_rng(seed)
    close = 100.0 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    tech = rng.normal(0, 1, (T, K, N))
    rets = np.diff(np.log(close), axis=0, prepend=np.log(close[:1]))
    cov = np.empty((T, N, N))
    for t in range(T):
        w = rets[max(0, t - lookback):t + 1]
        cov[t] = np.atleast_2d(np.cov(w.T)) if len(w) > 1 else np.eye(N) * 1e-4
    if constant:
        close = np.broadcast_to(close[0], (T, N)).copy()
    return close, cov, tech


def run(name, *, seed, T, N, K, initial_amount=1_000_000, act_scale=1.0, constant=False):
    import pandas as pd
    mod = rh.load_portfolio()
    close, cov, tech = panel(seed, T, N, K, constant=constant)
    rng = np.random.default_rng(seed + 2000)
    dates = [f"d{t:04d}" for t in range(T)]
    tickers = [f"TIC{i:03d}" for i in range(N)]
    names = [f"ind{k}" for k in range(K)]
    cols = {"date": np.repeat(dates, N), "tic": np.tile(tickers, T), "close": close.reshape(-1)}
    for k, nme in enumerate(names):
        cols[nme] = tech[:, k, :].reshape(-1)
    df = pd.DataFrame(cols)
    df["cov_list"] = [cov[t] for t in range(T) for _ in range(N)]
    df.index = np.repeat(np.arange(T), N)
    act = (rng.uniform(0, 1, (T, N)) * act_scale).astype(np.float32)
    printed = io.StringIO()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as work:
        os.makedirs(os.path.join(work, "results"))
        os.chdir(work)
        try:
            with contextlib.redirect_stdout(printed):
                env = mod.StockPortfolioEnv(df=df, stock_dim=N, hmax=100, initial_amount=initial_amount,
                                            transaction_cost_pct=0.001, reward_scaling=1e-4,
                                            state_space=N, action_space=N, tech_indicator_list=names)
                model = TableModel(act, env, T)
                acct, acts = hl.drl_prediction(model, env)
        finally:
            os.chdir(cwd)
    asset, ret, amem, dmem = model.memories
    assert len(asset) == len(ret) == len(amem) == len(dmem) == T and model.step == T
    a64, r64 = np.asarray(asset, np.float64), np.asarray(ret, np.float64)
    assert (a64[1:] == a64[:-1] * (1 + r64[1:])).all()
    assert isinstance(ret[0], int) and all(w.dtype == np.float32 for w in amem[1:])
    text = [ln for ln in printed.getvalue().splitlines() if ln.strip()]
    out = dict(
        close=close, cov=cov, tech=tech, actions=act, dates=np.asarray(dates), tickers=np.asarray(tickers),
        cfg_int=np.array([T, N, K], np.int64), cfg_float=np.array([initial_amount], np.float64),
        asset_memory=a64, portfolio_return_memory=r64,
        actions_memory=np.stack([np.asarray(w, np.float64) for w in amem]),
        date_memory=np.asarray([str(d) for d in dmem]),
        account_columns=np.asarray(acct.columns.tolist()), account_date=np.asarray(acct["date"].tolist()),
        account_daily_return=acct["daily_return"].to_numpy(np.float64),
        account_dtypes=np.asarray([str(t) for t in acct.dtypes]),
        action_values=acts.to_numpy(np.float64), action_columns=np.asarray(acts.columns.tolist()),
        action_index=np.asarray(acts.index.tolist()), action_index_name=np.array(str(acts.index.name)),
        action_dtypes=np.asarray([str(t) for t in acts.dtypes]),
        printout=np.asarray(text),
        meta=np.array([f"seed={seed}", f"numpy={np.__version__}", f"pandas={pd.__version__}",
                       "source=finrl/meta/env_portfolio_allocation/env_portfolio.py (unmodified) through "
                       "tests/harness_loops.py::drl_prediction"]))
    path = os.path.join(HERE, f"harness_portfolio_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB) T={T} N={N} end={a64[-1]:.2f} "
          f"printout={text}")


SCENARIOS = {
    "dow30": dict(seed=41, T=20, N=30, K=8),
    "n5": dict(seed=42, T=16, N=5, K=2, initial_amount=50_000, act_scale=3.0),
    "n2k1": dict(seed=43, T=12, N=2, K=1, initial_amount=1_000),
    "const": dict(seed=44, T=10, N=5, K=2, initial_amount=200_000, constant=True),
}


if __name__ == "__main__":
    for n in sys.argv[1:] or list(SCENARIOS):
        run(n, **SCENARIOS[n])
