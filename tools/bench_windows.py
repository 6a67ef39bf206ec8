#!/usr/bin/env python3
"""Step time of the batched stock, portfolio, crypto, array-state stock, cash-penalty and stop-loss envs
with per-env episode windows (VecStockTradingEnv / VecStockPortfolioEnv / VecCryptoEnv /
VecStockTradingEnvNP / VecCashPenaltyEnv / VecStopLossEnv(windows=...)), on bench.py's workloads
(same synthetic panel, actions and env settings).
usage: python3 tools/bench_windows.py <case> [envs] [steps]
  case: full      -- every env on the whole panel [0, T) (lock-step days, the WIN instantiation)
        random63  -- random 63-day windows, hint_desynchronised(True)
        n100      -- the N = 100 shape (turbulence p90) with random 63-day windows
        none      -- no windows (bench.py's headline path), for reference
        desync    -- no windows, bench.py --desync's per-env start days
        pf-none, pf-full, pf-random63
                  -- the same on bench.py --env portfolio's workload (DOW30 x 8)
        pf-split  -- portfolio, envs alternating between a train window [0, 0.8 T) and a trade
                     window [0.8 T, T) (the portfolio tutorial's two data_split frames)
        cr-none, cr-full, cr-split
                  -- the same on bench.py --env crypto's workload (10 pairs, one-minute bars)
        cr-random<L>
                  -- crypto, random windows of L rows (e.g. cr-random1440: one day of minutes)
        np-none, np-full, np-split, np-random63
                  -- the same on bench.py --env stocknp's workload (array-state env, DOW30 x 8);
                     np-split: the train / test date ranges of finrl/train.py and finrl/test.py
        cp-none, cp-full, cp-split, cp-random63
                  -- the same on bench.py --env cashpenalty's workload (30 assets x 5 columns, random
                     starts: with windows each env draws inside its own window)
        sl-none, sl-full, sl-split, sl-random63
                  -- the same on bench.py --env stoploss's workload"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    case = sys.argv[1]
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    import torch
    import bench
    from finrl_amd.data import random_windows
    dev = torch.device("cuda", 0)
    n100 = case == "n100"
    pf, cr, npy = case.startswith("pf-"), case.startswith("cr-"), case.startswith("np-")
    cp, sl = case.startswith("cp-"), case.startswith("sl-")
    prefix = case[:3] if pf or cr or npy or cp or sl else ""
    case = case[len(prefix):]
    args = type("A", (), dict(envs_per_gpu=E, action_pool=8, rollout=0, desync=case == "desync",
                              no_stats=False, env="portfolio" if pf else "crypto" if cr else "stocknp" if npy else "cashpenalty" if cp else "stoploss" if sl else "stock", tickers=100 if n100 else 30,
                              turbulence_pct=90.0 if n100 else None))()
    w = bench.build_workload(args, torch, dev, 0)
    env = w.env
    T = env.price_array.shape[0] if cr else env.price_ary.shape[0] if npy else env.panel.T
    if cr and case.startswith("random"):
        g = torch.Generator(device=dev).manual_seed(7)
        env.set_windows(*random_windows(T, E, int(case[len("random"):]), generator=g, device=dev))
    elif case == "full":
        env.set_windows(0, T)
    elif case in ("random63", "n100"):
        g = torch.Generator(device=dev).manual_seed(7)
        env.set_windows(*random_windows(T, E, 63, generator=g, device=dev))
        if not prefix:
            env.hint_desynchronised(True)
    elif case == "split":
        cut = int(0.8 * T)
        train = torch.arange(E, device=dev) % 2 == 0
        env.set_windows(torch.where(train, 0, cut), torch.where(train, cut, T))
    env.reset()
    if getattr(w, "after_reset", None):
        w.after_reset()
    for i in range(300):
        env.step(w.pool[i % len(w.pool)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        env.step(w.pool[i % len(w.pool)])
    e1.record()
    torch.cuda.synchronize()
    name = prefix + case
    print(f"{name} E={E} N={env.action_dim} T={T}: {e0.elapsed_time(e1) * 1e3 / steps:.2f} us/step", flush=True)


if __name__ == "__main__":
    main()
