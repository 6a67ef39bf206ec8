#!/usr/bin/env python3
"""Cost of the portfolio env's episode history (VecStockPortfolioEnv.enable_history) on
bench.py --env portfolio's workload: 65,536 envs x DOW30 x 8 indicators, 63-day episode windows.  ONE
process, ONE env; the variants alternate inside every round, each timed with HIP events over steps that
all record:
  a  history detached (the step kernel of a build without the feature)
  b  history attached, weights=False        (+20 B written, 8 B read per env and step)
  c  history attached, weights=True         (+20 + 4N B written)
  d  history detached, one state_numpy() and one weights.cpu() after every step: the host loop the
     history replaces
usage: python3 tools/bench_portfolio_history.py <lockstep|desync> [--variants a,b,c,d] [--rounds R]
                                                [--envs E] [--json PATH]
  lockstep  every env on the window [0, 63): one record row per step, written contiguously
  desync    random 63-day windows and a random half of the envs restarted 31 steps after the others:
            neighbouring envs sit on different panel rows AND on different record rows
A round of a variant is: reset (arms every record), [desync: 31 steps, reset of a random half], then the
timed steps -- 62 (lockstep) or 31 (desync), none of them terminal, so every env records on every timed
step (asserted).  FINENV_LIB=<libfinenv.so of another build> times that build; one without the history
entry points can run variant a only (that is how the parent commit is measured with this same script).
Under `rocprofv3 --kernel-trace --stats -- python3 tools/bench_portfolio_history.py lockstep --variants c`
the kernel stats give the recording instantiation's own time."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 63


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=("lockstep", "desync"))
    ap.add_argument("--variants", default="a,b,c,d")
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--json", default=None)
    o = ap.parse_args()
    variants = o.variants.split(",")
    import torch
    import bench
    from finrl_amd import _native as nat
    from finrl_amd.data import random_windows
    if not torch.cuda.is_available():
        sys.exit("bench_portfolio_history: no HIP device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    E = o.envs
    args = type("A", (), dict(envs_per_gpu=E, action_pool=8, rollout=0, desync=False, no_stats=False,
                              env="portfolio", tickers=30, turbulence_pct=None))()
    w = bench.build_workload(args, torch, dev, 0)
    env, N = w.env, w.env.stock_dim
    has_api = hasattr(nat.lib(), "finenv_portfolio_set_history")
    if not has_api and variants != ["a"]:
        sys.exit("bench_portfolio_history: this libfinenv.so has no portfolio history; --variants a only")
    desync = o.case == "desync"
    gen = torch.Generator(device=dev).manual_seed(7)
    if desync:
        env.set_windows(*random_windows(env.panel.T, E, WINDOW, generator=gen, device=dev))
    else:
        env.set_windows(0, WINDOW)
    timed = 31 if desync else WINDOW - 1
    rounds = o.rounds or -(-200 // timed)
    half = (torch.rand(E, generator=gen, device=dev) < 0.5).to(torch.uint8)

    hists = {}
    if has_api:
        from finrl_amd.history import PortfolioEpisodeHistory
        for v, wts in (("b", False), ("c", True)):
            if v in variants:
                hists[v] = PortfolioEpisodeHistory(env, WINDOW, weights=wts)
    if "d" in variants:
        env.enable_weights()
    weights_out = env.weights                    # passed to variant d's steps only

    def select(v):
        if has_api:
            env._call("set_history", C.byref(hists[v]._ptrs) if v in hists else None)
        env.weights = weights_out if v == "d" else None
        env._step_args = None                    # BatchedEnv.step caches the output pointers

    def one_round(v, record):
        select(v)
        env.reset()
        i = 0
        if desync:
            for i in range(31):
                env.step(w.pool[i % len(w.pool)])
            env.reset(half)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(timed):
            env.step(w.pool[(i + j) % len(w.pool)])
            if v == "d":
                env.state_numpy()
                env.weights.cpu()
        e1.record()
        torch.cuda.synchronize()
        if record:
            times[v].append(e0.elapsed_time(e1) * 1e3 / timed)
        if v in hists:                           # every env recorded on every timed step
            h = hists[v]
            assert int(h.length.min()) >= timed + 1 and not bool(h.complete.any()) \
                and not bool(h.overflow.any()), "a timed step did not record"

    times = {v: [] for v in variants}
    for v in variants:                           # warm-up: every variant's shapes, untimed
        one_round(v, False)
    for r in range(rounds):
        for v in variants:
            one_round(v, True)
    res = dict(case=o.case, envs=E, tickers=N, window=WINDOW, timed_steps_per_variant=timed * rounds,
               lib=os.path.abspath(nat.LIB_PATH), us_per_step={}, rounds_us={})
    for v in variants:
        t = sorted(times[v])
        res["us_per_step"][v] = round(t[len(t) // 2], 2)
        res["rounds_us"][v] = [round(x, 2) for x in times[v]]
    res["added_bytes_written_per_env_step"] = {"b": 20, "c": 20 + 4 * N}
    line = json.dumps(res)
    print(line, flush=True)
    if o.json:
        with open(o.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
