#!/usr/bin/env python3
"""A/B of two builds of libfinenv.so inside ONE process on ONE env: same handle, same device buffers
(so the same physical placement), only the library that launches the step kernel alternates.  The
handle is created by the base build, so both builds must share the layout of the finenv_<kind> handle
structs (variants of one source tree always do).
usage: python3 tools/exp_ab_inproc.py <variant .so> <n100|n30|n<tickers>|portfolio|portfolio-random63|stocknp> [rounds] [ascending]
  ascending: every action row sorted ascending in the ticker index, so the stock kernels' sort keys are in order
    as built (what the diagnostic switch FINENV_DIAG=4, "skip the sorting network", needs to leave results alone)
  portfolio-random63: the portfolio env with random 63-day episode windows (VecStockPortfolioEnv.set_windows)
  cashpenalty:c<C>:<disc|cont>, stoploss:c<C>:<disc|cont>: VecCashPenaltyEnv / VecStopLossEnv as bench.py builds
    them (65,536 envs, 30 assets, hmax=2_000, random starts) but with C columns per asset and the given
    discrete_actions setting -- C = 1: 61-column rows (one chunk), 5: 181 (the quad streamer; the bench.py
    line), 10: 331 (the one-wave step); a fourth field ":win63" attaches random 63-row windows (the WIN
    instantiations of the same kernels), drawn as for portfolio-random63"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("FINENV_OBS_PLACEMENT", "first")
sys.path.insert(0, ROOT)


def main():
    variants, kind = sys.argv[1].split(","), sys.argv[2]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ascending = "ascending" in sys.argv[4:]
    import torch
    import bench
    from finrl_amd import _native as nat
    base_path = nat.LIB_PATH
    libs = {}
    envs = {}
    for name, path in [("base", base_path)] + [(os.path.basename(v), v) for v in variants]:
        setting = None
        if "@" in path:                      # "<lib.so>@VAR=value": same library, an environment setting per run
            path, setting = path.split("@", 1)
        nat._lib, nat.LIB_PATH = None, os.path.abspath(path)
        key = name if name == "base" else name[10:].replace(".so", "")
        libs[key] = nat.lib()
        envs[key] = setting
    nat._lib, nat.LIB_PATH = libs["base"], base_path
    dev = torch.device("cuda", 0)
    E = 65536
    if kind.split(":")[0] in ("cashpenalty", "stoploss"):
        return two_wave_ab(libs, nat, torch, dev, E, kind, rounds)
    if ":" in kind:                        # "<kind>:<envs>", e.g. n30:262144
        kind, e_txt = kind.split(":")
        E = int(e_txt)
    if kind.startswith("crypto") and kind != "crypto":      # crypto32768 / crypto65536 / crypto131072 / crypto262144
        E = int(kind[6:])
    windows63 = kind == "portfolio-random63"
    if windows63:
        kind = "portfolio"
    a = dict(env="crypto", tickers=30, turbulence_pct=None) if kind.startswith("crypto") else \
        dict(env="portfolio", tickers=30, turbulence_pct=None) if kind == "portfolio" else \
        dict(env="stocknp", tickers=30, turbulence_pct=None) if kind == "stocknp" else \
        dict(env="stock", tickers=int(kind[1:]), turbulence_pct=90.0 if kind == "n100" else None)
    args = type("A", (), dict(envs_per_gpu=E, action_pool=8, rollout=0, desync=False, no_stats=False, **a))()
    w = bench.build_workload(args, torch, dev, 0)
    env = w.env
    if windows63:
        from finrl_amd.data import random_windows
        g = torch.Generator(device=dev).manual_seed(7)
        env.set_windows(*random_windows(env.panel.T, E, 63, generator=g, device=dev))
        kind = "portfolio-random63"
    pool = [torch.sort(a, dim=1).values.contiguous() for a in w.pool] if ascending else w.pool
    alternate(libs, envs, nat, torch, env, pool, kind + (" ascending" if ascending else ""), rounds)


def two_wave_ab(libs, nat, torch, dev, E, kind, rounds):
    import numpy as np
    import bench
    from finrl_amd.vec_cashpenalty import CashPenaltyPanel, VecCashPenaltyEnv, VecStopLossEnv
    name, cols, act, *win = kind.split(":")
    if win not in ([], ["win63"]):
        raise SystemExit(f"{kind}: the only fourth field is win63")
    T, N, Cc = bench.N_DAYS, bench.N_TICKERS, int(cols[1:])
    rng = np.random.default_rng(0)
    close = 50 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    panel = CashPenaltyPanel(close, rng.normal(0, 10, (T, N, Cc)), np.abs(rng.normal(0, 30, T)))
    cls = VecCashPenaltyEnv if name == "cashpenalty" else VecStopLossEnv
    env = cls(panel, E, hmax=2_000, random_start=True, discrete_actions={"disc": True, "cont": False}[act],
              device=dev, seed=0)
    gen = torch.Generator(device=dev).manual_seed(1234)
    pool = [torch.rand(E, N, generator=gen, device=dev) * 2.0 - 1.0 for _ in range(8)]
    if win:
        from finrl_amd.data import random_windows
        g = torch.Generator(device=dev).manual_seed(7)
        env.set_windows(*random_windows(T, E, 63, generator=g, device=dev))
    alternate(libs, dict.fromkeys(libs), nat, torch, env, pool, kind, rounds)


def alternate(libs, envs, nat, torch, env, pool, kind, rounds):
    env.reset()
    for i in range(2000):
        env.step(pool[i % 8])
    torch.cuda.synchronize()
    for r in range(rounds):
        for name in libs:
            nat._lib = libs[name]
            for k2, v2 in envs.items():      # clear the other runs' settings, apply this one's
                if v2:
                    os.environ.pop(v2.split("=")[0], None)
            if envs.get(name):
                os.environ[envs[name].split("=")[0]] = envs[name].split("=")[1]
            env._step_args = None                # BatchedEnv.step caches the previous library's function
            if hasattr(env, "hint_desynchronised"):
                # the stock handle keeps its step plan -- the kernel's address among it -- from the library that
                # planned it: have this one plan again (a change of the hint does), or both arms launch one kernel
                env.hint_desynchronised(True)
                env.hint_desynchronised(False)
            for i in range(100):
                env.step(pool[i % 8])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(500):
                env.step(pool[i % 8])
            e1.record()
            torch.cuda.synchronize()
            print(f"{kind} round {r} {name:8s} {e0.elapsed_time(e1) * 1e3 / 500:.2f} us", flush=True)


if __name__ == "__main__":
    main()
