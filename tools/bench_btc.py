#!/usr/bin/env python3
"""Step time of the batched BitcoinEnv (VecBitcoinEnv, finenv_btc_step) beside its yardstick, the
batched CryptoEnv at one asset (VecCryptoEnv, N = 1, W = 7, lookback 1): HIP events around `steps`
launches, an untimed prewarm, the two envs ALTERNATING inside one process (`rounds` rounds, so that
the spread between rounds of the same env is on the same page as the difference between the two).
Profiler off; for kernel times run it under `rocprofv3 --kernel-trace --stats` with --profile (one
size, fewer steps).

usage: python3 tools/bench_btc.py [--envs 65536,262144,1048576] [--steps 400] [--rounds 3]
                                  [--rows 512] [--profile] [--out FILE.jsonl]

Algorithmic bytes per env-step, B = 4 D + 97 with D = P + 9 (P = 1: 137 B):
    read   action 4, account / stocks / total_asset / gamma_return 4 x 8, day 4, stocks tag 4
    write  the same four f64 fields 32, day 4, tag 4, last_reward 8, observation 4 D, reward 4, done 1
(the panel rows -- two prices and one template row per WAVE in lock step -- are shared and stay in
cache).  Fraction of peak = B * E / time / 8 TB/s.  The yardstick's own count is 4 D' + 12 N + 69
= 117 B at D' = 1 + N + W = 9: its state is smaller (three f64 fields read, f32 holdings).
A bound by bytes shows as a time that grows in proportion to E; a latency bound as a time that
does not."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12


def btc_bytes(P):
    return 4 * (P + 9) + 97


def crypto_bytes(N, W):
    # read: action 4 N, cash / total_asset / gamma_return 24, time 4, holdings 4 N; written: cash,
    # total_asset, gamma_return, last_reward 32, time 4, holdings 4 N, observation 4 D', reward 4, done 1
    return 4 * (1 + N + W) + 12 * N + 69


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="65536,262144,1048576")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--profile", action="store_true", help="one short untimed pass per env (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_btc: no HIP device (there is no CPU path to time)")
    from finrl_amd.vec_btc import VecBitcoinEnv
    from finrl_amd.vec_crypto import VecCryptoEnv
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    T, P, W = args.rows, 1, 7
    price = 30000.0 * np.exp(np.cumsum(rng.normal(0, 0.002, (T, P)), axis=0))
    tech = rng.normal(0, 3000.0, (T, W))
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(env, pool, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            env.step(pool[i & 7])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps          # us per step

    for E in [int(x) for x in args.envs.split(",")]:
        g = torch.Generator(device=dev).manual_seed(1)
        pool = [torch.rand(E, 1, generator=g, device=dev) * 2 - 1 for _ in range(8)]
        envs = {
            "btc": VecBitcoinEnv(price, tech, E, device=dev),
            "crypto_n1": VecCryptoEnv({"price_array": price, "tech_array": tech}, E, lookback=1, device=dev),
        }
        # the same batch out of lock step: a masked reset every few steps leaves the envs of every
        # wave on different days (per-env template rows instead of one per wave)
        desync = VecBitcoinEnv(price, tech, E, device=dev)
        desync.reset()
        for k in range(48):
            desync.step(pool[k & 7])
            if k % 4 == 3:
                desync.reset(torch.rand(E, generator=g, device=dev) < 0.3)
        envs["btc_desync"] = desync
        nbytes = {"btc": btc_bytes(P), "btc_desync": btc_bytes(P), "crypto_n1": crypto_bytes(1, W)}
        for name in ("btc", "crypto_n1"):
            envs[name].reset()
        steps = 20 if args.profile else args.steps
        for env in envs.values():                          # untimed prewarm
            for i in range(50 if not args.profile else 5):
                env.step(pool[i & 7])
        torch.cuda.synchronize()
        if args.profile:
            for env in envs.values():
                timed(env, pool, steps)
            continue
        us = {name: [] for name in envs}
        for _ in range(args.rounds):                       # alternating: btc, yardstick, desync, btc, ...
            for name, env in envs.items():
                us[name].append(timed(env, pool, steps))
        for name, v in us.items():
            best = min(v)
            emit(dict(env=name, envs=E, rows=T, steps=steps, us_per_step=[round(x, 3) for x in v],
                      us_best=round(best, 3), env_steps_per_s=round(E / best * 1e6),
                      bytes_per_env_step=nbytes[name],
                      fraction_of_8TBps=round(nbytes[name] * E / (best * 1e-6) / PEAK_BYTES_PER_S, 4)))
        del envs, desync, pool
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
