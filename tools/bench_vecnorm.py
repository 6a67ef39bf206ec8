#!/usr/bin/env python3
"""Time of VecNormalize's launches (finenv_vecnorm_update / _apply / _step) beside the bare env step
and beside a torch formulation of the same update and normalise, in one process: HIP events around
`iters` calls, an untimed warm-up, the variants ALTERNATING over `rounds` rounds (the timing of
tools/replay_bench_common.py).  Profiler off.

usage: python3 tools/bench_vecnorm.py [--envs 65536] [--iters 200] [--rounds 3] [--out FILE.jsonl] [--md FILE.md]

Shapes: the DOW30 x 8 stock env of bench.py (D = 301, aligned pitch 304: 16-byte units) and VecCryptoEnv
at 10 pairs, 40 indicator columns, lookback 1 (D = 51, packed rows: dwords).

Variants: the update launch and the apply launch on the env's raw observation; norm.step (the env's
launch plus two) and its frozen form (plus one) beside the bare env.step, eager and as a captured graph
of 16 steps (eager calls include the host's time per launch); torch update (float64 mean, population
variance and the Chan merge, as SB3's RunningMeanStd states them) and torch normalise in float64 (the
kernel's formula, asserted equal to it bit for bit before anything is timed) and in float32.

Algorithmic bytes: 4 D E read for the update, 4 D E read + 4 D E written for the apply; the GB/s column
is those bytes over the best time."""
import numpy as np
import torch

import replay_bench_common as rb
from replay_bench_common import rounds_of

GRAPH_STEPS = 16


def envs_for(E, dev):
    import bench
    from finrl_amd import StockPanel
    from finrl_amd.vec_crypto import VecCryptoEnv
    from finrl_amd.vec_env import VecStockTradingEnv
    close, tech, risk = bench.synth_panel()
    yield "stock DOW30x8, aligned pitch", lambda: VecStockTradingEnv(
        StockPanel(close, tech, risk), E, device=dev, **bench.ENV_KW)
    rng = np.random.default_rng(0)
    T, N, W = 43_200, 10, 40
    price = 10.0 ** rng.uniform(0, 4.5, N) * np.exp(np.cumsum(rng.normal(0, 0.0005, (T, N)), axis=0))
    config = {"price_array": price, "tech_array": rng.normal(0, 3000, (T, W))}
    yield "crypto 10 pairs, packed rows", lambda: VecCryptoEnv(config, E, device=dev)


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_STEPS):
            fn()
    return graph.replay


def main():
    ap_args = rb.parse_args("bench_vecnorm")
    from finrl_amd import VecNormalize
    dev = torch.device("cuda", 0)
    E = ap_args.envs
    rep = rb.Report(ap_args, "| shape | variant | us (best) | us per round | algorithmic bytes | GB/s |",
                    "|---|---|---:|---|---:|---:|")
    for shape, make in envs_for(E, dev):
        env, frozen_env = make(), make()
        norm, frozen = VecNormalize(env), VecNormalize(frozen_env, training=False)
        D, P = norm.obs_dim, env.obs.stride(0)
        g = torch.Generator(device=dev).manual_seed(3)
        pool = [torch.rand(E, env.action_dim, generator=g, device=dev) * 2 - 1 for _ in range(8)]
        norm.reset()
        frozen.reset()
        for a in pool:                                  # statistics of a few real steps
            norm.step(a)
        frozen.load_state_dict(norm.state_dict())
        raw, rms = env.obs, norm.obs_rms
        out = torch.empty_like(norm._obs_buf)[:, :D]

        # the torch formulation on the same raw observation
        mean, var, count = rms.mean.clone(), rms.var.clone(), rms.count.clone()
        scale32, mean32 = rms.scale.float(), rms.mean.float()

        def torch_update():
            x = raw.double()
            bm, bv = x.mean(0), x.var(0, unbiased=False)
            delta, tot = bm - mean, count + E
            new_var = (var * count + bv * E + delta * delta * count * E / tot) / tot
            return mean + delta * E / tot, new_var, tot, 1.0 / torch.sqrt(new_var + 1e-8)

        def torch_norm64():
            return ((raw.double() - rms.mean) * rms.scale).clamp(-10.0, 10.0).float()

        def torch_norm32():
            return ((raw - mean32) * scale32).clamp(-10.0, 10.0)

        assert torch.equal(rms.apply(raw, out), torch_norm64())
        before = rms._block.clone()
        rms.update(raw)
        want = torch_update()
        assert torch.allclose(rms.var, want[1], rtol=1e-8, atol=0) and torch.equal(rms.count, want[2])
        rms._block.copy_(before)

        k = [0]

        def acts():
            k[0] += 1
            return pool[k[0] % len(pool)]

        variants = {
            "update launch": (lambda: rms.update(raw), 4 * D * E),
            "apply launch": (lambda: rms.apply(raw, out), 8 * D * E),
            "torch update (float64)": (torch_update, 4 * D * E),
            "torch normalise (float64)": (torch_norm64, 8 * D * E),
            "torch normalise (float32)": (torch_norm32, 8 * D * E),
            "env.step": (lambda: env.step(acts()), None),
            "norm.step": (lambda: norm.step(acts()), None),
            "norm.step, training=False": (lambda: frozen.step(acts()), None),
        }
        fixed = pool[0]
        for name, fn in (("env.step", lambda: frozen_env.step(fixed)), ("norm.step", lambda: norm.step(fixed)),
                         ("norm.step, training=False", lambda: frozen.step(fixed))):
            replay = graphed(fn)
            variants[f"{name}, per step of a {GRAPH_STEPS}-step graph"] = (replay, None)
        us = rounds_of({name: fn for name, (fn, _) in variants.items()}, ap_args.iters, ap_args.rounds)
        for name, v in us.items():
            per = GRAPH_STEPS if "graph" in name else 1
            v = [x / per for x in v]
            nbytes, best = variants[name][1], min(v)
            rate = None if nbytes is None else nbytes / (best * 1e-6) / 1e9
            rep.emit(dict(shape=shape, envs=E, D=D, P=P, variant=name, iters=ap_args.iters,
                          us_per_call=[round(x, 2) for x in v], us_best=round(best, 2),
                          algorithmic_bytes=nbytes, achieved_GBps=None if rate is None else round(rate, 1)))
            rep.md.append(f"| {shape} (E={E}, D={D}, P={P}) | {name} | {best:.2f} | "
                          f"{', '.join(f'{x:.2f}' for x in v)} | {'' if nbytes is None else nbytes} | "
                          f"{'' if rate is None else f'{rate:.0f}'} |")
        del env, frozen_env, norm, frozen, out, raw
        torch.cuda.empty_cache()
    rep.close()


if __name__ == "__main__":
    main()
