#!/usr/bin/env python3
"""Time of the replay buffer's fused sampler (ReplayBuffer.sample / .gather: finenv_replay_sample /
_gather, one launch) beside its yardstick, the torch formulation on the SAME ring and the SAME
(slot, env) pairs: five advanced-indexing gathers on flattened [S*E, ...] views (obs, next_obs,
action, reward, done), with the flat indices computed outside the timed window.  Both cycle through
the same 16 sets of pairs, drawn by sample(): one repeated set would be served by the Infinity Cache.
HIP events around `iters` calls, an untimed warm-up, the variants ALTERNATING inside one process
(`rounds` rounds, so the spread between rounds of one variant is on the same page as the difference
between two).  Then buf.step (finenv_replay_put + the env step into the ring) against a plain
env.step of the stock env and against env.step(out=ring slots) without the put, each eager (one
Python call per step) and as a captured graph of one turn of the ring (what a launch-bound loop
runs; the eager figures include the host's time per call).  Profiler off.

usage: python3 tools/bench_replay.py [--envs 65536] [--slots 16] [--batches 256,4096,65536]
                                     [--iters 200] [--rounds 3] [--out FILE.jsonl] [--md FILE.md]

Shapes: the DOW30 x 8 stock env (D = 301, aligned pitch P = 304, A = 30) and VecCryptoEnv at 10 assets,
40 indicator columns, lookback 1 (D = 51 packed, A = 10).

Algorithmic bytes per sample, B_sample = 2 * (4 D read + 4 D write) + 8 A + 21:
    read   two observation rows 8 D, the action row 4 A, reward 4, done 1, the index pair 8
    write  two observation rows 8 D, the action row 4 A, reward 4, done 4
(sample() writes the pair instead of reading it.)  Achieved bytes/s = B_sample * B / time; the
fraction is of the 8 TB/s HBM peak, which a gather from a 5 GB ring cannot exceed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12
POOL = 16            # sets of pairs the gather variants cycle through


def sample_bytes(D, A):
    return 2 * (4 * D + 4 * D) + 8 * A + 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--batches", default="256,4096,65536")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None, help="also write the tables as markdown")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_replay: no HIP device (there is no CPU path to time)")
    import bench
    from finrl_amd import ReplayBuffer, StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    dev = torch.device("cuda", 0)
    E, S = args.envs, args.slots
    out = open(args.out, "w") if args.out else None
    md = ["| shape | B | variant | us (best) | us per round | GB/s | of 8 TB/s | vs torch |",
          "|---|---:|---|---:|---|---:|---:|---:|"]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters           # us per call

    def rounds_of(variants, iters):
        for fn in variants.values():                       # untimed warm-up of every variant
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        us = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                us[name].append(timed(fn, iters))
        return us

    stock_buf = None
    for shape, D, A, pitch in (("stock DOW30x8", 301, 30, None), ("crypto 10 assets", 51, 10, "packed")):
        buf = ReplayBuffer(S, E, D, A, obs_pitch=pitch, device=dev, seed=1)
        g = torch.Generator(device=dev).manual_seed(2)
        for s in range(S):                                 # slot by slot: no 5 GB temporary
            buf._obs_buf[s].copy_(torch.rand(E, buf.obs_pitch, generator=g, device=dev))
        buf.actions.copy_(torch.rand(S, E, A, generator=g, device=dev))
        buf.rewards.copy_(torch.rand(S, E, generator=g, device=dev))
        buf.dones.copy_((torch.rand(S, E, generator=g, device=dev) < 0.01).to(torch.uint8))
        buf.pos, buf._n_valid = 3, S - 1                   # a full ring
        buf.head.copy_(torch.tensor([3, S - 1], dtype=torch.int32))
        obs2, act2 = buf._obs_buf.view(S * E, buf.obs_pitch), buf.actions.view(S * E, A)
        rew2, done2 = buf.rewards.view(S * E), buf.dones.view(S * E)
        nbytes = sample_bytes(D, A)
        for B in [int(x) for x in args.batches.split(",") if x]:      # --batches "": the step part only
            # POOL sets of pairs, cycled: repeating ONE set would serve its rows from the Infinity Cache
            # (a 65,536-sample crypto batch reads 27 MB) and time neither formulation on the ring
            idx_pool, flat_pool = [], []
            for _ in range(POOL):
                smp = buf.sample(B)
                idx = buf.last_indices.clone()
                idx_pool.append(idx)
                flat_pool.append((idx[0].long() * E + idx[1].long(),
                                  ((idx[0].long() + 1) % S) * E + idx[1].long()))
            k = [0]

            def torch_five():
                k[0] += 1
                flat, flat_next = flat_pool[k[0] % POOL]
                return (obs2[flat], act2[flat], obs2[flat_next], done2[flat], rew2[flat])

            def fused_gather():
                k[0] += 1
                return buf.gather(idx_pool[k[0] % POOL])

            k[0] = -1
            ref = torch_five()                             # same pairs -> the same batch, bit for bit
            got = buf.gather(idx_pool[0])
            assert torch.equal(got.observations, ref[0][:, :D]) and torch.equal(got.actions, ref[1])
            assert torch.equal(got.next_observations, ref[2][:, :D])
            assert torch.equal(got.dones[:, 0], ref[3].float()) and torch.equal(got.rewards[:, 0], ref[4])
            us = rounds_of({"sample (draw + gather + draw bump)": lambda: buf.sample(B),
                            "gather (caller pairs)": fused_gather,
                            "torch, 5 index gathers": torch_five}, args.iters)
            t_torch = min(us["torch, 5 index gathers"])
            for name, v in us.items():
                best = min(v)
                rate = nbytes * B / (best * 1e-6)
                emit(dict(shape=shape, D=D, P=buf.obs_pitch, A=A, slots=S, envs=E, batch=B, variant=name,
                          iters=args.iters, us_per_call=[round(x, 2) for x in v], us_best=round(best, 2),
                          bytes_per_sample=nbytes, achieved_GBps=round(rate / 1e9, 1),
                          fraction_of_8TBps=round(rate / PEAK_BYTES_PER_S, 4),
                          torch_over_this=round(t_torch / best, 2)))
                md.append(f"| {shape} (D={D}, P={buf.obs_pitch}, A={A}) | {B} | {name} | {best:.2f} | "
                          f"{', '.join(f'{x:.2f}' for x in v)} | {rate / 1e9:.1f} | "
                          f"{rate / PEAK_BYTES_PER_S:.2%} | {t_torch / best:.2f}x |")
        if pitch is None:
            stock_buf = buf
        else:
            del buf
        del obs2, act2, rew2, done2
        torch.cuda.empty_cache()

    # buf.step against a plain env.step: the stock env of bench.py at the same E
    close, tech, risk = bench.synth_panel()
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, device=dev, **bench.ENV_KW)
    g = torch.Generator(device=dev).manual_seed(3)
    pool = [torch.rand(E, 30, generator=g, device=dev) * 2 - 1 for _ in range(8)]
    k = [0]
    stock_buf.pos, stock_buf._n_valid = 0, 0
    stock_buf.start(env, env.reset())

    def plain():
        k[0] += 1
        env.step(pool[k[0] & 7])

    def ring():
        k[0] += 1
        stock_buf.step(env, pool[k[0] & 7])

    def ring_no_put():                                     # the env step into rotating ring slots alone
        k[0] += 1
        s = k[0] % S
        env.step(pool[k[0] & 7], out=(stock_buf.obs[(s + 1) % S], stock_buf.rewards[s], stock_buf.dones[s]))

    def graphed(fn):
        """S calls of fn captured once (a whole turn of the ring): what a launch-bound loop runs."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(S):
                fn()
        return graph.replay

    variants = {"env.step": plain, "env.step(out=ring slots), no put": ring_no_put,
                "buf.step (put + env.step into the ring)": ring}
    us = rounds_of(variants, args.iters)
    per_graph = rounds_of({name + f", {S} steps per graph replay": graphed(fn)
                           for name, fn in variants.items()}, max(args.iters // S, 10))
    us.update({name: [x / S for x in v] for name, v in per_graph.items()})
    md += ["", "| stock env, E = %d | us per step (best) | us per round |" % E, "|---|---:|---|"]
    for name, v in us.items():
        emit(dict(shape="stock DOW30x8", envs=E, slots=S, variant=name, iters=args.iters,
                  us_per_step=[round(x, 2) for x in v], us_best=round(min(v), 2)))
        md.append(f"| {name} | {min(v):.2f} | {', '.join(f'{x:.2f}' for x in v)} |")
    if out:
        out.close()
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
