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
import torch

import replay_bench_common as rb
from replay_bench_common import PEAK_BYTES_PER_S, POOL, rounds_of, sample_bytes


def main():
    args = rb.parse_args("bench_replay")
    import bench
    from finrl_amd import ReplayBuffer, StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    dev = torch.device("cuda", 0)
    E, S = args.envs, args.slots
    rep = rb.Report(args, "| shape | B | variant | us (best) | us per round | GB/s | of 8 TB/s | vs torch |",
                    "|---|---:|---|---:|---|---:|---:|---:|")

    stock_buf = None
    for shape, D, A, pitch in rb.SHAPES:
        buf = ReplayBuffer(S, E, D, A, obs_pitch=pitch, device=dev, seed=1)
        obs2, act2, rew2, done2 = rb.fill_ring(buf, torch.Generator(device=dev).manual_seed(2))
        nbytes = sample_bytes(D, A)
        for B in args.batch_sizes:
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
                            "torch, 5 index gathers": torch_five}, args.iters, args.rounds)
            t_torch = min(us["torch, 5 index gathers"])
            for name, v in us.items():
                best = min(v)
                rate = nbytes * B / (best * 1e-6)
                rep.emit(dict(shape=shape, D=D, P=buf.obs_pitch, A=A, slots=S, envs=E, batch=B, variant=name,
                              iters=args.iters, us_per_call=[round(x, 2) for x in v], us_best=round(best, 2),
                              bytes_per_sample=nbytes, achieved_GBps=round(rate / 1e9, 1),
                              fraction_of_8TBps=round(rate / PEAK_BYTES_PER_S, 4),
                              torch_over_this=round(t_torch / best, 2)))
                rep.md.append(f"| {shape} (D={D}, P={buf.obs_pitch}, A={A}) | {B} | {name} | {best:.2f} | "
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

    rb.step_table(rep, args, {"env.step": plain, "env.step(out=ring slots), no put": ring_no_put,
                              "buf.step (put + env.step into the ring)": ring})
    rep.close()


if __name__ == "__main__":
    main()
