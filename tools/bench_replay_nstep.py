#!/usr/bin/env python3
"""Time of the replay buffer's n-step sampler (ReplayBuffer.sample_nstep / .gather_nstep:
finenv_replay_sample_nstep / _gather_nstep, one launch) beside the one-step sampler and beside a
torch formulation of the same n-step batch, on the set-up of tools/bench_replay.py: one ring, the
SAME (slot, env) pairs for every variant (16 sets drawn by sample() and cycled: one repeated set
would be served by the Infinity Cache), HIP events around `iters` calls, an untimed warm-up, the
variants ALTERNATING inside one process over `rounds` rounds.  Profiler off.

usage: python3 tools/bench_replay_nstep.py [--envs 65536] [--slots 16] [--batches 256,4096,65536]
                                           [--iters 200] [--rounds 3] [--out FILE.jsonl] [--md FILE.md]

Variants: sample; sample_nstep at n = 1, 3, 5 (n = 1 against sample is the cost of the second round
trip: the same bytes, the next-observation row loaded after the length is known); gather;
gather_nstep at n = 3; torch at n = 3.

The torch formulation (asserted equal to the kernel's batch, bit for bit, before anything is timed):
the [B, n] window indices and the horizon mask are computed OUTSIDE the timed window, as the flat
indices of bench_replay.py's five gathers are; timed are two [B, n] gathers (rewards, dones), the
first-done mask by a cumulative sum, m, the float64 terms and their sum in step order (n - 1 adds: a
library reduction does not state its order), three row gathers (obs, action, the late next obs), and
the gathers of the last done and of the discount from a table of float32 powers.

Bytes per sample: B_sample + 5 h + 4 (+ 4 for the steps word the Python layer always asks for), with
B_sample = 2 * (4 D + 4 D) + 8 A + 21 as in bench_replay.py and h the mean horizon of the pairs used."""
import numpy as np
import torch

import replay_bench_common as rb
from replay_bench_common import PEAK_BYTES_PER_S, POOL, rounds_of, sample_bytes

GAMMA = 0.99
NS = (1, 3, 5)
N_TORCH = 3


def main():
    args = rb.parse_args("bench_replay_nstep")
    from finrl_amd import ReplayBuffer
    dev = torch.device("cuda", 0)
    E, S, pos = args.envs, args.slots, rb.HEAD_POS
    rep = rb.Report(args, "| shape | B | variant | us (best) | us per round | bytes / sample | GB/s | vs sample "
                    "| torch / this |", "|---|---:|---|---:|---|---:|---:|---:|---:|")

    # float32 powers of gamma by one multiply each, as the contract states them
    gtab_np = np.ones(max(NS) + 1, dtype=np.float32)
    for i in range(1, gtab_np.size):
        gtab_np[i] = gtab_np[i - 1] * np.float32(GAMMA)
    gtab = torch.from_numpy(gtab_np).to(dev)
    gtab64 = gtab.double()

    for shape, D, A, pitch in rb.SHAPES:
        buf = ReplayBuffer(S, E, D, A, obs_pitch=pitch, device=dev, seed=1)
        obs2, act2, rew2, done2 = rb.fill_ring(buf, torch.Generator(device=dev).manual_seed(2))
        base_bytes = sample_bytes(D, A)
        for B in args.batch_sizes:
            n = N_TORCH
            steps_i = torch.arange(n, device=dev)
            idx_pool, pre_pool, h_mean = [], [], {k: 0.0 for k in NS}
            for _ in range(POOL):
                buf.sample(B)
                idx = buf.last_indices.clone()
                idx_pool.append(idx)
                s, e = idx[0].long(), idx[1].long()
                ahead = (pos - 1 - s) % S
                for k in NS:
                    h_mean[k] += float(torch.clamp(ahead + 1, max=k).float().mean()) / POOL
                h = torch.clamp(ahead + 1, max=n)
                win = ((s[:, None] + steps_i) % S) * E + e[:, None]          # [B, n] flat (slot, env)
                pre_pool.append((s, e, win, steps_i[None, :] < h[:, None], h))
            k = [0]

            def torch_nstep():
                k[0] += 1
                s, e, win, inwin, h = pre_pool[k[0] % POOL]
                r, d = rew2[win], (done2[win] != 0) & inwin
                before = torch.cumsum(d, 1) - d.long()                        # dones before step i
                alive = inwin & (before == 0)
                m = alive.sum(1)
                terms = r.double() * gtab64[:n] * alive
                acc = terms[:, 0]
                for i in range(1, n):                                         # the stated order
                    acc = acc + terms[:, i]
                flat = win[:, 0]
                late = ((s + m) % S) * E + e
                last = torch.gather(win, 1, (m - 1)[:, None])[:, 0]
                return (obs2[flat], act2[flat], obs2[late], done2[last].float(), acc.float(), gtab[m], m)

            def pooled(fn):
                def call():
                    k[0] += 1
                    return fn(idx_pool[k[0] % POOL])
                return call

            k[0] = -1
            ref = torch_nstep()                            # same pairs -> the same batch, bit for bit
            got = buf.gather_nstep(idx_pool[0], n, GAMMA)
            assert torch.equal(got.observations, ref[0][:, :D]) and torch.equal(got.actions, ref[1])
            assert torch.equal(got.next_observations, ref[2][:, :D])
            assert torch.equal(got.dones[:, 0], ref[3]) and torch.equal(got.rewards[:, 0], ref[4])
            assert torch.equal(got.discounts[:, 0], ref[5]) and torch.equal(buf.last_steps.long(), ref[6])
            one = [t.clone() for t in buf.gather(idx_pool[0])]      # n = 1 is the one-step batch
            for a, b in zip(one, buf.gather_nstep(idx_pool[0], 1, GAMMA)):
                assert torch.equal(a, b)

            variants = {"sample": (lambda: buf.sample(B), None)}
            for kk in NS:
                variants[f"sample_nstep n={kk}"] = ((lambda kk=kk: buf.sample_nstep(B, kk, GAMMA)), kk)
            variants["gather"] = (pooled(buf.gather), None)
            variants[f"gather_nstep n={n}"] = (pooled(lambda i: buf.gather_nstep(i, n, GAMMA)), n)
            variants[f"torch n-step n={n}"] = (torch_nstep, n)
            us = rounds_of({name: fn for name, (fn, _) in variants.items()}, args.iters, args.rounds)
            t_sample, t_torch = min(us["sample"]), min(us[f"torch n-step n={n}"])
            for name, v in us.items():
                kk = variants[name][1]
                nbytes = base_bytes if kk is None else base_bytes + 5 * h_mean[kk] + 4 + 4
                best = min(v)
                rate = nbytes * B / (best * 1e-6)
                vs_torch = round(t_torch / best, 2) if kk == n else None
                rep.emit(dict(shape=shape, D=D, P=buf.obs_pitch, A=A, slots=S, envs=E, batch=B, variant=name,
                              gamma=GAMMA, iters=args.iters, us_per_call=[round(x, 2) for x in v],
                              us_best=round(best, 2), mean_horizon=None if kk is None else round(h_mean[kk], 3),
                              bytes_per_sample=round(nbytes, 1), achieved_GBps=round(rate / 1e9, 1),
                              fraction_of_8TBps=round(rate / PEAK_BYTES_PER_S, 4),
                              this_over_sample=round(best / t_sample, 3), torch_over_this=vs_torch))
                rep.md.append(f"| {shape} (D={D}, P={buf.obs_pitch}, A={A}) | {B} | {name} | {best:.2f} | "
                              f"{', '.join(f'{x:.2f}' for x in v)} | {nbytes:.1f} | {rate / 1e9:.1f} | "
                              f"{best / t_sample:.3f}x | {'' if vs_torch is None else f'{vs_torch:.2f}x'} |")
        del buf, obs2, act2, rew2, done2
        torch.cuda.empty_cache()
    rep.close()


if __name__ == "__main__":
    main()
