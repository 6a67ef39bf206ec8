#!/usr/bin/env python3
"""Time of the rollout buffer's shuffled minibatch (RolloutBuffer.minibatch: finenv_rollout_minibatch,
the permutation and the gather of six fields in one launch) beside its yardstick, what a user writes
in torch on the SAME tensors: one torch.randperm over the n_steps * E rows per epoch and, per
minibatch, a slice of it and six advanced-indexing gathers on flattened [M, ...] views (observations,
actions, values, log-probs, advantages, returns).  The per-epoch parts -- torch.randperm there,
next_epoch() here -- are timed on their own and charged to a minibatch at 1 / (minibatches per epoch).
Both walk the minibatches of an epoch in order, so neither re-reads rows the other does not.
HIP events around `iters` calls, an untimed warm-up, the variants ALTERNATING inside one process
(`rounds` rounds).  Profiler off.

Then the cost of the permutation's cycle walk: the same batch from M = 16 x 65,536 = 2^20 rows (the
Feistel domain is exactly M: no walk) and from M = 16 x 65,537 = 2^20 + 16 (domain 2^21: half of all
first passes land outside [0, M) and walk on; below a whole wave per sample the walk diverges).

usage: python3 tools/bench_rollout_minibatch.py [--envs 65536] [--slots 16] [--batches 256,4096,65536]
                                                [--iters 200] [--rounds 3] [--out FILE.jsonl] [--md FILE.md]
(--slots is n_steps.)

Shapes: the DOW30 x 8 stock env (D = 301, aligned pitch P = 304, A = 30) and VecCryptoEnv at 10 assets,
40 indicator columns, lookback 1 (D = 51 packed, A = 10).

Algorithmic bytes per sample, B_sample = 8 D + 8 A + 36:
    read   the observation row 4 D, the action row 4 A, four scalar words 16
    write  the observation row 4 D, the action row 4 A, four scalar words 16, the row number 4
Achieved bytes/s = B_sample * B / time; the fraction is of the 8 TB/s HBM peak."""
import torch

import replay_bench_common as rb
from replay_bench_common import PEAK_BYTES_PER_S, rounds_of


def minibatch_bytes(D, A):
    return 8 * D + 8 * A + 36


def filled(n_steps, E, D, A, pitch, dev, g):
    from finrl_amd import RolloutBuffer
    buf = RolloutBuffer(n_steps, E, D, A, device=dev, seed=1, obs_pitch=pitch or "aligned")
    for t in range(n_steps + 1):                           # slice by slice: no large temporary
        buf._obs_buf[t].copy_(torch.rand(E, buf.obs_pitch, generator=g, device=dev))
    for name in ("actions", "values", "log_probs", "advantages", "returns"):
        x = getattr(buf, name)
        x.copy_(torch.rand(x.shape, generator=g, device=dev))
    return buf


def main():
    args = rb.parse_args("bench_rollout_minibatch")
    dev = torch.device("cuda", 0)
    E, S = args.envs, args.slots
    rep = rb.Report(args, "| shape | M | B | variant | us (best) | us per round | GB/s | of 8 TB/s | vs torch |",
                    "|---|---:|---:|---|---:|---|---:|---:|---:|")
    g = torch.Generator(device=dev).manual_seed(2)

    for shape, D, A, pitch in rb.SHAPES:
        nbytes = minibatch_bytes(D, A)
        bufs = {"": filled(S, E, D, A, pitch, dev, g), ", walk": filled(S, E + 1, D, A, pitch, dev, g)}
        for B in args.batch_sizes:
            variants, per_epoch, n_mb = {}, {}, {}
            for tag, buf in bufs.items():
                M, P = buf.n_steps * buf.num_envs, buf.obs_pitch
                if B > M:
                    continue
                n_mb[tag] = nmb = M // B                  # whole minibatches only: every call moves B rows
                flat = (buf._obs_buf[:buf.n_steps].view(M, P), buf.actions.view(M, A), buf.values.view(M),
                        buf.log_probs.view(M), buf.advantages.view(M), buf.returns.view(M))
                state = {"k": -1, "perm": torch.randperm(M, device=dev)}

                def fused(buf=buf, state=state, nmb=nmb):
                    state["k"] = (state["k"] + 1) % nmb
                    return buf.minibatch(state["k"], B)

                def torch_six(flat=flat, state=state, nmb=nmb):
                    state["k"] = (state["k"] + 1) % nmb
                    idx = state["perm"][state["k"] * B:(state["k"] + 1) * B]
                    return tuple(x[idx] for x in flat)

                def randperm(state=state, M=M):
                    state["perm"] = torch.randperm(M, device=dev)

                got = buf.minibatch(0, B)                  # the same rows -> the same batch, bit for bit
                ref = tuple(x[buf.last_rows.long()] for x in flat)
                assert torch.equal(got.observations, ref[0][:, :D])
                assert all(torch.equal(a, b) for a, b in zip(got[1:], ref[1:]))
                assert buf.last_rows.long().max().item() < M
                variants["minibatch (permutation + gather, one launch)" + tag] = fused
                per_epoch["minibatch (permutation + gather, one launch)" + tag] = ("next_epoch" + tag, buf.next_epoch)
                if not tag:
                    variants["torch, slice of the permutation + 6 index gathers"] = torch_six
                    per_epoch["torch, slice of the permutation + 6 index gathers"] = ("torch.randperm", randperm)
            us = rounds_of(variants, args.iters, args.rounds)
            us_epoch = rounds_of(dict(per_epoch.values()), max(args.iters // 10, 10), args.rounds)
            total = {}
            for name, v in us.items():
                ep_name, _ = per_epoch[name]
                nmb = n_mb[", walk" if name.endswith(", walk") else ""]
                total[name] = min(v) + min(us_epoch[ep_name]) / nmb
            t_torch = total["torch, slice of the permutation + 6 index gathers"]
            for name, v in us.items():
                ep_name, _ = per_epoch[name]
                tag = ", walk" if name.endswith(", walk") else ""
                buf = bufs[tag]
                M = buf.n_steps * buf.num_envs
                best, tot = min(v), total[name]
                rate = nbytes * B / (tot * 1e-6)
                rep.emit(dict(shape=shape, D=D, P=buf.obs_pitch, A=A, n_steps=S, envs=buf.num_envs, rows=M,
                              batch=B, variant=name, iters=args.iters, us_per_call=[round(x, 2) for x in v],
                              us_best=round(best, 2), per_epoch=ep_name,
                              per_epoch_us=[round(x, 2) for x in us_epoch[ep_name]],
                              minibatches_per_epoch=n_mb[tag], us_with_epoch_share=round(tot, 2),
                              bytes_per_sample=nbytes, achieved_GBps=round(rate / 1e9, 1),
                              fraction_of_8TBps=round(rate / PEAK_BYTES_PER_S, 4),
                              torch_over_this=round(t_torch / tot, 2)))
                rep.md.append(f"| {shape} (D={D}, P={buf.obs_pitch}, A={A}) | {M} | {B} | {name} + "
                              f"{ep_name} / {n_mb[tag]} | {tot:.2f} | {', '.join(f'{x:.2f}' for x in v)} | "
                              f"{rate / 1e9:.1f} | {rate / PEAK_BYTES_PER_S:.2%} | {t_torch / tot:.2f}x |")
        del bufs
        torch.cuda.empty_cache()
    rep.close()


if __name__ == "__main__":
    main()
