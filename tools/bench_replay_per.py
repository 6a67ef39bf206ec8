#!/usr/bin/env python3
"""Time of prioritised replay (PrioritizedReplayBuffer: finenv_replay_per_*) on the set-up of
tools/bench_replay_nstep.py: the 16 x 65,536 DOW30 ring and the crypto ring, HIP events around `iters`
calls, an untimed warm-up, the variants ALTERNATING inside one process over `rounds` rounds.
Profiler off.

usage: python3 tools/bench_replay_per.py [--envs 65536] [--slots 16] [--batches 256,4096,65536]
                                         [--iters 200] [--rounds 3] [--out FILE.jsonl] [--md FILE.md]

Per ring and batch size B:
  (a) the uniform ReplayBuffer.sample and PrioritizedReplayBuffer.sample / .sample_nstep (n = 3):
      draw, descent and gather in one launch;
  (b) find + gather, the two-launch form, on 16 cycled sets of u made outside the timed window;
  (c) a torch formulation on the same u: cumsum over the tickets (held as int64 outside the timed
      window), searchsorted, five index gathers;
  (d) update_priorities(shaped=True) on 16 cycled sets of drawn pairs.
Then (e) PrioritizedReplayBuffer.step against ReplayBuffer.step on the stock env of bench.py, eager
and as a captured graph of one turn of the ring.

Asserted before anything is timed: find(u) is torch's searchsorted leaf, the fused sample's batch is
the gather of the pairs it reports, and its probabilities are ticket / total.

Bytes per sample of the fused draw: the gather's 2 * (4 D + 4 D) + 8 A + 21 (+ 8 for the pair, + 4
for the probability) plus the descent's 64 children per level: 3 levels of 512 B and the 256 B of
leaves, all but the leaves and level 1 shared by the whole batch and L2-resident."""
import torch

import replay_bench_common as rb
from replay_bench_common import POOL, rounds_of

GAMMA = 0.99


def main():
    args = rb.parse_args("bench_replay_per")
    import bench
    from finrl_amd import PrioritizedReplayBuffer, ReplayBuffer, StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    dev = torch.device("cuda", 0)
    E, S, pos = args.envs, args.slots, rb.HEAD_POS
    rep = rb.Report(args, "| shape | B | variant | us (best) | us per round | vs uniform sample |",
                    "|---|---:|---|---:|---|---:|")

    for shape, D, A, pitch in rb.SHAPES:
        uni = ReplayBuffer(S, E, D, A, obs_pitch=pitch, device=dev, seed=1)
        buf = PrioritizedReplayBuffer(S, E, D, A, obs_pitch=pitch, device=dev, seed=1)
        g = torch.Generator(device=dev).manual_seed(2)
        obs2, act2, rew2, done2 = rb.fill_ring(buf, g, twin=uni)
        # tickets of (|N(0, 1)| + eps)^0.6 TD errors; the head slot holds no complete transition
        w = (torch.randn(S, E, generator=g, device=dev).abs() + buf.eps) ** buf.alpha
        q = torch.clamp(torch.round(w.double() * 2.0 ** buf.frac_bits), 1, 2 ** 32 - 1).long()
        q[pos] = 0
        buf.tickets.copy_(torch.where(q >= 2 ** 31, q - 2 ** 32, q).to(torch.int32))
        buf.rebuild()
        total = buf.total
        assert total == int(q.sum())
        q_flat = q.view(-1)
        for B in args.batch_sizes:
            u_pool = [torch.randint(0, total, (B,), generator=g, device=dev, dtype=torch.int64)
                      for _ in range(POOL)]
            idx_pool, w_pool = [], []
            for _ in range(POOL):
                buf.sample(B)
                idx_pool.append(buf.last_indices.clone())
                w_pool.append((torch.randn(B, generator=g, device=dev).abs() + buf.eps) ** buf.alpha)
            k = [0]

            def torch_per():
                k[0] += 1
                c = torch.cumsum(q_flat, 0)
                flat = torch.searchsorted(c, u_pool[k[0] % POOL], right=True)
                nxt = (flat + E) % (S * E)
                return (obs2[flat], act2[flat], obs2[nxt], done2[flat].float(), rew2[flat], flat)

            def find_gather():
                k[0] += 1
                return buf.gather(buf.find(u_pool[k[0] % POOL]))

            def update():
                k[0] += 1
                buf.update_priorities(idx_pool[k[0] % POOL], w_pool[k[0] % POOL], shaped=True)

            k[0] = -1
            ref = torch_per()                              # same u -> the same leaves and batch
            pairs = buf.find(u_pool[0]).long()
            assert torch.equal(pairs[0] * E + pairs[1], ref[5])
            k[0] = -1
            got = find_gather()
            assert torch.equal(got.observations, ref[0][:, :D]) and torch.equal(got.actions, ref[1])
            assert torch.equal(got.next_observations, ref[2][:, :D])
            assert torch.equal(got.dones[:, 0], ref[3]) and torch.equal(got.rewards[:, 0], ref[4])
            smp = [t.clone() for t in buf.sample(B)]
            li = buf.last_indices.long()
            for a, b in zip(smp[:5], buf.gather(buf.last_indices)):
                assert torch.equal(a, b)
            want_p = (q_flat[li[0] * E + li[1]].double() / float(total)).float()
            assert torch.equal(smp[5][:, 0], want_p) and bool((want_p > 0).all())

            variants = {"uniform sample": lambda: uni.sample(B),
                        "prioritized sample (one launch)": lambda: buf.sample(B),
                        "prioritized sample_nstep n=3": lambda: buf.sample_nstep(B, 3, GAMMA),
                        "uniform sample_nstep n=3": lambda: uni.sample_nstep(B, 3, GAMMA),
                        "find + gather (two launches)": find_gather,
                        "torch cumsum + searchsorted + 5 gathers": torch_per}
            us = rounds_of(variants, args.iters, args.rounds)
            tickets_before = buf.tickets.clone()
            us.update(rounds_of({"update_priorities": update}, args.iters, args.rounds))
            buf.tickets.copy_(tickets_before)              # the timed draws of the next B see the same tree
            buf.rebuild()
            t_uni = min(us["uniform sample"])
            for name, v in us.items():
                best = min(v)
                rep.emit(dict(shape=shape, D=D, P=buf.obs_pitch, A=A, slots=S, envs=E, batch=B, variant=name,
                              iters=args.iters, us_per_call=[round(x, 2) for x in v], us_best=round(best, 2),
                              this_over_uniform=round(best / t_uni, 3)))
                rep.md.append(f"| {shape} (D={D}, P={buf.obs_pitch}, A={A}) | {B} | {name} | {best:.2f} | "
                              f"{', '.join(f'{x:.2f}' for x in v)} | {best / t_uni:.3f}x |")
        if D != 301:
            del uni, buf
        del obs2, act2, rew2, done2
        if D == 301:
            stock = (uni, buf)
        torch.cuda.empty_cache()

    # (e) the step: the stock env of bench.py at the same E, one env per buffer
    close, tech, risk = bench.synth_panel()
    g = torch.Generator(device=dev).manual_seed(3)
    pool = [torch.rand(E, 30, generator=g, device=dev) * 2 - 1 for _ in range(8)]
    variants = {}
    for name, b in zip(("ReplayBuffer.step", "PrioritizedReplayBuffer.step"), stock):
        env = VecStockTradingEnv(StockPanel(close, tech, risk), E, device=dev, **bench.ENV_KW)
        b.pos, b._n_valid = 0, 0
        b.start(env, env.reset())
        k = [0]

        def step(b=b, env=env, k=k):
            k[0] += 1
            b.step(env, pool[k[0] & 7])
        variants[name] = step

    rb.step_table(rep, args, variants)
    rep.close()


if __name__ == "__main__":
    main()
