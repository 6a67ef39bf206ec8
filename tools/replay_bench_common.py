"""What tools/bench_replay.py, bench_replay_nstep.py and bench_replay_per.py share: the arguments, the
two ring shapes and their fill, the timing (HIP events around `iters` calls, 10 untimed warm-up calls
per variant, the variants ALTERNATING inside one process over `rounds` rounds, profiler off), the
JSON-lines / markdown report and the table of step variants, eager and as a captured graph."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12
POOL = 16            # sets of pairs (or of u) a variant cycles through: one repeated set would be served
#                      by the Infinity Cache (a 65,536-sample crypto batch reads 27 MB)
HEAD_POS = 3
SHAPES = (("stock DOW30x8", 301, 30, None), ("crypto 10 assets", 51, 10, "packed"))


def sample_bytes(D, A):
    return 2 * (4 * D + 4 * D) + 8 * A + 21


def parse_args(tool):
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
        sys.exit(f"{tool}: no HIP device (there is no CPU path to time)")
    args.batch_sizes = [int(x) for x in args.batches.split(",") if x]      # --batches "": the step part only
    return args


class Report:
    """One JSON line per record on stdout (and in --out), markdown rows kept for --md."""

    def __init__(self, args, *header):
        self.md, self.md_path = list(header), args.md
        self.out = open(args.out, "w") if args.out else None

    def emit(self, rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if self.out:
            self.out.write(line + "\n")
            self.out.flush()

    def close(self):
        if self.out:
            self.out.close()
        if self.md_path:
            with open(self.md_path, "w") as f:
                f.write("\n".join(self.md) + "\n")


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters           # us per call


def rounds_of(variants, iters, rounds):
    import torch
    for fn in variants.values():                       # untimed warm-up of every variant
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            us[name].append(timed(fn, iters))
    return us


def fill_ring(buf, g, twin=None):
    """Uniform rows, 1 % dones and a full ring with the head at HEAD_POS (in `twin`, a second buffer of
    the same shape, too) -> the flattened [S*E, ...] views of buf's obs, actions, rewards, dones that
    the torch formulations index."""
    import torch
    S, E, A, dev = buf.n_slots, buf.num_envs, buf.action_dim, buf.device
    for s in range(S):                                 # slot by slot: no 5 GB temporary
        buf._obs_buf[s].copy_(torch.rand(E, buf.obs_pitch, generator=g, device=dev))
        if twin is not None:
            twin._obs_buf[s].copy_(buf._obs_buf[s])
    buf.actions.copy_(torch.rand(S, E, A, generator=g, device=dev))
    buf.rewards.copy_(torch.rand(S, E, generator=g, device=dev))
    buf.dones.copy_((torch.rand(S, E, generator=g, device=dev) < 0.01).to(torch.uint8))
    for name in ("actions", "rewards", "dones") if twin is not None else ():
        getattr(twin, name).copy_(getattr(buf, name))
    for b in (buf,) if twin is None else (twin, buf):
        b.pos, b._n_valid = HEAD_POS, S - 1
        b.head.copy_(torch.tensor([HEAD_POS, S - 1], dtype=torch.int32))
    return (buf._obs_buf.view(S * E, buf.obs_pitch), buf.actions.view(S * E, A), buf.rewards.view(S * E),
            buf.dones.view(S * E))


def step_table(report, args, variants):
    """The step variants eager (one Python call per step; includes the host's time per call) and as a
    captured graph of S calls, a whole turn of the ring: what a launch-bound loop runs."""
    import torch
    S, E = args.slots, args.envs

    def graphed(fn):
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

    us = rounds_of(variants, args.iters, args.rounds)
    per_graph = rounds_of({name + f", {S} steps per graph replay": graphed(fn)
                           for name, fn in variants.items()}, max(args.iters // S, 10), args.rounds)
    us.update({name: [x / S for x in v] for name, v in per_graph.items()})
    report.md += ["", "| stock env, E = %d | us per step (best) | us per round |" % E, "|---|---:|---|"]
    for name, v in us.items():
        report.emit(dict(shape="stock DOW30x8", envs=E, slots=S, variant=name, iters=args.iters,
                         us_per_step=[round(x, 2) for x in v], us_best=round(min(v), 2)))
        report.md.append(f"| {name} | {min(v):.2f} | {', '.join(f'{x:.2f}' for x in v)} |")
