#!/usr/bin/env python3
"""Cost of the episode history (enable_history) of the batched stock, portfolio, crypto, array-state
stock, cash-penalty or stop-loss env on bench.py's workload for that env: 65,536 envs x DOW30 x 8
indicators, 63-day episode windows
(crypto: 10 pairs x 40 indicator columns, 1,440-row windows, --envs 32768 / 65536 / 262144; stocknp:
64-row windows -- that env is done one step earlier, and the timed steps stay the same).  ONE process, ONE
env; the variants alternate inside every round, each timed with HIP events over steps that all record:
  a  history detached (the step path of a build without the feature)
  b  history attached without the per-ticker tensor (actions=False / weights=False)
       stock +12 B written per env and step; portfolio +20 B written, 8 B read; crypto +16 B
       written, 8 B read; stocknp +13 B written (asset, tag, len), 8 B read
  c  history attached with it: stock +12 + 4N B (the step kernel also writes `realised`);
       portfolio +20 + 4N B written; crypto +16 + 4N B written; stocknp +13 + 4N B written
  d  history detached, the host copy the history replaces after every step: one state_numpy()
     (portfolio: and one weights.cpu())
--env cashpenalty / stoploss (30 assets x 5 columns, starts pinned to each window's first row): the
record is a copy of the audit row taken by tw_history_record_kernel behind the step, so there is one
more variant, and b / c / d keep the audit block:
  u  history detached, audit block attached (the step kernel writes its 8 (4 + N) B row per env)
  b  history without transactions and actions: record_bytes_twowave(N, False) read / written
  c  history with both: record_bytes_twowave(N, True)
  d  history detached, one state_numpy() and one audit.cpu() after every step
usage: python3 tools/bench_history.py <lockstep|desync>
                                      [--env stock|portfolio|crypto|stocknp|cashpenalty|stoploss]
                                      [--variants a,b,c,d] [--rounds R] [--envs E] [--json PATH]
  lockstep  every env on the window [0, 63): one record row per step, written contiguously
  desync    random 63-day windows (stock: with hint_desynchronised(True)) and a random half of the envs
            restarted 31 steps after the others: neighbouring envs sit on different panel rows AND on
            different record rows
A round of a variant is: reset (arms every record), [desync: 31 steps, reset of a random half],
then the timed steps -- 62 (lockstep) or 31 (desync), none of them terminal, so every env records on
every timed step (asserted).  Rounds default to what gives at least 200 timed steps per variant.
--env crypto: windows of 1,440 rows, 64 timed steps per round in both cases (a record of 100 entries per
env, not of the whole window: 262,144 envs x 100 x (16 + 4N) B is 1.5 GB).
FINENV_LIB=<libfinenv.so of another build> times that build; one without the history entry points
can run variant a only (that is how a commit before the feature is measured with this same script).
Under `rocprofv3 --kernel-trace --stats -- python3 tools/bench_history.py lockstep --variants c` the
kernel stats give stock_history_record_kernel's own time (record_bytes() below is what it moves) or,
with `--env cashpenalty` / `--env stoploss`, tw_history_record_kernel's (record_bytes_twowave());
with `--env portfolio` / `--env crypto` / `--env stocknp`, the recording instantiation's of the step kernel."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 63
CRYPTO_WINDOW, CRYPTO_TIMED, CRYPTO_CAPACITY = 1440, 64, 100


def record_bytes(N, actions):
    """Bytes per env and step the record kernel needs: it reads len, flags (4 + 4), done (1), cash (8),
    price_day and day (4 + 4), N holdings (4N) [+ N realised trades (4N)] and writes asset, row and len
    (8 + 4 + 4) [+ N actions (4N)].  The N closes of the price row are shared by a lock-step batch."""
    return 25 + 4 * N + 16 + (8 * N if actions else 0)


def record_bytes_twowave(N, both):
    """(read, written) bytes per env and step of tw_history_record_kernel: it reads flags, len, ntx
    (12), done (1) and the audit head (32) [+ the N transactions of the audit row (8N) and the action row
    (4N)] and writes the four scalar columns (28), len and ntx (8) [+ transactions and actions (12N)]."""
    return 45 + (12 * N if both else 0), 36 + (12 * N if both else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=("lockstep", "desync"))
    ap.add_argument("--env", choices=("stock", "portfolio", "crypto", "stocknp", "cashpenalty",
                                     "stoploss"), default="stock")
    ap.add_argument("--variants", default=None)
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--json", default=None)
    o = ap.parse_args()
    twowave = o.env in ("cashpenalty", "stoploss")
    variants = (o.variants or ("a,u,b,c,d" if twowave else "a,b,c,d")).split(",")
    import torch
    import bench
    from finrl_amd import _native as nat
    from finrl_amd.data import random_windows
    if not torch.cuda.is_available():
        sys.exit("bench_history: no HIP device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    E = o.envs
    args = type("A", (), dict(envs_per_gpu=E, action_pool=8, rollout=0, desync=False, no_stats=False,
                              env=o.env, tickers=30, turbulence_pct=None))()
    w = bench.build_workload(args, torch, dev, 0)
    stock, crypto, stocknp = o.env == "stock", o.env == "crypto", o.env == "stocknp"
    env, N = w.env, w.env.action_dim if crypto or stocknp or twowave else w.env.stock_dim
    if twowave:                                 # every env starts on its window's first row
        env.random_start = False
        env._call("set_random_start", 0, 0)
        env.set_next_start(0)
        audit = C.c_void_p(env.enable_audit().data_ptr())
    window = CRYPTO_WINDOW if crypto else WINDOW + stocknp
    rows = env.price_array.shape[0] if crypto else env.price_ary.shape[0] if stocknp else env.panel.T
    has_api = hasattr(nat.lib(), f"finenv_{o.env}_set_history")
    if not has_api and variants != ["a"]:
        sys.exit(f"bench_history: this libfinenv.so has no {o.env} history; it can run --variants a only")
    desync = o.case == "desync"
    gen = torch.Generator(device=dev).manual_seed(7)
    if desync:
        env.set_windows(*random_windows(rows, E, window, generator=gen, device=dev))
        if stock:
            env.hint_desynchronised(True)
    else:
        env.set_windows(0, window)
    timed = CRYPTO_TIMED if crypto else (31 if desync else WINDOW - 1)
    rounds = o.rounds or -(-200 // timed)
    half = (torch.rand(E, generator=gen, device=dev) < 0.5).to(torch.uint8)

    hists = {}
    if has_api:
        from finrl_amd import history as H
        for v, per_ticker in (("b", False), ("c", True)):
            if v in variants:
                hists[v] = H.EpisodeHistory(env, WINDOW, actions=per_ticker) if stock else \
                    H.TwoWaveEpisodeHistory(env, WINDOW, per_ticker, per_ticker) if twowave else \
                    H.CryptoEpisodeHistory(env, CRYPTO_CAPACITY, stocks=per_ticker) if crypto else \
                    H.StockNpEpisodeHistory(env, window, stocks=per_ticker) if stocknp else \
                    H.PortfolioEpisodeHistory(env, WINDOW, weights=per_ticker)
    # the step's optional per-ticker output: stock `realised`, enabled by variant c's history and passed
    # to its steps only; portfolio `weights`, variant d's host copy
    # (the crypto and stocknp steps have no such output)
    extra, extra_v = ("realised", "c") if stock else ("weights", "d")
    if o.env == "portfolio" and "d" in variants:
        env.enable_weights()
    extra_out = getattr(env, extra, None)

    def select(v):
        if has_api:
            env._call("set_history", C.byref(hists[v]._ptrs) if v in hists else None)
        if twowave:
            env._call("set_audit", None if v == "a" else audit)
        elif not (crypto or stocknp):
            setattr(env, extra, extra_out if v == extra_v else None)
        env._step_args = None                   # BatchedEnv.step caches the output pointers

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
                if o.env == "portfolio":
                    env.weights.cpu()
                if twowave:
                    env.audit.cpu()
        e1.record()
        torch.cuda.synchronize()
        if record:
            times[v].append(e0.elapsed_time(e1) * 1e3 / timed)
        if v in hists:                          # every env recorded on every timed step
            h = hists[v]
            assert int(h.length.min()) >= timed + (not twowave) and not bool(h.complete.any()) \
                and not bool(h.overflow.any()), "a timed step did not record"

    times = {v: [] for v in variants}
    for v in variants:                          # warm-up: every variant's shapes, untimed
        one_round(v, False)
    for r in range(rounds):
        for v in variants:
            one_round(v, True)
    res = dict(case=o.case, env=o.env, envs=E, tickers=N, window=window, timed_steps_per_variant=timed * rounds,
               lib=os.path.abspath(nat.LIB_PATH), us_per_step={}, rounds_us={})
    for v in variants:
        t = sorted(times[v])
        res["us_per_step"][v] = round(t[len(t) // 2], 2)
        res["rounds_us"][v] = [round(x, 2) for x in times[v]]
    if stock:
        res["added_bytes_per_env_step"] = {"b": 12, "c": 12 + 4 * N}
        res["record_kernel_bytes_per_env_step"] = {"b": record_bytes(N, False), "c": record_bytes(N, True)}
    elif crypto:
        res["added_bytes_written_per_env_step"] = {"b": 16, "c": 16 + 4 * N}
        res["added_bytes_read_per_env_step"] = {"b": 8, "c": 8}
    elif stocknp:
        res["added_bytes_written_per_env_step"] = {"b": 13, "c": 13 + 4 * N}
        res["added_bytes_read_per_env_step"] = {"b": 8, "c": 8}
    elif twowave:
        res["audit_row_bytes_per_env_step"] = 8 * (4 + N)
        res["record_kernel_bytes_read_written_per_env_step"] = {
            "b": record_bytes_twowave(N, False), "c": record_bytes_twowave(N, True)}
    else:
        res["added_bytes_written_per_env_step"] = {"b": 20, "c": 20 + 4 * N}
    line = json.dumps(res)
    print(line, flush=True)
    if o.json:
        with open(o.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
