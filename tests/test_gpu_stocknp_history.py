"""Episode history of the batched array-state stock env (VecStockTradingEnvNP.enable_history(),
finenv_stocknp_set_history) on the MI355X: the record written by the step kernel against the reference
fixtures, the ElegantRL prediction loop, a host tracker that restates the header's recording rule and
is fed by one CPU oracle per env, inside a captured graph, detached, past 4 GiB, and its metrics.  The
recorded values are the step's own, so every comparison with the fixtures, with this build's step and
with oracle.stocknp.StockNpOracle is exact (tolerance 0)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import harness_loops as hl  # noqa: E402
from test_stocknp_history_abi import NAMES, SCALARS, _initial  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
COMPLETE, OVERFLOW = 1, 2
SENTINEL = -7
TAG_SENTINEL = SENTINEL & 0xFF                     # the u8 tensor's fill pattern
TENSORS = ("asset", "tag", "stocks", "start", "length", "flags")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(rng, T, N, K):
    price = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    return price, rng.normal(0, 50, (T, N * K)), np.abs(rng.normal(0, 70, T))


def _config(price, tech, turb, if_train=False):
    return {"price_array": price, "tech_array": tech, "turbulence_array": turb, "if_train": if_train}


def _u8(mask):
    return torch.from_numpy(np.asarray(mask).astype(np.uint8)).cuda()


def _host(hist):
    return {k: getattr(hist, k).cpu().numpy() if getattr(hist, k) is not None else None for k in TENSORS}


def _fill(hist):
    """The fill pattern in every tensor, nobody armed."""
    for k in ("asset", "stocks", "start"):
        if getattr(hist, k) is not None:
            getattr(hist, k).fill_(SENTINEL)
    if hist.tag is not None:
        hist.tag.fill_(TAG_SENTINEL)
    hist.length.zero_()
    hist.flags.zero_()


def _shorten(env, hist, cap):
    """Tell the kernel a capacity shorter than the tensors: the rows past it must keep their pattern."""
    hist._ptrs.capacity = cap
    env._call("set_history", C.byref(hist._ptrs))


# ------------------------------------------------------------------------------------------
# 1. the reference fixtures
# ------------------------------------------------------------------------------------------
def _fixture_env(name, E=70):
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    z = np.load(os.path.join(GOLDEN, f"stocknp_{name}.npz"), allow_pickle=False)
    cap, ms, bc, sc, g = z["cfg_float"].tolist()
    extra = {}
    if "obs_amount_floor" in z.files:            # StockEnvNAS100 fixtures (env_nas100_wrds.py)
        extra = dict(obs_amount_floor=float(z["obs_amount_floor"]),
                     turbulence_thresh=float(z["turbulence_thresh"]))
    env = VecStockTradingEnvNP(_config(z["price_array"], z["tech_array"], z["turbulence_array"]), E,
                               gamma=g, max_stock=ms, initial_capital=cap, buy_cost_pct=bc,
                               sell_cost_pct=sc, auto_reset=True, **extra)
    return z, env


def _fixture_episode(z, r):
    """The record the r-th episode of the fixture must leave: entry 0 the armed one."""
    marks = z["reset_step"].tolist() + [len(z["done"]) - 1]
    s0, s1 = marks[r] + 1, marks[r + 1]
    first = _initial(z, r)
    asset = np.concatenate([[float(first)], z["total_asset"][s0:s1 + 1]])
    tag = np.concatenate([[SCALARS.index(type(first))], z["ta_tag"][s0:s1 + 1]]).astype(np.uint8)
    stocks = np.concatenate([z["reset_stocks0"][r:r + 1], z["stocks"][s0:s1 + 1]])
    return dict(first=s0, last=s1, asset=asset, tag=tag, stocks=stocks, n=len(asset))


def _assert_fixture_record(hist, ep, E, what):
    h = _host(hist)
    n = ep["n"]
    np.testing.assert_array_equal(h["length"], n, err_msg=what)
    np.testing.assert_array_equal(h["flags"], COMPLETE, err_msg=what)
    np.testing.assert_array_equal(h["start"], 0, err_msg=what)
    np.testing.assert_array_equal(h["asset"][:n], np.broadcast_to(ep["asset"][:, None], (n, E)), err_msg=what)
    np.testing.assert_array_equal(h["tag"][:n], np.broadcast_to(ep["tag"][:, None], (n, E)), err_msg=what)
    np.testing.assert_array_equal(h["stocks"][:n], np.broadcast_to(ep["stocks"][:, :, None],
                                                                  ep["stocks"].shape + (E,)), err_msg=what)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_episodes_are_recorded_under_auto_reset(name):
    """E = 70 (a full wave and a 6-lane tail), auto_reset=True, every env fed the fixture's actions: after
    the first done the record is the first episode's total_asset / ta_tag / stocks -- the terminal values
    the state no longer holds -- and stays so through the second episode; reset() re-arms and the second
    record is the second episode."""
    _need_gpu()
    assert len(NAMES) == 10
    z, env = _fixture_env(name)
    E, N = env.num_envs, env.action_dim
    T = z["price_array"].shape[0]

    def start(r):
        env.set_start_state(z["reset_stocks0"][r], z["reset_amount0"][r], z["reset_amount0_tag"][r])

    def step(s):
        return env.step(torch.from_numpy(np.broadcast_to(z["actions"][s], (E, N)).copy()).cuda())

    start(0)
    env.reset()
    hist = env.enable_history()
    assert env.enable_history(capacity=3) is hist is env.history
    assert hist.capacity == T == env.max_step + 1
    assert hist.nbytes == E * (9 * T + 12) + 4 * E * N * T
    assert tuple(hist.stocks.shape) == (T, N, E) and hist.tag.dtype == torch.uint8
    np.testing.assert_array_equal(hist.length.cpu().numpy(), 1)      # armed from the current state
    ep0, ep1 = _fixture_episode(z, 0), _fixture_episode(z, 1)
    start(1)                                             # what the auto-reset of the first end restores
    for s in range(ep1["last"] + 1):
        _, _, done, _ = step(s)
        assert bool(done.all()) == bool(z["done"][s])
        if s == ep0["last"]:
            _assert_fixture_record(hist, ep0, E, f"{name} first episode")
            st = env.state_numpy()                       # ... and the env was reset in the same launch
            assert (st["day"] == 0).all() and (st["total_asset"] == float(_initial(z, 1))).all()
            assert (st["total_asset"] != ep0["asset"][-1]).all()
        if s == ep0["last"] + 3:
            _assert_fixture_record(hist, ep0, E, f"{name} first episode, three steps later")
    _assert_fixture_record(hist, ep0, E, f"{name} first episode at the second end")
    # the readers, from the device tensors: values and element types of the reference's list
    want = [SCALARS[t](x) for x, t in zip(ep0["asset"].tolist(), ep0["tag"].tolist())]
    for got in hist.episode_total_assets([0, 63, 64, E - 1]):
        assert got == want and [type(x) for x in got] == [type(x) for x in want]
    ret = hist.episode_returns(E - 1)
    assert float(ret[-1]) == z["episode_return"][ep0["last"]] and len(ret) == ep0["n"] - 1
    assert all(type(r) is type(x / want[0]) and r == x / want[0] for r, x in zip(ret, want[1:]))
    np.testing.assert_array_equal(hist.account_values(64), ep0["asset"])
    np.testing.assert_array_equal(hist.positions(69), ep0["stocks"])
    np.testing.assert_array_equal(hist.rows(1), np.arange(ep0["n"]))
    # reset() re-arms: the second episode again, from its start state
    start(1)
    env.reset()
    h = _host(hist)
    assert (h["length"] == 1).all() and not h["flags"].any()
    for s in range(ep1["first"], ep1["last"] + 1):
        step(s)
    _assert_fixture_record(hist, ep1, E, f"{name} second episode")


# ------------------------------------------------------------------------------------------
# 2. the ElegantRL prediction loop on windows, no state_numpy() in the loop
# ------------------------------------------------------------------------------------------
def test_elegantrl_prediction_loop_reads_the_curves_afterwards():
    """The harness_erl_stocknp panel at three offsets of one NaN-padded panel, E = 3, auto_reset=True:
    the loop only steps; afterwards each env's record is the reference loop's two lists."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    z = np.load(os.path.join(GOLDEN, "harness_erl_stocknp.npz"), allow_pickle=False)
    T, N, K = z["cfg_int"].tolist()
    offs = np.array([2, 2 + T + 1, 2 + 2 * T + 6])
    P = int(offs[2]) + T + 3
    arrays = []
    for a in (z["price_array"], z["tech_array"], z["turbulence_array"]):
        big = np.full((P,) + a.shape[1:], np.nan, dtype=a.dtype)
        for o in offs:
            big[o:o + T] = a
        arrays.append(big)
    with np.errstate(invalid="ignore"):
        env = VecStockTradingEnvNP(_config(*arrays), 3, auto_reset=True, windows=(offs, offs + T))
    hist = env.enable_history()
    assert hist.capacity == T
    acts = [hl.scripted_act(z["base"], 3 + np.arange(N)) for _ in range(3)]
    obs = env.reset().cpu().numpy()
    for i in range(env.max_step):
        a = np.concatenate([act(obs[e:e + 1]) for e, act in enumerate(acts)])
        o, _, done, _ = env.step(torch.from_numpy(a).cuda())
        obs = o.cpu().numpy()                           # (the policy's input; the state is never read)
        assert bool(done.all()) == (i == env.max_step - 1)
    assert bool(hist.complete.all()) and not bool(hist.overflow.any())
    for e, (assets, returns) in enumerate(zip(hist.episode_total_assets([0, 1, 2]),
                                              hist.episode_returns([0, 1, 2]))):
        np.testing.assert_array_equal(np.asarray(assets, np.float64), z["episode_total_assets"], err_msg=str(e))
        np.testing.assert_array_equal(np.asarray(returns, np.float64), z["episode_returns"], err_msg=str(e))
        np.testing.assert_array_equal(hist.rows(e), offs[e] + np.arange(T))
    assert {type(x) for x in hist.episode_total_assets(0)} <= {float, np.float32, np.float64}


# ------------------------------------------------------------------------------------------
# 3. the recording rule against a host tracker fed by one oracle per env
# ------------------------------------------------------------------------------------------
class _Oracles:
    """One StockNpOracle(price[s:t], tech[s:t], turb[s:t], n_envs=1) per env, stepped WITHOUT
    auto-reset so that the values of a terminal step can be read before reset() (which is what an
    auto-reset is)."""

    def __init__(self, arrays, s, t, starts, **kw):
        self.arrays, self.kw = arrays, kw
        self.s = np.array(s, dtype=np.int64)
        self.orc = [None] * len(self.s)
        self.starts = starts
        for e in range(len(self.s)):
            self.restart(e, int(s[e]), int(t[e]))

    def restart(self, e, s, t):
        """Env e on a fresh oracle on [s, t), reset from its start state."""
        from oracle.stocknp import StockNpOracle
        self.s[e] = s
        self.orc[e] = StockNpOracle(*(a[s:t] for a in self.arrays), n_envs=1, **self.kw)
        self.set_initial(self.starts, [e])
        self.orc[e].reset()

    def set_initial(self, starts, envs=None):
        self.starts = starts
        for e in range(len(self.orc)) if envs is None else envs:
            self.orc[e].set_initial(*(x[e:e + 1] for x in starts))

    def reset(self, mask):
        for e in np.flatnonzero(mask):
            self.orc[e].reset()

    def step(self, actions):
        return np.array([o.vec_step(actions[e:e + 1], auto_reset=False)[2][0]
                         for e, o in enumerate(self.orc)])

    def snapshot(self):
        sts = [o.state() for o in self.orc]
        st = {k: np.concatenate([x[k] for x in sts]) for k in ("total_asset", "ta_tag", "stocks", "day")}
        st["day"] = st["day"] + self.s                                    # the panel row
        return st


class _Tracker:
    """The recording rule of include/finenv.h, restated on the host."""

    def __init__(self, E, N, cap, rows):
        self.cap = cap
        self.asset = np.full((rows, E), float(SENTINEL))
        self.tag = np.full((rows, E), TAG_SENTINEL, np.uint8)
        self.stocks = np.full((rows, N, E), SENTINEL, np.float32)
        self.start = np.full(E, SENTINEL, np.int32)
        self.length = np.zeros(E, np.int32)
        self.flags = np.zeros(E, np.int32)

    def arm(self, mask, st):
        j = np.flatnonzero(mask)
        self.asset[0, j], self.tag[0, j] = st["total_asset"][j], st["ta_tag"][j]
        self.stocks[0][:, j] = st["stocks"][j].T
        self.start[j], self.length[j], self.flags[j] = st["day"][j], 1, 0

    def step(self, st, done):
        live = (self.length >= 1) & ((self.flags & COMPLETE) == 0)
        room = live & (self.length < self.cap)
        j = np.flatnonzero(room)
        k = self.length[j]
        self.asset[k, j], self.tag[k, j] = st["total_asset"][j], st["ta_tag"][j]
        self.stocks[k, :, j] = st["stocks"][j]
        self.length[j] = k + 1
        self.flags[live & ~room] |= OVERFLOW
        self.flags[live & done] |= COMPLETE

    def assert_equals(self, hist, what):
        h = _host(hist)
        for k in TENSORS:
            np.testing.assert_array_equal(h[k], getattr(self, k), err_msg=f"{k} {what}")


def _start_states(rng, E, N, cap):
    """Per-env start states, a mix of Python-float and float32 amounts (eval / train style)."""
    st0 = rng.integers(0, 20, (E, N)).astype(np.float32)
    tag0 = rng.integers(0, 2, E).astype(np.int32)
    am0 = np.where(tag0 == 1, (cap * rng.uniform(0.9, 1.1, E)).astype(np.float32),
                   cap * rng.uniform(0.9, 1.1, E))
    return st0, am0, tag0


def _drawn(env):
    st = env.state_numpy()
    return st["stocks0"], st["amount0"], st["amount0_tag"]


RULE_CASES = [
    dict(E=70, T=24, N=3, K=2, win=True, auto=True, short=True),
    dict(E=70, T=12, N=1, K=0, win=False, auto=False),
    dict(E=300, T=20, N=30, K=8, win=True, auto=False, short=True),   # two blocks, DOW30 rows
    dict(E=300, T=14, N=32, K=1, win=False, auto=True),               # N at the limit
    dict(E=70, T=16, N=30, K=8, win=False, auto=True, short=True, train=True),
    dict(E=300, T=30, N=3, K=2, win=True, auto=True, train=True),
    dict(E=70, T=10, N=32, K=1, win=True, auto=False),
    dict(E=300, T=8, N=1, K=0, win=False, auto=True, short=True),
]


def _case_id(c):
    return "E{E}-N{N}-T{T}".format(**c) + "".join(
        f"-{k}" for k in ("win", "auto", "train", "short") if c.get(k))


@pytest.mark.parametrize("cfg", RULE_CASES, ids=_case_id)
def test_recording_rule_against_a_host_tracker(cfg):
    _need_gpu()
    from finrl_amd.vec_stocknp import TAG_F32, VecStockTradingEnvNP
    E, T, N, K = cfg["E"], cfg["T"], cfg["N"], cfg["K"]
    win, auto, short, train = cfg["win"], cfg["auto"], cfg.get("short", False), cfg.get("train", False)
    rng = np.random.default_rng(E + 7 * N + T + auto)
    arrays = _panel(rng, T, N, K)
    if win:                                              # random windows of mixed lengths
        length = rng.integers(4, min(T, 13) + 1, E)
        s = (rng.random(E) * (T - length + 1)).astype(np.int64)
        t = s + length
    else:
        s, t = np.zeros(E, np.int64), np.full(E, T, np.int64)
    kw = dict(gamma=0.98, initial_capital=2e5, buy_cost_pct=0.0012, sell_cost_pct=0.0008)
    env = VecStockTradingEnvNP(_config(*arrays, if_train=train), E, auto_reset=auto, seed=E + N,
                               windows=(s, t) if win else None, **kw)
    if not train:
        env.set_start_state(*_start_states(rng, E, N, 2e5))
    env.reset()                                          # (train mode: draws the start states)
    starts = _drawn(env)
    assert not train or (starts[2] == TAG_F32).all()
    orc = _Oracles(arrays, s, t, starts, **kw)
    longest = int((t - s).max())                         # entries of the longest episode
    assert env.max_step + 1 == longest
    rows = longest + 2
    hist = env.enable_history(capacity=rows)
    cap = 4 if short else longest
    _shorten(env, hist, cap)
    _fill(hist)
    trk = _Tracker(E, N, cap, rows)
    # never armed: only where nothing on the host has to reset them (auto-reset keeps them running)
    never = (rng.random(E) < 0.1) if auto else np.zeros(E, bool)
    never[1] = auto

    def host_reset(mask):
        """env.reset(mask) and what it means for the twins: in train mode every env's start state is
        redrawn, the envs of the mask restart (on it) and are armed."""
        env.reset(_u8(mask))
        if train:
            orc.set_initial(_drawn(env))
        orc.reset(mask)
        trk.arm(mask, orc.snapshot())

    host_reset(~never)
    trk.assert_equals(hist, "after the first reset")
    steps = 2 * longest + 6
    ends = np.zeros(E, int)
    both = np.zeros(E, bool)                             # OVERFLOW and COMPLETE seen together
    for k in range(steps):
        if k == 3:                                       # arm in mid-episode, from the current state
            m = (rng.random(E) < 0.3) & ~never
            hist.arm(_u8(m))
            trk.arm(m, orc.snapshot())
        if k == 5:                                       # masked reset: arms what it resets
            host_reset((rng.random(E) < 0.3) & ~never)
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        _, _, g_done, _ = env.step(torch.from_numpy(a).cuda())
        done = orc.step(a)
        st = orc.snapshot()                              # (a terminal step: before any reset)
        g_done = g_done.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(g_done, done, err_msg=f"done step {k}")
        trk.step(st, done)
        ends += done
        both |= (trk.flags & (OVERFLOW | COMPLETE)) == 3
        if auto:
            orc.reset(done)                              # the auto-reset arms nothing
        elif done.any():
            trk.assert_equals(hist, f"finished, before the reset of step {k}")
            host_reset(done)                             # the caller's reset arms the envs it resets
        trk.assert_equals(hist, f"step {k}")
    assert (ends >= 2).all()
    h = _host(hist)
    assert (h["asset"][cap:] == SENTINEL).all() and (h["tag"][cap:] == TAG_SENTINEL).all()
    assert (h["stocks"][cap:] == SENTINEL).all()         # nothing at or past the capacity, in any env
    assert (h["length"] <= cap).all()
    assert (h["stocks"][1:cap] != 0).any() and len(np.unique(h["tag"][:cap][h["tag"][:cap] != TAG_SENTINEL])) >= 2
    if short:                                            # OVERFLOW, then COMPLETE (a host reset clears both)
        assert both.any()
    if auto:                                             # finished and not re-armed by the auto-reset
        assert ((trk.flags & COMPLETE) != 0)[~never].all()
        assert (h["length"][never] == 0).all() and (h["flags"][never] == 0).all()
        assert (h["asset"][:, never] == SENTINEL).all() and (h["start"][never] == SENTINEL).all()
        m = hist.metrics(2.0).cpu().numpy()
        assert np.isnan(m[never]).all() and not np.isnan(m[~never][:, :2]).any()


# ------------------------------------------------------------------------------------------
# 4. captured graph
# ------------------------------------------------------------------------------------------
def test_record_inside_a_captured_graph():
    """History enabled before the capture; step + redraw of the windows on done + arm(done) captured in
    one graph, the draws fed from the host: after every replay the record equals the tracker's, whose
    twins restart on the window that was pending when their env ended."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K, L, steps = 130, 40, 5, 2, 8, 26
    rng = np.random.default_rng(31)
    arrays = _panel(rng, T, N, K)
    length = rng.integers(3, L + 1, E)
    s0 = (rng.random(E) * (T - length + 1)).astype(np.int64)
    kw = dict(initial_capital=2e5)
    starts = _start_states(rng, E, N, 2e5)
    env = VecStockTradingEnvNP(_config(*arrays), E, windows=(s0, s0 + length), **kw)
    env.set_start_state(*starts)
    hist = env.enable_history(capacity=L)
    env.reset()
    orc = _Oracles(arrays, s0, s0 + length, starts, **kw)
    trk = _Tracker(E, N, L, L)
    trk.asset[:], trk.tag[:], trk.stocks[:] = 0.0, 0, 0.0           # (zero-initialised tensors here)
    trk.arm(np.ones(E, bool), orc.snapshot())
    pend = np.stack([s0, s0 + length])                   # what each env's next reset takes
    act = torch.zeros(E, N, device="cuda")
    ns = torch.zeros(E, dtype=torch.int32, device="cuda")
    nt = torch.zeros(E, dtype=torch.int32, device="cuda")

    def body():
        env.step(act)
        env.set_windows(ns, nt, mask=env.done)
        hist.arm(env.done)                               # the envs that were just auto-reset start a record

    def feed_and_follow(run, what):
        ln = rng.integers(3, L + 1, E)
        st = (rng.random(E) * (T - ln + 1)).astype(np.int64)
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        act.copy_(torch.from_numpy(a))
        ns.copy_(torch.from_numpy(st.astype(np.int32)))
        nt.copy_(torch.from_numpy((st + ln).astype(np.int32)))
        run()
        torch.cuda.synchronize()
        done = orc.step(a)
        np.testing.assert_array_equal(env.done.cpu().numpy().astype(bool), done, err_msg=what)
        trk.step(orc.snapshot(), done)
        for e in np.flatnonzero(done):                   # auto-reset onto the pending window, then the redraw
            orc.restart(e, int(pend[0, e]), int(pend[1, e]))
            pend[:, e] = st[e], st[e] + ln[e]
        trk.arm(done, orc.snapshot())
        trk.assert_equals(hist, what)
        return int(done.sum())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def warm():
        with torch.cuda.stream(side):
            body()                                      # warm-up step (eager, on the side stream)
        torch.cuda.current_stream().wait_stream(side)

    feed_and_follow(warm, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    nd, seen = 0, set()
    for k in range(steps):
        nd += feed_and_follow(graph.replay, f"replay {k}")
        seen.update(trk.length.tolist())
    assert nd >= 3 * E and len(seen) >= 4


# ------------------------------------------------------------------------------------------
# 5. detached; recording changes nothing the step returns
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [False, True], ids=["whole-panel", "windows"])
@pytest.mark.parametrize("E,N,K", [(300, 30, 8), (70, 3, 2)])
def test_outputs_and_state_equal_with_and_without_a_history_and_detach(E, N, K, win):
    _need_gpu()
    from finrl_amd._native import FinenvError
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    T = 12
    rng = np.random.default_rng(E + N + win)
    arrays = _panel(rng, T, N, K)
    windows = None
    if win:
        length = rng.integers(3, 10, E)
        s = (rng.random(E) * (T - length + 1)).astype(np.int64)
        windows = (s, s + length)
    starts = _start_states(rng, E, N, 1e5)
    envs = [VecStockTradingEnvNP(_config(*arrays), E, windows=windows, initial_capital=1e5) for _ in range(2)]
    for env in envs:
        env.enable_terminal_obs()
        env.set_start_state(*starts)
    assert torch.equal(envs[0].reset(), envs[1].reset())
    hist = envs[1].enable_history(capacity=4)            # (also through overflow)

    def same_step(k):
        a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
        p_out, h_out = envs[0].step(a), envs[1].step(a)
        for x, y, what in zip(p_out[:3], h_out[:3], ("obs", "reward", "done")):
            assert torch.equal(x, y), (what, k)
        for key in envs[0].state:
            assert torch.equal(envs[0].state[key], envs[1].state[key]), (key, k)
        if bool(p_out[2].any()):
            assert torch.equal(envs[0].term_obs, envs[1].term_obs)
        return bool(p_out[2].any())

    nd = 0
    for k in range(2 * T):
        nd += same_step(k)
        if k == T:
            m = _u8(rng.random(E) < 0.5)
            assert torch.equal(envs[0].reset(m), envs[1].reset(m))
    assert nd >= 2 and bool(hist.complete.any()) and bool(hist.overflow.any())
    # detached: nothing in the former tensors changes, the step is the plain one again
    for k in ("asset", "stocks", "start"):
        getattr(hist, k).fill_(SENTINEL)
    hist.tag.fill_(TAG_SENTINEL)
    hist.length.fill_(1)                                 # (armed, were it still attached)
    hist.flags.zero_()
    envs[1]._call("set_history", None)
    for k in range(T + 2):                               # episode ends, auto-resets and a host reset
        same_step(k)
        if k == 3:
            assert torch.equal(envs[0].reset(), envs[1].reset())
    torch.cuda.synchronize()
    for k in ("asset", "stocks", "start"):
        assert bool((getattr(hist, k) == SENTINEL).all()), k
    assert bool((hist.tag == TAG_SENTINEL).all())
    assert bool((hist.length == 1).all()) and not bool(hist.flags.any())
    with pytest.raises(FinenvError, match="no history attached"):
        hist.arm()


# ------------------------------------------------------------------------------------------
# 6. past 4 GiB
# ------------------------------------------------------------------------------------------
def test_stocks_slab_past_4_gib():
    """65,536 envs x 32 tickers x 516 entries: every entry of the holdings slab is 8 MiB, entry 512
    starts at byte 2^32.  A lock-step episode of 516 steps; the entries on both sides of the boundary
    against state["stocks"] read at those steps and, for a sample of envs, against twins; early entries
    are still what they were (a wrapped offset would land there); the rows past the capacity keep their
    pattern."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    from oracle.stocknp import StockNpOracle
    E, N, K, cap = 65_536, 32, 1, 514
    need = (cap + 2) * (N * 4 + 9) * E + (1 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of free device memory")
    T = cap + 2                                          # episodes of cap + 2 entries: they overflow
    rng = np.random.default_rng(9)
    price, tech, _ = _panel(rng, T, N, K)
    arrays = price, tech, np.zeros(T)                    # (no turbulence day: every entry holds stocks)
    env = VecStockTradingEnvNP(_config(*arrays), E, initial_capital=1e6)
    env.reset()
    hist = env.enable_history(capacity=cap + 2)
    assert hist.stocks.numel() * 4 > 2 ** 32 + 2 * E * N * 4
    assert 511 * N * E * 4 < 2 ** 32 == 512 * N * E * 4 < (cap - 1) * N * E * 4
    _shorten(env, hist, cap)
    _fill(hist)
    env.reset()
    sample = np.unique(np.concatenate([[0, 63, 64, 255, 256, E - 1], rng.integers(0, E, 10)]))
    twin = StockNpOracle(*arrays, n_envs=len(sample), initial_capital=1e6)
    twin.reset()
    pool = [rng.uniform(-1, 1, (E, N)).astype(np.float32) for _ in range(4)]
    dev_pool = [torch.from_numpy(a).cuda() for a in pool]
    watch = (1, 2, 300, 510, 511, 512, 513)
    snap, tsnap = {}, {}
    for k in range(1, cap + 2):                          # entry k is written by the k-th step
        _, _, done, _ = env.step(dev_pool[k % 4])
        t_done = twin.vec_step(pool[k % 4][sample], auto_reset=False)[2]
        if k in watch:
            snap[k] = (env.state["stocks"].clone(), env.state["total_asset"].clone())
            tsnap[k] = twin.state()
    assert bool(done.all()) and t_done.all()             # ... the last one terminal
    torch.cuda.synchronize()
    idx = torch.from_numpy(sample).cuda()
    for k, (stocks, asset) in snap.items():
        assert torch.equal(hist.stocks[k], stocks), k
        assert torch.equal(hist.asset[k], asset), k
        assert bool((stocks != 0).any())
        np.testing.assert_array_equal(hist.stocks[k].index_select(1, idx).cpu().numpy().T, tsnap[k]["stocks"])
        np.testing.assert_array_equal(hist.asset[k].index_select(0, idx).cpu().numpy(), tsnap[k]["total_asset"])
        np.testing.assert_array_equal(hist.tag[k].index_select(0, idx).cpu().numpy(), tsnap[k]["ta_tag"])
    assert bool((hist.length == cap).all()) and bool((hist.flags == (COMPLETE | OVERFLOW)).all())
    for k in (cap, cap + 1):
        assert bool((hist.stocks[k] == SENTINEL).all()) and bool((hist.asset[k] == SENTINEL).all())
        assert bool((hist.tag[k] == TAG_SENTINEL).all())
    assert bool((hist.stocks[0] == 0).all()) and bool((hist.start == 0).all())


# ------------------------------------------------------------------------------------------
# 7. metrics
# ------------------------------------------------------------------------------------------
def _pandas_metrics(asset, a):
    import pandas as pd
    v = pd.Series(asset)
    r = v.pct_change(1).dropna()
    mean, std = r.mean(), r.std()
    sharpe = a * mean / std if len(r) >= 2 and std != 0 else np.nan
    mdd = (v / v.cummax() - 1.0).min()
    return [len(r), v.iloc[-1] / v.iloc[0] - 1.0, mean, std, sharpe, mdd]


def test_metrics_against_pandas():
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K = 96, 40, 5, 2
    rng = np.random.default_rng(12)
    arrays = _panel(rng, T, N, K)
    length = rng.integers(3, T + 1, E)
    s = (rng.random(E) * (T - length + 1)).astype(np.int64)
    env = VecStockTradingEnvNP(_config(*arrays), E, auto_reset=True, windows=(s, s + length),
                               initial_capital=1e5)
    hist = env.enable_history()
    env.reset()
    hist.length[5] = 0                                   # one env never armed
    for k in range(int(length.max()) - 1):
        env.step(torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda())
    h = _host(hist)
    np.testing.assert_array_equal(np.delete(h["length"], 5), np.delete(length, 5))
    assert len(np.unique(h["length"])) > 10
    for a in (252 ** 0.5, 4 ** 0.5):
        m = hist.metrics(a).cpu().numpy()
        d = hist.metrics_dict(a)
        assert list(d) == list(hist.metric_keys) and torch.equal(d["sharpe"], hist.metrics(a)[:, 4])
        for e in range(E):
            if e == 5:
                assert np.isnan(m[e]).all()
                continue
            n = h["length"][e]
            want = _pandas_metrics(h["asset"][:n, e], a)
            assert m[e, 0] == n - 1 == want[0]
            np.testing.assert_allclose(m[e, 1:], want[1:], rtol=1e-9, atol=1e-12, err_msg=f"env {e}")


def test_metrics_of_a_constant_price_panel():
    """Constant prices of 16.0, no costs, whole-share trades: every product and sum is exact in float32
    and float64, the account value never moves although the envs trade -- std 0, Sharpe NaN."""
    _need_gpu()
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    E, T, N, K = 70, 20, 3, 2
    rng = np.random.default_rng(4)
    arrays = np.full((T, N), 16.0), rng.normal(0, 50, (T, N * K)), np.zeros(T)
    env = VecStockTradingEnvNP(_config(*arrays), E, buy_cost_pct=0.0, sell_cost_pct=0.0)
    hist = env.enable_history()
    env.reset()
    for k in range(T - 1):
        env.step(torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda())
    h = _host(hist)
    assert (h["length"] == T).all() and (h["flags"] == COMPLETE).all()
    assert (h["asset"] == 1e6).all() and (h["stocks"][1:] != 0).any()
    m = hist.metrics(252 ** 0.5).cpu().numpy()
    np.testing.assert_array_equal(m[:, 0], T - 1)
    np.testing.assert_array_equal(m[:, [1, 2, 3, 5]], 0.0)
    assert np.isnan(m[:, 4]).all()
