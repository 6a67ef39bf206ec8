"""Episode history of the batched crypto env (VecCryptoEnv.enable_history(), finenv_crypto_set_history)
on the MI355X: the record written by the step kernel against the reference fixtures, against a host
tracker that restates the header's recording rule and is fed by one CPU oracle per env, inside a
captured graph, past 4 GiB, detached, and its metrics.  The recorded values are the step's own, so every
comparison with this build's step and with oracle.crypto.CryptoOracle is exact (tolerance 0)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("n1", "n9_poor", "pairs10", "lookback3")
COMPLETE, OVERFLOW = 1, 2
SENTINEL = -7
TENSORS = ("asset", "holdings", "stocks", "start", "length", "flags")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(rng, T, N, W, decades=2.0):
    drift = np.linspace(0.0, decades, T)[:, None] * rng.choice([-1.0, 1.0], N)
    price = 10.0 ** (rng.uniform(0.0, 3.0, N) + drift) * np.exp(
        np.cumsum(rng.normal(0, 0.004, (T, N)), axis=0))
    return price, rng.normal(0, 3000, (T, W))


def _row_sums(stocks, price_rows):
    """np.sum(stocks[e] * price[time_e]) of every env (:82): the reduction along the contiguous axis is
    the 1-D pairwise sum of each row (checked on a few rows against the 1-D call itself)."""
    prod = np.ascontiguousarray(stocks * price_rows)
    out = prod.sum(axis=1)
    for e in range(0, len(prod), max(1, len(prod) // 16)):
        assert out[e] == prod[e].sum()
    return out


def _host(hist):
    return {k: getattr(hist, k).cpu().numpy() if getattr(hist, k) is not None else None for k in TENSORS}


def _fill(hist, cap_rows=None):
    """Sentinel in every tensor, nobody armed."""
    for k in ("asset", "holdings", "stocks", "start"):
        if getattr(hist, k) is not None:
            getattr(hist, k).fill_(SENTINEL)
    hist.length.zero_()
    hist.flags.zero_()


# ------------------------------------------------------------------------------------------
# 1., 2., 9. the reference fixtures
# ------------------------------------------------------------------------------------------
def _fixture_episodes(z):
    """Per finished episode of the fixture: the record it must leave (asset, holdings, stocks), entry 0
    the armed one."""
    T, N, W, S, L = z["cfg_int"].tolist()
    cap0 = z["cfg_float"][0]
    marks = z["reset_step"].tolist()
    out = []
    for a, b in zip(marks[:-1], marks[1:]):
        steps = range(a + 1, b + 1)
        asset = np.array([cap0] + [z["total_asset"][s] for s in steps])
        hold = np.array([0.0] + [(z["stocks"][s] * z["price"][z["time"][s]]).sum() for s in steps])
        stocks = np.concatenate([np.zeros((1, N), np.float32), z["stocks"][a + 1:b + 1]])
        out.append(dict(last=b, asset=asset, holdings=hold, stocks=stocks, n=len(asset)))
    return out


def _assert_fixture_record(hist, ep, E, L, tag):
    h = _host(hist)
    n = ep["n"]
    np.testing.assert_array_equal(h["length"], n, err_msg=tag)
    np.testing.assert_array_equal(h["flags"], COMPLETE, err_msg=tag)
    np.testing.assert_array_equal(h["start"], L - 1, err_msg=tag)
    np.testing.assert_array_equal(h["asset"][:n], np.broadcast_to(ep["asset"][:, None], (n, E)), err_msg=tag)
    np.testing.assert_array_equal(h["holdings"][:n], np.broadcast_to(ep["holdings"][:, None], (n, E)),
                                  err_msg=tag)
    np.testing.assert_array_equal(h["stocks"][:n], np.broadcast_to(ep["stocks"][:, :, None],
                                                                  ep["stocks"].shape + (E,)), err_msg=tag)


def _fixture_env(name, auto, E=300):
    from finrl_amd.vec_crypto import VecCryptoEnv
    z = np.load(os.path.join(GOLDEN, f"crypto_{name}.npz"), allow_pickle=False)
    T, N, W, S, L = z["cfg_int"].tolist()
    cap, bc, sc, g = z["cfg_float"].tolist()
    env = VecCryptoEnv({"price_array": z["price"], "tech_array": z["tech"]}, E, lookback=L,
                       initial_capital=cap, buy_cost_pct=bc, sell_cost_pct=sc, gamma=g, auto_reset=auto)
    return z, env


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_episodes_are_recorded(name):
    """E = 300 (four full waves and a 44-lane tail), auto_reset=False, host reset() between episodes: the
    record of each episode equals the fixture's total_asset, np.sum(stocks * price[time]) and stocks."""
    _need_gpu()
    z, env = _fixture_env(name, False)
    T, N, W, S, L = z["cfg_int"].tolist()
    E = env.num_envs
    hist = env.enable_history()
    assert env.enable_history(capacity=3) is hist is env.history
    assert hist.capacity == T - 2 * L + 1 == env.max_step - L + 2
    assert hist.nbytes == E * (16 * hist.capacity + 12) + 4 * E * N * hist.capacity
    assert tuple(hist.stocks.shape) == (hist.capacity, N, E)
    eps = {ep["last"]: ep for ep in _fixture_episodes(z)}
    env.reset()
    since = 0
    for k in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][k], (E, N)).copy()).cuda()
        env.step(a)
        since += 1
        if k in eps:
            assert bool(hist.complete.all()) and not bool(hist.overflow.any())
            _assert_fixture_record(hist, eps[k], E, L, f"{name} episode ending at step {k}")
            env.reset()
            since = 0
    assert len(eps) == 2
    # the unfinished third episode: armed by the reset, one entry per step, not complete
    h = _host(hist)
    np.testing.assert_array_equal(h["length"], since + 1)
    np.testing.assert_array_equal(h["flags"], 0)
    np.testing.assert_array_equal(h["asset"][since], z["total_asset"][S - 1])


@pytest.mark.parametrize("name", FIXTURES)
def test_auto_reset_leaves_the_record_alone(name):
    """auto_reset=True: the terminal step is recorded from the values before the reset, the state is
    reset in the same launch, and the record stays as it is through the next episode's steps; arm() at
    the fresh state then records the second episode, equal to the host-reset run's."""
    _need_gpu()
    z, env = _fixture_env(name, True)
    T, N, W, S, L = z["cfg_int"].tolist()
    E, cap0 = env.num_envs, z["cfg_float"][0]
    hist = env.enable_history()
    eps = _fixture_episodes(z)
    env.reset()
    for k in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][k], (E, N)).copy()).cuda()
        env.step(a)
        if k == eps[0]["last"]:
            _assert_fixture_record(hist, eps[0], E, L, f"{name} first episode")
            st = env.state_numpy()
            assert (st["total_asset"] == cap0).all() and not st["stocks"].any()      # ... and was reset
            assert (st["time"] == L - 1).all()
        if k == eps[0]["last"] + 3:                     # three steps into the next episode: untouched
            _assert_fixture_record(hist, eps[0], E, L, f"{name} first episode, later")
        if k == eps[1]["last"]:
            _assert_fixture_record(hist, eps[0], E, L, f"{name} first episode at the second end")
            hist.arm()                                  # (the auto-reset has put every env at its start)
            np.testing.assert_array_equal(hist.length.cpu().numpy(), 1)
    # the second episode again from a fresh arm: replay its actions
    z2, env2 = _fixture_env(name, True)
    hist2 = env2.enable_history()
    env2.reset()
    for k in range(eps[1]["last"] + 1):
        if k == eps[0]["last"] + 1:
            hist2.arm()
        env2.step(torch.from_numpy(np.broadcast_to(z["actions"][k], (E, N)).copy()).cuda())
    _assert_fixture_record(hist2, eps[1], E, L, f"{name} second episode")


@pytest.mark.parametrize("name", FIXTURES)
def test_readers_on_the_device_path(name):
    _need_gpu()
    z, env = _fixture_env(name, True)
    T, N, W, S, L = z["cfg_int"].tolist()
    E, cap0 = env.num_envs, float(z["cfg_float"][0])
    hist = env.enable_history()
    ep = _fixture_episodes(z)[0]
    env.reset()
    for k in range(ep["last"] + 1):
        env.step(torch.from_numpy(np.broadcast_to(z["actions"][k], (E, N)).copy()).cuda())
    envs = [0, 63, 64, 257, E - 1]
    want = [cap0]
    for s in range(ep["last"] + 1):                     # models.py:146-156 on the recorded state
        want.append(cap0 + (z["price"][z["time"][s]] * z["stocks"][s]).sum())
    want = [float(x) for x in want]
    got = hist.episode_total_assets(envs)
    assert len(got) == len(envs) and all(g == want and type(g[1]) is float for g in got)
    assert hist.episode_total_assets(E - 1) == want
    assert hist.episode_total_assets(5, 10.0)[1] == 10.0 + ep["holdings"][1]
    for av in hist.account_values(envs):
        np.testing.assert_array_equal(av, ep["asset"])
    np.testing.assert_array_equal(hist.account_values(64), ep["asset"])
    for pos in hist.positions(envs):
        np.testing.assert_array_equal(pos, ep["stocks"])
    for rows in hist.rows(envs):
        np.testing.assert_array_equal(rows, L - 1 + np.arange(ep["n"]))
    no_stocks = _fixture_env(name, True, E=64)[1]
    h2 = no_stocks.enable_history(stocks=False)
    assert h2.stocks is None and h2.nbytes == 64 * (16 * h2.capacity + 12)
    no_stocks.reset()
    for k in range(ep["last"] + 1):
        no_stocks.step(torch.from_numpy(np.broadcast_to(z["actions"][k], (64, N)).copy()).cuda())
    assert h2.episode_total_assets(7) == want
    from finrl_amd._native import FinenvError
    with pytest.raises(FinenvError):
        h2.positions(0)


# ------------------------------------------------------------------------------------------
# 3., 4. the recording rule against a host tracker fed by one oracle per env
# ------------------------------------------------------------------------------------------
class _Oracles:
    """One CryptoOracle(price[s:t], tech[s:t], n_envs=1) per env of `idx`, stepped WITHOUT auto-reset so
    that the values of a terminal step can be read before reset() (which is what an auto-reset is)."""

    def __init__(self, price, tech, s, t, idx, **kw):
        from oracle.crypto import CryptoOracle
        self.price, self.idx = price, np.asarray(idx)
        self.s = np.asarray(s, dtype=np.int64)[self.idx]
        self.orc = [CryptoOracle(price[a:b], tech[a:b], n_envs=1, **kw)
                    for a, b in zip(self.s, np.asarray(t, dtype=np.int64)[self.idx])]
        for o in self.orc:
            o.reset()

    def reset(self, mask):
        for o, e in zip(self.orc, self.idx):
            if mask[e]:
                o.reset()

    def step(self, actions):
        return np.array([o.vec_step(actions[e:e + 1], auto_reset=False)[2][0]
                         for o, e in zip(self.orc, self.idx)])

    def snapshot(self):
        sts = [o.state() for o in self.orc]
        st = {k: np.concatenate([x[k] for x in sts]) for k in ("total_asset", "stocks", "time")}
        st["time"] = st["time"] + self.s                                  # the panel row
        st["holdings"] = _row_sums(st["stocks"], self.price[st["time"]])
        return st


class _Tracker:
    """The recording rule of include/finenv.h, restated on the host for the envs of `idx`."""

    def __init__(self, n, N, cap, rows):
        self.cap = cap
        self.asset = np.full((rows, n), float(SENTINEL))
        self.holdings = np.full((rows, n), float(SENTINEL))
        self.stocks = np.full((rows, N, n), SENTINEL, np.float32)
        self.start = np.full(n, SENTINEL, np.int32)
        self.length = np.zeros(n, np.int32)
        self.flags = np.zeros(n, np.int32)

    def arm(self, mask, st):
        j = np.flatnonzero(mask)
        self.asset[0, j], self.holdings[0, j] = st["total_asset"][j], st["holdings"][j]
        self.stocks[0][:, j] = st["stocks"][j].T
        self.start[j], self.length[j], self.flags[j] = st["time"][j], 1, 0

    def step(self, st, done):
        live = (self.length >= 1) & ((self.flags & COMPLETE) == 0)
        room = live & (self.length < self.cap)
        j = np.flatnonzero(room)
        k = self.length[j]
        self.asset[k, j], self.holdings[k, j] = st["total_asset"][j], st["holdings"][j]
        self.stocks[k, :, j] = st["stocks"][j]
        self.length[j] = k + 1
        self.flags[live & ~room] |= OVERFLOW
        self.flags[live & done] |= COMPLETE

    def assert_equals(self, hist, idx, tag):
        h = _host(hist)
        for k in TENSORS:
            np.testing.assert_array_equal(h[k][..., idx], getattr(self, k), err_msg=f"{k} {tag}")


def _shorten(env, hist, cap):
    """Tell the kernel a capacity shorter than the tensors: the rows past it must keep their sentinel."""
    hist._ptrs.capacity = cap
    env._call("set_history", C.byref(hist._ptrs))


RULE_CASES = [
    # E, T, N, W, L, windows, auto, record, short capacity
    dict(E=200, T=40, N=10, W=40, L=1, win=True, auto=True),        # trader + streamer, column split
    dict(E=200, T=40, N=10, W=40, L=1, win=True, auto=False),
    dict(E=200, T=30, N=10, W=40, L=1, win=False, auto=True, record=True),   # step(..., record=...)
    dict(E=136, T=40, N=10, W=40, L=1, win=True, auto=True, record=True, short=True),
    dict(E=130, T=40, N=1, W=0, L=1, win=True, auto=True),          # one asset, no indicators
    dict(E=70, T=24, N=4, W=7, L=3, win=False, auto=False),         # 8-wide build, no windows
    dict(E=70, T=24, N=4, W=7, L=3, win=False, auto=True, short=True),
    dict(E=136, T=50, N=9, W=5, L=2, win=True, auto=True),          # 12-wide build
    dict(E=128, T=24, N=16, W=47, L=1, win=False, auto=True),       # 16-wide build, D = 64: block form
    dict(E=128, T=40, N=16, W=47, L=1, win=True, auto=False, short=True),
    dict(E=68, T=40, N=20, W=1, L=2, win=True, auto=True),          # 32-wide build
    dict(E=68, T=24, N=20, W=1, L=2, win=False, auto=False),
    dict(E=140_005, T=40, N=10, W=40, L=1, win=True, auto=True),    # four-wave form, 37-lane tail
    dict(E=140_005, T=16, N=10, W=40, L=1, win=False, auto=True, short=True),
    dict(E=131_200, T=16, N=4, W=7, L=1, win=False, auto=True, record=True),
]


def _case_id(c):
    return "E{E}-N{N}-L{L}".format(**c) + "".join(
        f"-{k}" for k in ("win", "auto", "record", "short") if c.get(k))


@pytest.mark.parametrize("cfg", RULE_CASES, ids=_case_id)
def test_recording_rule_against_a_host_tracker(cfg):
    _need_gpu()
    from finrl_amd.rollout import RolloutBuffer
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = cfg["E"], cfg["T"], cfg["N"], cfg["W"], cfg["L"]
    win, auto, record, short = cfg["win"], cfg["auto"], cfg.get("record", False), cfg.get("short", False)
    rng = np.random.default_rng(E + 7 * N + L + auto)
    price, tech = _panel(rng, T, N, W)
    if win:                                              # random windows of mixed lengths
        length = rng.integers(2 * L + 4, 2 * L + 13, E)
        s = (rng.random(E) * (T - length + 1)).astype(np.int64)
        t = s + length
    else:
        s, t = np.zeros(E, np.int64), np.full(E, T, np.int64)
    kw = dict(lookback=L, initial_capital=3e4, buy_cost_pct=0.0012, sell_cost_pct=0.0008, gamma=0.98)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, auto_reset=auto,
                       windows=(s, t) if win else None, **kw)
    longest = int((t - s).max()) - 2 * L + 1             # entries of the longest episode
    assert env.max_step - L + 2 == longest
    rows = longest + 2
    hist = env.enable_history(capacity=rows)
    cap = 4 if short else longest
    _shorten(env, hist, cap)
    _fill(hist)
    big = E > 4096
    idx = np.unique(np.concatenate([np.arange(64), np.arange(E - 101, E), rng.integers(0, E, 90)])) \
        if big else np.arange(E)
    orc = _Oracles(price, tech, s, t, idx, **kw)
    trk = _Tracker(len(idx), N, cap, rows)
    # never armed: only where nothing on the host has to reset them (auto-reset keeps them running)
    never = (rng.random(E) < 0.1) if auto else np.zeros(E, bool)
    never[idx[1]] = auto

    def u8(mask):
        return torch.from_numpy(mask.astype(np.uint8)).cuda()

    first = ~never
    env.reset(u8(first))                                 # (every env is at its start already) arms them
    trk.arm(first[idx], orc.snapshot())
    trk.assert_equals(hist, idx, "after the first reset")
    steps = 2 * longest + 3
    buf = RolloutBuffer(steps, E, env.obs_dim, N) if record else None
    ends = np.zeros(len(idx), int)
    both = np.zeros(len(idx), bool)                      # OVERFLOW and COMPLETE seen together
    for k in range(steps):
        if k == 3:                                       # arm in mid-episode, from the current state
            m = (rng.random(E) < 0.3) & ~never
            hist.arm(u8(m))
            st = orc.snapshot()
            trk.arm(m[idx], st)
            h = _host(hist)
            j = np.flatnonzero(m[idx])
            np.testing.assert_array_equal(h["asset"][0, idx[j]], st["total_asset"][j])
            np.testing.assert_array_equal(h["holdings"][0, idx[j]], st["holdings"][j])
            assert (st["holdings"][j] != 0).any()
        if k == 5:                                       # masked reset: arms what it resets
            m = (rng.random(E) < 0.3) & ~never
            env.reset(u8(m))
            orc.reset(m)
            trk.arm(m[idx], orc.snapshot())
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        at = torch.from_numpy(a).cuda()
        if record:
            v, lp = torch.randn(E, device="cuda"), torch.randn(E, device="cuda")
            buf.step(env, k, at, v, lp)
            g_rew, g_done = buf.rewards[k], buf.dones[k]
            assert torch.equal(buf.actions[k], at) and torch.equal(buf.values[k], v)
            assert torch.equal(buf.log_probs[k], lp)
        else:
            _, g_rew, g_done, _ = env.step(at)
        done = orc.step(a)
        st = orc.snapshot()                              # (a terminal step: before any reset)
        g_done = g_done.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(g_done[idx], done, err_msg=f"done step {k}")
        trk.step(st, done)
        ends += done
        both |= (trk.flags & (OVERFLOW | COMPLETE)) == 3
        if not auto and done.any():                      # the finished record, before the reset re-arms it
            np.testing.assert_array_equal(hist.flags.cpu().numpy()[idx], trk.flags, err_msg=f"flags {k}")
            np.testing.assert_array_equal(hist.length.cpu().numpy()[idx], trk.length, err_msg=f"len {k}")
        full = np.zeros(E, bool)
        full[idx] = done
        if auto:
            orc.reset(full)                              # the auto-reset arms nothing
        elif g_done.any():
            env.reset(u8(g_done))                        # the caller's reset arms the envs it resets
            orc.reset(full)
            trk.arm(done, orc.snapshot())
        if not big or k % 5 == 0 or k == steps - 1:
            trk.assert_equals(hist, idx, f"step {k}")
    assert (ends >= 2).all()
    h = _host(hist)
    assert (h["asset"][cap:] == SENTINEL).all() and (h["holdings"][cap:] == SENTINEL).all()
    assert (h["stocks"][cap:] == SENTINEL).all()         # nothing at or past the capacity, in any env
    assert (h["length"] <= cap).all()
    if short:                                            # OVERFLOW, then COMPLETE (a host reset clears both)
        assert (trk.flags & OVERFLOW).any() and both.any()
    if auto:                                             # finished and not re-armed by the auto-reset
        assert not short or ((trk.flags & (OVERFLOW | COMPLETE)) == 3).any()
        assert ((trk.flags & COMPLETE) != 0)[~never[idx]].all()
        assert (h["length"][never] == 0).all() and (h["flags"][never] == 0).all()
        assert (h["asset"][:, never] == SENTINEL).all() and (h["start"][never] == SENTINEL).all()
        m = hist.metrics(2.0).cpu().numpy()
        assert np.isnan(m[never]).all() and not np.isnan(m[~never][:, :2]).any()


# ------------------------------------------------------------------------------------------
# 5. captured graph
# ------------------------------------------------------------------------------------------
def test_record_inside_a_captured_graph():
    """History enabled before the capture; step + window redraw on done + arm(done) captured in one
    graph: after every replay the record equals that of an eager env fed the same draws."""
    _need_gpu()
    from finrl_amd.data import random_windows
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L, LEN, steps = 256, 90, 10, 40, 1, 8, 30
    rng = np.random.default_rng(31)
    price, tech = _panel(rng, T, N, W)
    gen = torch.Generator(device="cuda").manual_seed(5)
    s0, t0 = random_windows(T, E, torch.randint(3, LEN + 1, (E,)), generator=gen)
    s0n, t0n = s0.cpu().numpy().astype(np.int64), t0.cpu().numpy().astype(np.int64)

    def make():
        env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, windows=(s0n, t0n))
        env.enable_history(capacity=LEN)
        env.reset()
        return env

    env, eager = make(), make()
    a_in = torch.zeros(E, N, device="cuda")
    drawn = torch.zeros(2, E, dtype=torch.int32, device="cuda")

    def body():
        obs, rew, done, _ = env.step(a_in)
        ns, nt = random_windows(T, E, LEN, device="cuda")
        env.set_windows(ns, nt, mask=done)
        env.history.arm(done)                           # the envs that were just auto-reset start a record
        drawn[0].copy_(ns)
        drawn[1].copy_(nt)

    def follow(a, tag):
        _, _, e_done, _ = eager.step(torch.from_numpy(a).cuda())
        eager.set_windows(drawn[0], drawn[1], mask=e_done)
        eager.history.arm(e_done)
        torch.cuda.synchronize()
        for k in TENSORS:
            assert torch.equal(getattr(env.history, k), getattr(eager.history, k)), (k, tag)
        for key in env.state:
            assert torch.equal(env.state[key], eager.state[key]), (key, tag)
        return int(e_done.sum())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                          # warm-up step (eager, on the side stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    follow(np.zeros((E, N), np.float32), "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    acts = rng.uniform(-1, 1, (steps, E, N)).astype(np.float32)
    nd, seen = 0, set()
    for k in range(steps):
        a_in.copy_(torch.from_numpy(acts[k]))
        graph.replay()
        torch.cuda.synchronize()
        nd += follow(acts[k], f"replay {k}")
        seen.update(env.history.length.cpu().numpy().tolist())
    assert nd >= 2 * E and len(seen) >= 4 and bool((env.history.holdings != 0).any())


# ------------------------------------------------------------------------------------------
# 6. detach
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [200, 140_005])
def test_detached_history_is_not_written(E):
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    T, N, W = 14, 10, 40
    rng = np.random.default_rng(3)
    price, tech = _panel(rng, T, N, W)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E)
    hist = env.enable_history()
    env.reset()
    a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
    env.step(a)
    assert int(hist.length.min()) == 2
    for k in ("asset", "holdings", "stocks", "start", "length", "flags"):
        getattr(hist, k).fill_(SENTINEL if k != "length" else 1)       # (armed, were it still attached)
    hist.flags.zero_()
    env._call("set_history", None)
    for k in range(2 * T):                               # episode ends, auto-resets and a host reset
        env.step(a)
        if k == T:
            env.reset()
    torch.cuda.synchronize()
    for k in ("asset", "holdings", "stocks", "start"):
        assert bool((getattr(hist, k) == SENTINEL).all()), k
    assert bool((hist.length == 1).all()) and not bool(hist.flags.any())
    from finrl_amd._native import FinenvError
    with pytest.raises(FinenvError, match="no history attached"):
        hist.arm()


# ------------------------------------------------------------------------------------------
# 7. past 4 GiB
# ------------------------------------------------------------------------------------------
def test_stocks_slab_past_4_gib():
    """262,144 envs x 10 pairs x 420 entries: the holdings slab is 4.4 GB, entry 409 straddles byte
    2^32.  Entries on both sides of it against state["stocks"] read at those steps; early entries are
    still what they were (a wrapped offset would land there); the rows past the capacity keep their
    sentinel."""
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, N, W, cap = 262_144, 10, 2, 420
    T = cap + 3                                          # episodes of cap + 2 entries: they overflow
    rng = np.random.default_rng(9)
    price, tech = _panel(rng, T, N, W, decades=0.5)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E)
    hist = env.enable_history(capacity=cap + 2)
    assert hist.stocks.numel() * 4 > 2 ** 32 + 2 * E * N * 4
    _shorten(env, hist, cap)
    _fill(hist)
    env.reset()
    pool = [torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda() for _ in range(4)]
    watch = (1, 2, 200, 405, 408, 409, 410, 411, 415, 419)
    assert 409 * N * E * 4 < 2 ** 32 < 410 * N * E * 4
    snap = {}
    for k in range(1, cap + 2):                          # entry k is written by the k-th step
        _, _, done, _ = env.step(pool[k % 4])
        if k in watch:
            snap[k] = (env.state["stocks"].clone(), env.state["total_asset"].clone())
    assert bool(done.all())                              # ... the last one terminal
    torch.cuda.synchronize()
    for k, (stocks, asset) in snap.items():
        assert torch.equal(hist.stocks[k], stocks), k
        assert torch.equal(hist.asset[k], asset), k
        assert bool((stocks != 0).any())
    assert bool((hist.length == cap).all()) and bool((hist.flags == (COMPLETE | OVERFLOW)).all())
    for k in (cap, cap + 1):
        assert bool((hist.stocks[k] == SENTINEL).all()) and bool((hist.asset[k] == SENTINEL).all())
        assert bool((hist.holdings[k] == SENTINEL).all())
    assert bool((hist.stocks[0] == 0).all()) and bool((hist.start == 0).all())


# ------------------------------------------------------------------------------------------
# 8. metrics
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
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = 96, 60, 4, 3, 2
    rng = np.random.default_rng(12)
    price, tech = _panel(rng, T, N, W, decades=0.3)
    length = rng.integers(2 * L + 3, T, E)
    s = (rng.random(E) * (T - length + 1)).astype(np.int64)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, lookback=L, auto_reset=True,
                       windows=(s, s + length))
    hist = env.enable_history()
    env.reset()
    hist.length[5] = 0                                   # one env never armed
    for k in range(int(length.max()) - 2 * L + 2):
        env.step(torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda())
    h = _host(hist)
    np.testing.assert_array_equal(np.delete(h["length"], 5), np.delete(length - 2 * L + 1, 5))
    assert len(np.unique(h["length"])) > 10
    for a in (252 ** 0.5, (365 * 1440) ** 0.5):
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
    """Constant prices of 16.0, no costs, actions that are multiples of 2^-10 (trades of multiples of
    1000 / 1024 units): every product and sum is exact, the account value never moves although the envs
    trade -- std 0, Sharpe NaN."""
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W = 70, 20, 3, 2
    rng = np.random.default_rng(4)
    price, tech = np.full((T, N), 16.0), rng.normal(0, 3000, (T, W))
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, buy_cost_pct=0.0, sell_cost_pct=0.0)
    hist = env.enable_history()
    env.reset()
    for k in range(T - 2):
        a = rng.integers(-1024, 1025, (E, N)).astype(np.float32) / 1024
        env.step(torch.from_numpy(a).cuda())
    h = _host(hist)
    assert (h["length"] == T - 1).all() and (h["flags"] == COMPLETE).all()
    assert (h["asset"] == 1e6).all() and (h["holdings"][1:] != 0).any() and (h["stocks"][1:] != 0).any()
    m = hist.metrics(252 ** 0.5).cpu().numpy()
    np.testing.assert_array_equal(m[:, 0], T - 2)
    np.testing.assert_array_equal(m[:, [1, 2, 3, 5]], 0.0)
    assert np.isnan(m[:, 4]).all()


# ------------------------------------------------------------------------------------------
# 10. recording changes nothing the step returns
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(E=300, T=20, N=10, W=40, L=1, win=False),
                                 dict(E=200, T=40, N=10, W=40, L=2, win=True),
                                 dict(E=70, T=20, N=20, W=3, L=1, win=True),
                                 dict(E=140_005, T=14, N=10, W=40, L=1, win=False)],
                         ids=lambda c: "E{E}-N{N}-L{L}".format(**c))
def test_outputs_and_state_equal_with_and_without_a_history(cfg):
    _need_gpu()
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, L = cfg["E"], cfg["T"], cfg["N"], cfg["W"], cfg["L"]
    rng = np.random.default_rng(E + N)
    price, tech = _panel(rng, T, N, W)
    windows = None
    if cfg["win"]:
        length = rng.integers(2 * L + 2, 2 * L + 9, E)
        s = (rng.random(E) * (T - length + 1)).astype(np.int64)
        windows = (s, s + length)
    envs = [VecCryptoEnv({"price_array": price, "tech_array": tech}, E, lookback=L, windows=windows)
            for _ in range(2)]
    for env in envs:
        env.enable_terminal_obs()
    hist = envs[1].enable_history(capacity=4)            # (also through overflow)
    assert torch.equal(envs[0].reset(), envs[1].reset())
    nd = 0
    for k in range(2 * T):
        a = torch.from_numpy(rng.uniform(-1, 1, (E, N)).astype(np.float32)).cuda()
        p_out, h_out = envs[0].step(a), envs[1].step(a)
        for x, y, what in zip(p_out[:3], h_out[:3], ("obs", "reward", "done")):
            assert torch.equal(x, y), (what, k)
        for key in envs[0].state:
            assert torch.equal(envs[0].state[key], envs[1].state[key]), (key, k)
        if bool(p_out[2].any()):
            nd += 1
            assert torch.equal(envs[0].term_obs, envs[1].term_obs)
        if k == T:
            m = torch.from_numpy((rng.random(E) < 0.5).astype(np.uint8)).cuda()
            assert torch.equal(envs[0].reset(m), envs[1].reset(m))
    assert nd >= 2 and bool(hist.complete.any())
