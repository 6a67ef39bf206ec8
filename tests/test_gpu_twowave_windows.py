"""Per-env episode windows of the HIP cash-penalty and stop-loss envs (finenv_<kind>_set_windows):
env e on window [s_e, t_e) of one shared panel equals the reference env built on the frame restricted
to dates[s_e:t_e] -- against the reference fixtures laid into a NaN-padded panel (money rel 1e-12,
market-data columns exact) and, bit for bit, against one CPU oracle per env on its slice
(tests/twowave_windows_cases.py; tests/test_twowave_windows_scenarios.py shows what those scenarios
reach)."""
import glob
import os

import numpy as np
import pytest

from twowave_windows_cases import (COMMON, KINDS, SCENARIOS, SCENARIO_IDS, T_ROWS, Script, Twins,
                                   classes, draw_windows, env_kwargs, make_panel, nan_padded, state_keys)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = [(kind, os.path.basename(p)[len(kind) + 1:-4]) for kind in KINDS
            for p in sorted(glob.glob(os.path.join(GOLDEN, f"{kind}_*.npz")))]
SL_VEC = ("holdings", "avg_buy_price", "n_buys", "closing_diff_avg_buy", "profit_sell_diff_avg_buy")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _fixture_kw(kind, z):
    T, N, Cc, S, disc, inc, use_t, patient = z["cfg_int"].tolist()
    f = z["cfg_float"].tolist()
    kw = dict(buy_cost_pct=f[1], sell_cost_pct=f[2], hmax=f[0], discrete_actions=bool(disc),
              shares_increment=inc, turbulence_threshold=f[5] if use_t else None,
              initial_amount=f[3], cash_penalty_proportion=f[4], patient=bool(patient))
    if kind == "stoploss":
        kw.update(stoploss_penalty=f[6], profit_loss_ratio=f[7])
    return kw


def _no_nan(env, *tensors):
    for t in tensors:
        assert not torch.isnan(t).any()
    for k, v in env.state.items():
        assert not torch.isnan(v.to(torch.float64)).any(), k


# ------------------------------------------------------------------------------------------
# 1. reference fixtures as windows of a NaN-padded panel
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", FIXTURES, ids=[f"{k}-{n}" for k, n in FIXTURES])
def test_reference_fixture_as_windows_of_a_nan_padded_panel(kind, name):
    _need_gpu()
    Panel, Env, _ = classes(kind)
    z = np.load(os.path.join(GOLDEN, f"{kind}_{name}.npz"), allow_pickle=False)
    T, N, Cc, S = z["cfg_int"].tolist()[:4]
    E = 70
    block = (z["close"], z["info"], z["turb"])
    close, info, turb, offs = nan_padded([block, block], 3, N, Cc)
    w0 = np.where(np.arange(E) % 2 == 0, offs[0], offs[1])
    env = Env(Panel(close, info, turb), E, random_start=False, auto_reset=False,
              windows=(w0, w0 + T), **_fixture_kw(kind, z))
    ri = 0
    env.set_next_start(int(z["reset_start"][ri]))           # offsets from each window's first row
    obs = env.reset()
    _no_nan(env, obs)
    np.testing.assert_allclose(obs.cpu().numpy()[:2], np.broadcast_to(
        z["reset_obs"][ri].astype(np.float32), (2, obs.shape[1])), rtol=1e-6)
    ri += 1
    nd = 0
    for s in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][s], (E, N)).copy()).cuda()
        obs, rew, done, _ = env.step(a)
        _no_nan(env, obs, rew)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        st = env.state_numpy()
        np.testing.assert_array_equal(env.window_day().cpu().numpy(), st["date_index"] - w0)
        for e in (0, 1, 63, 64, E - 1):
            assert bool(done[e]) == bool(z["done"][s]), (s, e)
            assert st["date_index"][e] - w0[e] == z["date_index"][s], (s, e)
            assert st["start"][e] - w0[e] == z["reset_start"][ri - 1], (s, e)
            for k in (SL_VEC if kind == "stoploss" else ("holdings",)):
                np.testing.assert_allclose(st[k][e], z[k][s], rtol=1e-12, atol=1e-12,
                                           err_msg=f"{k} step {s} env {e}")
            assert st["coh"][e] == pytest.approx(z["coh"][s], rel=1e-12)
            assert rew[e] == pytest.approx(z["reward"][s], rel=1e-6, abs=1e-12)
            np.testing.assert_array_equal(obs[e][1 + N:], z["obs"][s][1 + N:].astype(np.float32))
            np.testing.assert_allclose(obs[e][:1 + N], z["obs"][s][:1 + N].astype(np.float32),
                                       rtol=1e-6, atol=1e-6)
            if kind == "stoploss" and not done[e]:
                assert st["actual_num_trades"][e] == z["actual_num_trades"][s]
        if z["done"][s]:
            nd += 1
            env.set_next_start(int(z["reset_start"][ri]))
            env.reset()
            ri += 1
    assert nd >= 2


# ------------------------------------------------------------------------------------------
# 2. random windows against one oracle per env on its slice
# ------------------------------------------------------------------------------------------
def _make(kind, sc, script, close, info, turb, **kw):
    Panel, Env, _ = classes(kind)
    env = Env(Panel(close, info, turb), sc["E"], random_start=False, auto_reset=sc["auto"],
              windows=(script.start, script.end), **env_kwargs(sc), **kw)
    env.enable_terminal_obs()
    return env, Twins(kind, sc, close, info, turb, script.start, script.end)


def _assert_state(kind, sc, env, tw, tag):
    st, os_ = env.state_numpy(), tw.state()
    for k in state_keys(kind):
        if k == "turbulence" and sc["thr"] is None:
            continue
        np.testing.assert_array_equal(st[k], os_[k], err_msg=f"{k} {tag}")
    # rows 2, 3 are what the twins are running; rows 0, 1 what the caller wrote
    np.testing.assert_array_equal(env.active_windows.cpu().numpy(), tw.active, err_msg=f"active {tag}")
    np.testing.assert_array_equal(env.windows.cpu().numpy(), tw.pending, err_msg=f"pending {tag}")
    np.testing.assert_array_equal(env.window_day().cpu().numpy(), os_["date_index"] - tw.active[0])


def _assert_step(kind, sc, env, tw, out, ref, tag):
    g_obs, g_rew, g_done = (t.cpu().numpy() for t in out[:3])
    o_obs, o_rew, o_done, o_term = ref
    np.testing.assert_array_equal(g_done.astype(bool), o_done, err_msg=f"done {tag}")
    np.testing.assert_array_equal(g_obs, o_obs.astype(np.float32), err_msg=f"obs {tag}")
    np.testing.assert_array_equal(g_rew, o_rew.astype(np.float32), err_msg=f"reward {tag}")
    if sc["auto"] and o_done.any():
        np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done],
                                      o_term[o_done].astype(np.float32), err_msg=f"term_obs {tag}")
    _assert_state(kind, sc, env, tw, tag)


def _reset_manual(kind, sc, env, tw, off, done, tag):
    """auto_reset off: reset(mask) of the envs that reported done, on their pending windows."""
    obs = env.reset(_dev(done.astype(np.uint8))).cpu().numpy()
    ref = tw.reset(off, done)
    np.testing.assert_array_equal(obs[done], ref[done].astype(np.float32), err_msg=f"reset obs {tag}")
    _assert_state(kind, sc, env, tw, f"reset {tag}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sc", SCENARIOS, ids=SCENARIO_IDS)
def test_random_windows_match_one_oracle_per_env(kind, sc):
    _need_gpu()
    close, info, turb = make_panel(sc["N"], sc["C"])
    script = Script(sc)
    env, tw = _make(kind, sc, script, close, info, turb)
    env.set_next_start(script.offsets0)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), tw.reset(script.offsets0).astype(np.float32))
    _assert_state(kind, sc, env, tw, "first reset")
    for s in range(sc["steps"]):
        a, off, redraw = script.step(s)
        if redraw is not None:                      # pending windows of a random subset rewritten
            m, ns, nt = redraw
            env.set_windows(ns, nt, mask=m)
            tw.set_pending(m, ns, nt)
        env.set_next_start(off)
        out = env.step(_dev(a))
        ref = tw.step(a, off, sc["auto"])
        _assert_step(kind, sc, env, tw, out, ref, f"step {s}")
        if not sc["auto"] and ref[2].any():
            _reset_manual(kind, sc, env, tw, off, ref[2], f"step {s}")
    assert tw.episodes_done.min() >= 2


# ------------------------------------------------------------------------------------------
# 3. whole-panel windows equal no windows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,C", [(5, 2), (30, 5), (30, 10)], ids=["nch1", "nch2", "nch0"])
def test_whole_panel_windows_equal_no_windows(kind, N, C):
    _need_gpu()
    Panel, Env, _ = classes(kind)
    E, T = 70, 30
    close, info, turb = make_panel(N, C, T)
    rng = np.random.default_rng(N + C)
    kw = dict(hmax=60_000, turbulence_threshold=40.0, patient=False, discrete_actions=False,
              random_start=False, **COMMON)
    plain, windowed = (Env(Panel(close, info, turb), E, **kw) for _ in range(2))
    windowed.set_windows(0, T)
    for env in (plain, windowed):
        env.enable_terminal_obs()
    starts = rng.integers(0, T // 2, E).astype(np.int32)
    for env in (plain, windowed):
        env.set_next_start(starts)
        env.reset()
    assert torch.equal(plain.obs, windowed.obs)
    n_done = 0
    for s in range(60):
        a = _dev(rng.uniform(-1, 1, (E, N)).astype(np.float32))
        starts = rng.integers(0, T // 2, E).astype(np.int32)
        for env in (plain, windowed):
            env.set_next_start(starts)
            env.step(a)
        for k in ("obs", "reward", "done"):
            assert torch.equal(getattr(plain, k), getattr(windowed, k)), (s, k)
        d = plain.done.bool()
        assert torch.equal(plain.term_obs[d], windowed.term_obs[d]), s
        for k in plain.state:
            assert torch.equal(plain.state[k], windowed.state[k]), (s, k)
        n_done += int(d.sum())
    assert n_done >= 2 * E
    assert torch.equal(windowed.window_day(), plain.state["date_index"])


# ------------------------------------------------------------------------------------------
# 4. random_start on windows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_random_start_draws_inside_each_window(kind):
    _need_gpu()
    Panel, Env, _ = classes(kind)
    E, L, N, C, pad = 4096, 40, 4, 2, 5
    close, info, turb = make_panel(N, C, L)
    rng = np.random.default_rng(4)
    w0 = rng.integers(pad, pad + 8, E)                       # per-env offsets inside the padding
    big = nan_padded([(np.concatenate([close, close[:8]]), np.concatenate([info, info[:8]]),
                       np.concatenate([turb, turb[:8]]))], pad, N, C)[:3]
    # (every window [w0, w0 + 40) lies in the 48 finite rows [pad, pad + 48))
    env = Env(Panel(*big), E, hmax=1000, random_start=True, seed=7, windows=(w0, w0 + L))
    ref = Env(Panel(close, info, turb), E, hmax=1000, random_start=True, seed=7)
    env.reset()
    ref.reset()
    st, rs = env.state_numpy(), ref.state_numpy()
    np.testing.assert_array_equal(st["start"] - w0, rs["start"])     # the same function of (seed, env, episode, hi)
    np.testing.assert_array_equal(st["start"], st["date_index"])
    assert (st["start"] - w0).max() < L // 2 and (st["start"] - w0).min() >= 0
    # windows of two different lengths pending; step every env past an episode end
    length = np.where(np.arange(E) % 2 == 0, 7, 20)
    p0 = rng.integers(pad, pad + 48 - length + 1)
    env.set_windows(p0, p0 + length)
    zero = torch.zeros(E, N, device="cuda")
    seen = np.zeros(E, bool)
    for s in range(L):
        _, _, done, _ = env.step(zero)
        d = done.cpu().numpy().astype(bool)
        new = d & ~seen
        st = env.state_numpy()
        lo, hi = p0[new], p0[new] + np.maximum(1, length[new] // 2)
        assert ((st["start"][new] >= lo) & (st["start"][new] < hi)).all(), s
        np.testing.assert_array_equal(st["start"][new], st["date_index"][new])
        seen |= d
        _no_nan(env, env.obs, env.reward)
    assert seen.all()
    np.testing.assert_array_equal(env.active_windows.cpu().numpy(), np.stack([p0, p0 + length]))
    draws = env.state_numpy()["start"] - p0
    for ln in (7, 20):                                       # every value of each range is drawn
        assert set(draws[length == ln].tolist()) == set(range(ln // 2))


# ------------------------------------------------------------------------------------------
# 5. pending edits wait for each env's own reset
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_pending_edits_wait_for_each_envs_own_reset(kind):
    _need_gpu()
    # small trades: episodes run to the last date; 4 steps: the envs on windows of up to 5 rows finish
    sc = dict(SCENARIOS[0], E=70, steps=4, hmax=2_000)
    close, info, turb = make_panel(sc["N"], sc["C"])
    rng = np.random.default_rng(5)
    E = sc["E"]
    script = Script(sc)
    env, tw = _make(kind, sc, script, close, info, turb)
    off = np.zeros(E, np.int32)
    env.set_next_start(off)
    env.reset()
    tw.reset(off)
    ns, nt = draw_windows(rng, T_ROWS, E)
    env.set_windows(ns, nt)                                   # mid-episode edit of rows 0, 1 of every env
    tw.set_pending(np.ones(E, bool), ns, nt)
    moved = np.zeros(E, bool)
    first_active = tw.active.copy()
    for s in range(sc["steps"]):
        a = rng.uniform(-1, 1, (E, sc["N"])).astype(np.float32)
        out = env.step(_dev(a))
        ref = tw.step(a, off, True)
        _assert_step(kind, sc, env, tw, out, ref, f"step {s}")
        moved |= ref[2]
        act = env.active_windows.cpu().numpy()
        np.testing.assert_array_equal(act[:, ~moved], first_active[:, ~moved])     # nothing until its done
        np.testing.assert_array_equal(act[:, moved], np.stack([ns, nt])[:, moved])
    assert moved.any() and not moved.all()
    # set_windows(s, t, mask=m) then reset(m) moves exactly the selected envs
    m = ~moved
    ms, mt = draw_windows(rng, T_ROWS, E)
    env.set_windows(ms, mt, mask=_dev(m))
    tw.set_pending(m, ms, mt)
    obs = env.reset(_dev(m.astype(np.uint8))).cpu().numpy()
    ref = tw.reset(off, m)
    np.testing.assert_array_equal(obs[m], ref[m].astype(np.float32))
    _assert_state(kind, sc, env, tw, "masked reset")
    act = env.active_windows.cpu().numpy()
    np.testing.assert_array_equal(act[:, m], np.stack([ms, mt])[:, m])
    np.testing.assert_array_equal(act[:, ~m], np.stack([ns, nt])[:, ~m])


# ------------------------------------------------------------------------------------------
# 6. redraw on done inside a captured graph
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_redraw_on_done_inside_a_captured_graph(kind):
    """step, then a torch.where redraw of the pending windows of the envs that reported done, as one
    graph; every replay equals the twins."""
    _need_gpu()
    sc = dict(SCENARIOS[0], E=130, steps=40)
    E, N = sc["E"], sc["N"]
    close, info, turb = make_panel(N, sc["C"])
    rng = np.random.default_rng(6)
    script = Script(sc)
    env, tw = _make(kind, sc, script, close, info, turb)      # the windows are attached before the capture
    off = np.zeros(E, np.int32)
    env.set_next_start(off)
    env.reset()
    tw.reset(off)
    act = torch.zeros(E, N, device="cuda")
    new_s = torch.zeros(E, dtype=torch.int32, device="cuda")
    new_t = torch.ones(E, dtype=torch.int32, device="cuda")

    def body():
        env.step(act)
        env.set_windows(new_s, new_t, mask=env.done)

    def feed():
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        ns, nt = draw_windows(rng, T_ROWS, E)
        act.copy_(torch.from_numpy(a))
        new_s.copy_(torch.from_numpy(ns.astype(np.int32)))
        new_t.copy_(torch.from_numpy(nt.astype(np.int32)))
        return a, ns, nt

    def check(tag, a, ns, nt):
        ref = tw.step(a, off, True)
        tw.set_pending(ref[2], ns, nt)
        _assert_step(kind, sc, env, tw, (env.obs, env.reward, env.done), ref, tag)

    fed = feed()
    side = torch.cuda.Stream()                      # one eager run first (caches, allocations)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    check("warm-up", *fed)
    g = torch.cuda.CUDAGraph()
    fed = feed()
    with torch.cuda.graph(g):
        body()
    for rep in range(sc["steps"]):
        if rep:
            fed = feed()
        g.replay()
        torch.cuda.synchronize()
        check(f"replay {rep}", *fed)
    assert tw.episodes_done.min() >= 2 and tw.n_reset_on_new_window >= E


# ------------------------------------------------------------------------------------------
# 7. clamping of invalid device-side windows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,C", [(5, 2), (30, 5), (30, 10)], ids=["nch1", "nch2", "nch0"])
def test_invalid_device_side_windows_are_clamped(kind, N, C):
    """Windows written on the device are not validated: starts < 0, ends > T and ends <= starts are
    clamped into the panel by the kernel (a wrong answer at worst); the date index stays a panel row."""
    _need_gpu()
    Panel, Env, _ = classes(kind)
    E, T = 70, 24
    close, info, turb = make_panel(N, C, T)
    rng = np.random.default_rng(9)
    env = Env(Panel(close, info, turb), E, hmax=20_000, random_start=False, turbulence_threshold=40.0,
              windows=(0, T))
    s = rng.integers(-5, T + 5, E)
    t = np.where(np.arange(E) % 3 == 0, s - rng.integers(0, 4, E), s + rng.integers(1, T, E))
    env.set_windows(_dev(s.astype(np.int32)), _dev(t.astype(np.int32)))
    env.set_next_start(rng.integers(-3, T + 3, E).astype(np.int32))
    env.reset()
    for _ in range(20):
        env.step(_dev(rng.uniform(-1, 1, (E, N)).astype(np.float32)))
        di = env.state["date_index"]
        assert int(di.min()) >= 0 and int(di.max()) < T
        act = env.active_windows
        assert int(act[0].min()) >= 0 and int(act[1].max()) <= T and bool((act[1] > act[0]).all())
        _no_nan(env, env.obs, env.reward)


# ------------------------------------------------------------------------------------------
# 8. two shards
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_shards_equal_the_single_batch(kind):
    _need_gpu()
    from finrl_amd.distributed import make_sharded_env, shard_range
    Panel = classes(kind)[0]
    sc = SCENARIOS[0]
    E, N = 131, sc["N"]
    close, info, turb = make_panel(N, sc["C"])
    rng = np.random.default_rng(8)
    ws, wt = draw_windows(rng, T_ROWS, E, one_row=(0, 70))
    kw = dict(kind=kind, windows=(ws, wt), random_start=False, device=torch.device("cuda", 0),
              **env_kwargs(sc))
    panel = Panel(close, info, turb)
    whole = make_sharded_env(panel, E, rank=0, world=1, **kw)
    shards = [make_sharded_env(panel, E, rank=r, world=2, **kw) for r in range(2)]
    bounds = [shard_range(E, r, 2) for r in range(2)]
    assert [sh.num_envs for sh in shards] == [hi - lo for lo, hi in bounds]

    def same(tag):
        for k in ("obs", "reward", "done", "windows", "active_windows"):
            assert torch.equal(getattr(whole, k), torch.cat([getattr(sh, k) for sh in shards], -1 if
                                                            k.endswith("windows") else 0)), (tag, k)
        for k in whole.state:
            assert torch.equal(whole.state[k], torch.cat([sh.state[k] for sh in shards], -1)), (tag, k)

    for env in [whole] + shards:
        env.reset()
    same("reset")
    n_done = 0
    for s in range(30):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        off = rng.integers(0, 6, E).astype(np.int32)
        whole.set_next_start(off)
        whole.step(_dev(a))
        for sh, (lo, hi) in zip(shards, bounds):
            sh.set_next_start(off[lo:hi])
            sh.step(_dev(a[lo:hi]))
        same(s)
        n_done += int(whole.done.sum())
    assert n_done >= 2 * E
