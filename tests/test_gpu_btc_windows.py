"""Per-env episode windows of the batched BitcoinEnv (VecBitcoinEnv(windows=...),
finenv_btc_set_windows) on the MI355X: env e on panel rows [s_e, t_e) equals the reference env whose
arrays are those rows -- the recorded train / test / trade envs of btc_modes inside one mode_panel
panel, and one tests/btc_model.py model per env on its slice -- bit for bit."""
import numpy as np
import pytest

import btc_model as bm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(initial_account=1e3, transaction_fee_percent=1e-3, gamma=0.99)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(rng, T, P, W):
    p0 = 300.0 * np.exp(np.cumsum(rng.normal(0, 0.01, T)))
    cols = [p0] + [p0 * (1.003 + 0.002 * k) for k in range(P - 1)]
    return np.ascontiguousarray(np.stack(cols, 1)), rng.normal(0, 3e3, (T, W))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _windows(rng, T, E, lo=3, hi=9):
    length = rng.integers(lo, hi, E)
    start = (rng.random(E) * (T - length + 1)).astype(np.int64)
    return start, start + length


def test_three_modes_in_one_batch():
    """btc_modes: one env per mode over ONE panel, with NaN rows put between the modes' rows.  Each
    env replays the recorded reference env of its mode; no NaN reaches an output."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv, mode_panel
    modes = bm.load_fixture("btc_modes")
    names = ("train", "test", "trade")
    kw = modes["train"]["kwargs"]
    price, tech, win = mode_panel(modes["train"]["raw_price"], modes["train"]["raw_tech"],
                                  *[kw[k] for k in ("time_frequency", "start", "mid1", "mid2", "end")])
    # two NaN rows in front of every mode's rows and behind the last
    gap, ps, ts, start, end = 2, [], [], [], []
    for m in names:
        s, t = win[m]
        ps += [np.full((gap, price.shape[1]), np.nan), price[s:t]]
        ts += [np.full((gap, tech.shape[1]), np.nan), tech[s:t]]
        start.append(sum(len(x) for x in ps) - (t - s))
        end.append(start[-1] + t - s)
    ps.append(np.full((gap, price.shape[1]), np.nan))
    ts.append(np.full((gap, tech.shape[1]), np.nan))
    price_n, tech_n = np.concatenate(ps), np.concatenate(ts)
    env = VecBitcoinEnv(price_n, tech_n, 3, auto_reset=False, windows=(np.array(start), np.array(end)),
                        **bm.model_kwargs(kw))
    assert env.max_step == max(e - s for s, e in zip(start, end))
    n_ops = [len(modes[m]["ops"]) for m in names]
    obs = env.reset().cpu().numpy()
    for j, m in enumerate(names):
        assert modes[m]["ops"][0] == bm.OP_RESET
        np.testing.assert_array_equal(bm.bits(obs[j]), bm.bits(modes[m]["obs"][0]))
    for i in range(1, max(n_ops)):
        a = np.array([modes[m]["actions"][min(i, n - 1)] for m, n in zip(names, n_ops)], np.float32)
        o, r, d, _ = env.step(_dev(a[:, None]))
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
        st = env.state_numpy()
        assert np.isfinite(o).all() and np.isfinite(r).all()
        for k in bm.STATE_F64 + ("last_reward",):
            assert np.isfinite(st[k]).all(), k
        for j, (m, n) in enumerate(zip(names, n_ops)):
            c = modes[m]
            if i >= n:                                            # a shorter mode: past its end, defined
                assert d[j] == 1 and r[j] == 0
                continue
            what = f"{m} op {i}"
            np.testing.assert_array_equal(bm.bits(o[j]), bm.bits(c["obs"][i]), err_msg=what)
            assert bm.bits(r[j]) == bm.bits(np.float32(c["reward"][i])) and d[j] == c["done"][i], what
            assert bm.bits(st["last_reward"][j]) == bm.bits(c["reward"][i]), what
            for k in bm.STATE_F64:
                assert bm.bits(st[k][j]) == bm.bits(c[k][i]), f"{what}: {k}"
            assert st["stocks_tag"][j] == c["tag"][i] and st["window_day"][j] == i, what
    assert len(set(n_ops)) >= 2


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "manual"])
def test_random_windows_one_model_per_env(auto_reset):
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    E, T, P = 70, 40, 2
    rng = np.random.default_rng(31 + auto_reset)
    price, tech = _panel(rng, T, P, 8)
    s, t = _windows(rng, T, E)
    env = VecBitcoinEnv(price, tech, E, auto_reset=auto_reset, windows=(s, t), **SMALL)
    term = env.enable_terminal_obs()
    mb = bm.ModelBatch(price, tech, E, start=s, end=t, **SMALL)
    bm.assert_state_equal(env.state_numpy(), mb.state(), "constructed")
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(bm.bits(obs), bm.bits(np.stack(list(mb.reset().values()))))
    ends = np.zeros(E, int)
    for k in range(20):
        a = rng.uniform(-1, 1, E).astype(np.float32)
        got = env.step(_dev(a[:, None]))
        want = mb.step(a, auto_reset)
        bm.assert_state_equal(bm.assert_step_equal(env, got, want, f"step {k}"), mb.state(), f"step {k}")
        np.testing.assert_array_equal(env.window_day().cpu().numpy(), mb.state()["day"] - s)
        for e, row in want[3].items():
            np.testing.assert_array_equal(bm.bits(term[e].cpu().numpy()), bm.bits(row))
        ends += want[2]
        if not auto_reset and want[2].any():                      # the finished ones start again
            mask = want[2]
            obs = env.reset(_dev(mask.astype(np.uint8))).cpu().numpy()
            for e, row in mb.reset(mask).items():
                np.testing.assert_array_equal(bm.bits(obs[e]), bm.bits(row))
    assert (ends >= 2).all()


def test_edited_end_applies_next_step_edited_start_at_next_reset_and_detach():
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    E, T, P = 70, 30, 1
    rng = np.random.default_rng(17)
    price, tech = _panel(rng, T, P, 7)
    s, t = np.full(E, 4), np.full(E, 14)
    env = VecBitcoinEnv(price, tech, E, auto_reset=True, windows=(s, t), **SMALL)
    mb = bm.ModelBatch(price, tech, E, start=s, end=t, **SMALL)
    env.reset()
    mb.reset()

    def run(n, what):
        done_seen = np.zeros(E, bool)
        for k in range(n):
            a = rng.uniform(-1, 1, E).astype(np.float32)
            want = mb.step(a, True)
            bm.assert_state_equal(bm.assert_step_equal(env, env.step(_dev(a[:, None])), want, f"{what} {k}"),
                                  mb.state(), f"{what} {k}")
            done_seen |= want[2]
        return done_seen

    assert not run(3, "before").any()
    # half the envs: end moved in to row 9 (terminal row 8: the next step ends them), start moved to 6
    half = np.arange(E) % 2 == 0
    s2, t2 = np.where(half, 6, s), np.where(half, 9, t)
    env.set_windows(s2, t2)
    assert env.max_step == 10
    assert (env.state["day"] == 7).all()                          # nothing moves an env in mid episode
    for m, a, b in zip(mb.m, s2, t2):
        m.set_window(a, b)                  # (the model too reads its end every step, its start at a reset)
    np.testing.assert_array_equal(run(1, "edited end"), half)     # the end: from the next step
    st = env.state_numpy()
    np.testing.assert_array_equal(st["day"][half], 6)             # the start: at the reset that followed
    np.testing.assert_array_equal(st["day"][~half], 8)
    np.testing.assert_array_equal(st["window_day"], np.where(half, 0, 4))
    d = run(4, "on the new windows")
    assert d[half].all() and not d[~half].any()
    # detached: the whole panel
    env.set_windows(None)
    assert env.windows is None and env.max_step == T
    for m in mb.m:
        m.set_window(0, T)
    d = run(T, "detached")
    assert d.all() and (env.state["day"] < T).all()


def test_redrawn_windows_inside_a_captured_graph():
    """step, set_windows(mask=done), reset(done) captured once: the envs that finish restart on the
    windows drawn for them, with no host round trip."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    E, T, P = 70, 40, 1
    rng = np.random.default_rng(23)
    price, tech = _panel(rng, T, P, 7)
    s, t = _windows(rng, T, E)
    env = VecBitcoinEnv(price, tech, E, auto_reset=False, windows=(s, t), **SMALL)
    mb = bm.ModelBatch(price, tech, E, start=s, end=t, **SMALL)
    env.reset()
    mb.reset()
    a_in = torch.zeros(E, 1, device="cuda")
    new_s = torch.zeros(E, dtype=torch.int32, device="cuda")
    new_t = torch.zeros(E, dtype=torch.int32, device="cuda")
    outs = {}

    def body():
        obs, rew, done, _ = env.step(a_in)
        outs["step"] = (obs.clone(), rew.clone(), done.clone())
        env.set_windows(new_s, new_t, mask=done.bool())
        outs["obs"] = env.reset(done).clone()

    def follow(a, ns, nt, what):
        torch.cuda.synchronize()
        want = mb.step(a, False)
        got = outs["step"]
        np.testing.assert_array_equal(got[2].cpu().numpy().astype(bool), want[2], err_msg=what)
        np.testing.assert_array_equal(bm.bits(got[0].cpu().numpy()), bm.bits(want[0]), err_msg=what)
        np.testing.assert_array_equal(bm.bits(got[1].cpu().numpy()), bm.bits(want[1].astype(np.float32)))
        obs = outs["obs"].cpu().numpy()
        for e in np.flatnonzero(want[2]):
            mb.m[e].set_window(ns[e], nt[e])
            np.testing.assert_array_equal(bm.bits(obs[e]), bm.bits(mb.m[e].reset()), err_msg=what)
        bm.assert_state_equal(env.state_numpy(), mb.state(), what)
        return want[2]

    ns, nt = _windows(rng, T, E)
    new_s.copy_(_dev(ns.astype(np.int32)))
    new_t.copy_(_dev(nt.astype(np.int32)))
    body()
    ends = follow(np.zeros(E, np.float32), ns, nt, "warm-up").astype(int)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for k in range(16):
        a = rng.uniform(-1, 1, E).astype(np.float32)
        ns, nt = _windows(rng, T, E)
        a_in.copy_(_dev(a[:, None]))
        new_s.copy_(_dev(ns.astype(np.int32)))
        new_t.copy_(_dev(nt.astype(np.int32)))
        graph.replay()
        ends += follow(a, ns, nt, f"replay {k}")
    assert (ends >= 2).all()
    assert len(np.unique(env.windows[0].cpu().numpy())) > 10          # really on redrawn windows
