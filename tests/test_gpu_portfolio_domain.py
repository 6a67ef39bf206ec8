"""The batched StockPortfolioEnv step (finenv_portfolio.hip) on the action and panel domain of
tests/portfolio_domain_cases.py: negative scores, exponentials that are subnormal, zero or infinite, a
float32 sum that overflows over finite terms, -inf scores; closes of 0, flat days and x1e6 jumps -- the
reference does not stabilise its softmax and takes whatever IEEE gives (include/finenv.h, "Portfolio action
and panel domain"), and so must the kernel.

Against oracle/portfolio_oracle.c: done, day, observation and terminal-observation rows exact; weights that
are 0 or NaN by overflow / underflow exact; every other weight inside the interval DERIVED from "expf within
1 ulp", and the new value inside the interval that follows from it and from the device's own value before the
step; NaN / +-inf / exact-0 values where the oracle has them; reward = float32 of the value; a reset clears a
NaN.  The windowed and the recording instantiations of the kernel against the plain one, bit for bit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import portfolio_domain_cases as pc  # noqa: E402

F32 = np.float32
AMOUNT = 1_000_000.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _env(close, cov, tech, E, **kw):
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    with np.errstate(divide="ignore", invalid="ignore"):      # PortfolioPanel.gross_returns(): zero closes
        env = VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, initial_amount=AMOUNT, **kw)
    env.enable_weights()
    env.enable_terminal_obs()
    return env


def _oracle(close, cov, tech, E):
    from oracle.portfolio import PortfolioOracle
    return PortfolioOracle(close, cov, tech, n_envs=E, initial_amount=AMOUNT)


def _f32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(F32)


def _bits_equal(a, b):
    return np.array_equal(a, b, equal_nan=True)


def checked_step(env, a, t, g, names, what, host_reset=False):
    """One device step on actions a [E, N] against the oracle's record t of it (pc.oracle_trace).  -> the
    device's outputs of the step (before any host reset), for the tests that compare kernels."""
    pre = env.state_numpy()
    np.testing.assert_array_equal(pre["day"], t["day0"], err_msg=what)
    obs, rew, done, _ = env.step(torch.from_numpy(a).cuda())
    obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
    w = env.weights.cpu().numpy()
    st = env.state_numpy()
    np.testing.assert_array_equal(done, t["done"], err_msg=what)
    live = ~done
    counts = dict(bounded=0, values=0)
    if live.any():
        counts["bounded"] = pc.check_weights(a[live], w[live], t["weights"][live], what)
        m = live & (names == "sum_order")
        if m.any():
            pc.check_sum_order(a[m], w[m], t["weights"][m], what)
        counts["values"] = pc.check_values(a[live], pre["value"][live], g[pre["day"][live]], st["value"][live],
                                           t["rew"][live], t["weights"][live], what)
        assert _bits_equal(rew[live], _f32(st["value"][live])), (what, "reward != float32(value)")
    if done.any():
        assert _bits_equal(rew[done], _f32(pre["last_reward"][done])), (what, "terminal reward")
        np.testing.assert_array_equal(env.term_obs.cpu().numpy()[done], t["term"][done].astype(F32),
                                      err_msg=what)
        if env.auto_reset:
            assert (st["value"][done] == AMOUNT).all(), (what, "value after the auto-reset")
        else:
            assert _bits_equal(st["value"][done], pre["value"][done]), what
    out = dict(weights=w, value=st["value"].copy(), reward=rew, done=done, day=st["day"].copy(),
               pre=pre, **counts)
    if host_reset and done.all():
        obs = env.reset().cpu().numpy()
        st = env.state_numpy()
        assert (st["value"] == AMOUNT).all(), (what, "value after reset()")
    np.testing.assert_array_equal(st["day"], t["day"], err_msg=what)
    np.testing.assert_array_equal(obs, t["obs"].astype(F32), err_msg=what)
    return out


def run_checked(E, N, K, T, steps, kinds, panel, auto_reset=True, seed=0):
    """A whole run; -> the oracle trace, the actions and per-step device outputs."""
    close, cov, tech = panel
    acts = pc.actions(kinds, E, N, steps, T, seed)
    names, _ = pc.kinds_of(E, kinds)
    obs0, trace = pc.oracle_trace(_oracle(close, cov, tech, E), acts, auto_reset=auto_reset)
    share = pc.finite_share(trace)
    assert share >= 0.5, f"only {share:.2f} of the trading (env, step) pairs start from a finite value"
    env = _env(close, cov, tech, E, auto_reset=auto_reset)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), obs0.astype(F32))
    g = pc.gross_returns(close)
    outs = [checked_step(env, acts[s], trace[s], g, names, f"step {s}", host_reset=not auto_reset)
            for s in range(steps)]
    assert sum(t["done"].all() for t in trace) >= 2, "fewer than two episode ends"
    assert sum(o["bounded"] for o in outs) > 0 and sum(o["values"] for o in outs) > 0
    return trace, acts, outs


def _kind_outcomes(trace, outs, E, N, kinds):
    """What the kinds exist for happened on the device: NaN weights and values from the poisoning kinds,
    all-zero weights and an unchanged value from `sum_overflow`, weights of exactly 1 / 0 from `one_hot`."""
    names, _ = pc.kinds_of(E, kinds)
    seen = dict.fromkeys(("nan_value", "sum_overflow", "one_hot", "all_underflow_row", "exp_overflow_row"), 0)
    T = _T(trace)
    for s, (t, o) in enumerate(zip(trace, outs)):
        live = ~t["done"]
        seen["nan_value"] += int((live & np.isfinite(o["pre"]["value"]) & np.isnan(o["value"])).sum())
        m = live & (names == "sum_overflow")
        if N >= 2 and m.any():
            assert (o["weights"][m] == 0).all()
            assert _bits_equal(o["value"][m], o["pre"]["value"][m]), f"step {s}: zero weights move the value"
            seen["sum_overflow"] += int(m.sum())
        m = live & (names == "one_hot")
        if m.any():
            assert ((o["weights"][m] == 1).sum(1) == 1).all() and ((o["weights"][m] == 0).sum(1) == N - 1).all()
            seen["one_hot"] += int(m.sum())
        for k in pc.POISONING:
            m = live & (names == k) & (pc.poison_step(np.arange(E) // len(kinds), T) == s % T)
            if m.any():
                assert np.isnan(o["weights"][m]).any(1).all() and np.isnan(o["value"][m]).all(), (s, k)
                seen[k + "_row"] += int(m.sum())
    assert all(v > 0 for k, v in seen.items() if k != "sum_overflow" or N >= 2), seen


def _T(trace):
    """Steps per episode of a lock-step trace: the first terminal step's index + 1."""
    return next(s for s, t in enumerate(trace) if t["done"].all()) + 1


SHAPES = [(128, 9, 2), (130, 30, 8), (70, 64, 1), (128, 1, 1), (128, 8, 0)]


@pytest.mark.parametrize("E,N,K", SHAPES)
def test_action_kinds(E, N, K):
    """Every action kind in every 64-env block, auto-reset on, a benign panel.  At N = 1 the weights are
    exactly 1 or NaN (`sum_overflow` is `wide` there)."""
    _need_gpu()
    T, steps = 12, 30
    trace, acts, outs = run_checked(E, N, K, T, steps, pc.KINDS, pc.benign_panel(T, N, K, 7 + N), seed=E + N)
    _kind_outcomes(trace, outs, E, N, pc.KINDS)
    if N == 1:
        w = np.concatenate([o["weights"][~o["done"]] for o in outs])
        assert ((w == 1) | np.isnan(w)).all() and (w == 1).any() and np.isnan(w).any()


def test_action_kinds_without_auto_reset():
    """The same run with the resets done on the host when every env is done: a NaN value stays through the
    terminal step and is gone after reset()."""
    _need_gpu()
    E, N, K, T, steps = 128, 9, 2, 12, 30
    trace, acts, outs = run_checked(E, N, K, T, steps, pc.KINDS, pc.benign_panel(T, N, K, 5), auto_reset=False,
                                    seed=3)
    _kind_outcomes(trace, outs, E, N, pc.KINDS)
    ends = [o for o in outs if o["done"].all()]
    assert ends and all(np.isnan(o["value"]).any() for o in ends)


@pytest.mark.parametrize("variant", ["zeros", "nan"])
@pytest.mark.parametrize("E,N,K", [(128, 9, 2), (70, 30, 1)])
def test_panel_values(E, N, K, variant):
    """pc.edit_close panels: returns of exactly 0, -1, +inf and NaN, x1e6 jumps.  The events are counted from
    the oracle's outputs among the pairs that start from a finite value; a `one_hot` env that holds exactly
    the ticker that goes to 0 ends at exactly 0.0 (checked by class in checked_step, and here)."""
    _need_gpu()
    T, steps = 14, 32
    close, cov, tech = pc.benign_panel(T, N, K, 11 + N)
    close = pc.edit_close(close, variant)
    trace, acts, outs = run_checked(E, N, K, T, steps, pc.PANEL_KINDS, (close, cov, tech), seed=E)
    ev = pc.panel_events(pc.gross_returns(close), trace)
    pc.require_panel_events(variant, ev)
    zero = sum(int((~t["done"] & (t["rew"] == 0)).sum()) for t in trace)
    zero_dev = sum(int((~o["done"] & (o["value"] == 0)).sum()) for o in outs)
    assert zero > 0 and zero_dev == zero
    if variant == "zeros":
        assert sum(int((o["value"] == np.inf).sum()) for o in outs) > 0


def test_windows_and_history_forms():
    """The WIN and HIST instantiations of the step kernel run the same softmax in differently compiled
    kernels: stepped beside the plain form on the same actions, weights agree bit for bit wherever both
    envs trade, value and reward wherever they started the step on the same panel day with the same
    value; every recorded history.weights row is env.weights of its step."""
    _need_gpu()
    E, N, K, T, steps = 128, 9, 2, 12, 30
    close, cov, tech = pc.benign_panel(T, N, K, 21)
    acts = pc.actions(pc.KINDS, E, N, steps, T, 17)
    names, _ = pc.kinds_of(E, pc.KINDS)
    _, trace = pc.oracle_trace(_oracle(close, cov, tech, E), acts)
    g = pc.gross_returns(close)
    plain = _env(close, cov, tech, E)
    start = (np.arange(E) // 7) % 3                              # staggered: a block holds all three
    win = _env(close, cov, tech, E, windows=(start, np.full(E, T)))
    rec = _env(close, cov, tech, E)
    hist = rec.enable_history(weights=True)
    for env in (plain, win, rec):
        env.reset()
    n_w = n_v = n_other_day = n_rec = 0
    for s in range(steps):
        a = torch.from_numpy(acts[s]).cuda()
        p = checked_step(plain, acts[s], trace[s], g, names, f"plain step {s}")
        for form, env in (("windows", win), ("history", rec)):
            what = f"{form} step {s}"
            pre = env.state_numpy()
            len0 = hist.length.cpu().numpy().copy() if form == "history" else None
            _, rew, done, _ = env.step(a)
            rew, done, w = rew.cpu().numpy(), done.cpu().numpy().astype(bool), env.weights.cpu().numpy()
            st = env.state_numpy()
            both = ~done & ~p["done"]
            assert _bits_equal(w[both], p["weights"][both]), what
            n_w += int(both.sum())
            n_other_day += int((both & (pre["day"] != p["pre"]["day"])).sum())
            same = (pre["day"] == p["pre"]["day"]) & \
                (pre["value"].view(np.uint64) == p["pre"]["value"].view(np.uint64)) & \
                (pre["last_reward"].view(np.uint64) == p["pre"]["last_reward"].view(np.uint64))
            if form == "history":
                assert same.all(), what
            else:
                assert same[start == 0].all(), what
            np.testing.assert_array_equal(done[same], p["done"][same], err_msg=what)
            assert _bits_equal(st["value"][same], p["value"][same]), what
            assert _bits_equal(rew[same], p["reward"][same]), what
            n_v += int(same.sum())
            if form == "history":
                len1 = hist.length.cpu().numpy()
                took = len1 == len0 + 1
                assert not (took & done).any() and (len1[~took] == len0[~took]).all(), what
                e = np.flatnonzero(took)
                hw = hist.weights.cpu().numpy()[len1[e] - 1, e]
                assert _bits_equal(hw, w[e]), (what, "history.weights row != env.weights")
                assert _bits_equal(hist.value.cpu().numpy()[len1[e] - 1, e], st["value"][e]), what
                n_rec += len(e)
                if done.all():
                    hist.arm()                                   # an auto-reset does not arm
    assert n_other_day > E and n_v > 1.3 * E * steps and n_rec > E * (steps - 4), (n_other_day, n_v, n_rec)
    assert n_w > 1.5 * E * steps


def test_reference_fixture_on_the_domain():
    """tests/golden/portfolio_domain.npz (the unmodified reference on every action kind and the `zeros`
    panel) on the device: 70 envs on the fixture's actions, resets on the host as in the fixture."""
    _need_gpu()
    z = np.load(os.path.join(HERE, "golden", "portfolio_domain.npz"), allow_pickle=False)
    T, N, K, S = z["cfg_int"].tolist()
    E = 70
    assert z["cfg_float"][0] == AMOUNT
    env = _env(z["close"], z["cov"], z["tech"], E, auto_reset=False)
    resets = dict(zip(z["reset_step"].tolist(), z["reset_obs"]))
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(obs, np.broadcast_to(resets[-1].astype(F32), obs.shape))
    n_done = n_bounded = 0
    for s in range(S):
        pre = env.state_numpy()
        a = torch.from_numpy(np.broadcast_to(z["actions"][s], (E, N)).copy()).cuda()
        obs, rew, done, _ = env.step(a)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
        w, st = env.weights.cpu().numpy(), env.state_numpy()
        np.testing.assert_array_equal(done, np.full(E, bool(z["done"][s])), err_msg=f"step {s}")
        np.testing.assert_array_equal(st["day"], z["day"][s], err_msg=f"step {s}")
        np.testing.assert_array_equal(obs, np.broadcast_to(z["obs"][s].astype(F32), obs.shape))
        for name, v in (("value", st["value"]), ("reward", rew), ("weights", w)):   # every env alike
            assert _bits_equal(v, np.broadcast_to(v[:1], v.shape)), (s, name)
        if z["done"][s]:
            assert _bits_equal(rew, _f32(pre["last_reward"])) and _bits_equal(st["value"], pre["value"])
            n_done += 1
            obs = env.reset().cpu().numpy()
            np.testing.assert_array_equal(obs, np.broadcast_to(resets[s].astype(F32), obs.shape))
            assert (env.state_numpy()["value"] == AMOUNT).all()
            continue
        assert _bits_equal(rew, _f32(st["value"]))
        for e in (0, 33, E - 1):
            n = pc.check_fixture_step(z, s, w[e], pre["value"][e], st["value"][e], f"env {e}")
        n_bounded += n
    assert n_done == 3 and n_bounded >= 20, (n_done, n_bounded)
