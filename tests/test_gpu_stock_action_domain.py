"""The stock step kernels on the part of the action domain no other test enters: actions on the
truncation boundaries of `int(action * hmax)`, actions outside [-1, 1] up to and past each kernel's
saturation value, and `cash // unit` at quotients of 10^6 .. 10^7.  HIP (VecStockTradingEnv, so
through the C ABI) vs oracle.stock.StockOracle with tolerance 0 on obs, reward, done, `realised`,
cash, shares, cost and trades, through every leaf of the step launcher's choice of instantiation
(`_LEAVES` of tests/test_gpu_stock_edges.py), on two full 64-env blocks and a partial one.

The reference does not clip (env_stocktrading.py:304-305); a kernel saturates the scaled integer at
`_amax` (include/finenv.h, "Action domain").  Where an action exceeds it the expectation is the
oracle's on `action_domain_cases.saturated()` actions.  Those cases, and every case that names a
scaled magnitude, run at a power-of-two hmax (128; 512 for the leaves whose hmax > 255 is what
selects their kernel), so that the division building the action and the kernel's f32 multiply are
both exact -- checked where the actions are built.  `amax - 1` / `amax + 1` are the nearest integers a
float32 product can be (2^25 -+ 1 is none).  NaN and +-inf actions are out of scope: the reference's
own cast is undefined there.

Before the N = 100 fast kernel saturated at 255 (it clamped at 2^23 and parked a * 128 + i as int16),
test_beyond_unit_interval and test_past_the_clamp failed at every (100, 100) leaf -- a scaled buy of
257 was booked as a sell of 255 and the like -- and test_past_the_clamp at N = 50, whose kernel
clamped at 2^24 where the header said 2^23 (profiles/stock_action_domain.md)."""
import functools

import numpy as np
import pytest

import action_domain_cases as adc
from test_gpu_stock_edges import _LEAVES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E, T, K = 130, 6, 2
WIDE_AMAX = 255             # WideGeom<100>::kMaxHmax: what the int16 keys of the N = 100 fast kernel hold


def _amax(N, hmax):
    """Saturation value of the kernel that steps (N, hmax): include/finenv.h, "Action domain"."""
    if N <= 32:
        return 1 << 25
    if N == 100 and hmax <= 255:
        return WIDE_AMAX
    return 1 << 23


def _panel(N, T_=T):
    rng = np.random.default_rng(77 + N)
    close = (50 + rng.uniform(0, 10, (T_, N))).astype(np.float32).astype(np.float64)
    tech = rng.normal(0, 1, (T_, K, N)).astype(np.float32).astype(np.float64)
    risk = np.abs(rng.normal(0, 30, T_))
    return close, tech, risk


@functools.lru_cache(maxsize=None)
def _oracle_trace(case, N, hmax, amax, use_turbulence):
    """(env kwargs, actions [S, E, N], per-step oracle outputs): computed once per distinct
    (case, N, hmax, amax) and shared by the leaves that differ in the launch form only."""
    from oracle.stock import StockOracle
    close, tech, risk = _panel(N)
    steps = 2 * T + 2
    if case == "boundary":
        rng = np.random.default_rng(N)
        act = adc.boundary_tiles(hmax, E, N, steps, seed=1000 * N + hmax)
        fed = act
        kw = dict(hmax=hmax, initial_amount=1_000_000, num_stock_shares=rng.integers(0, 40, N))
    else:
        mags = adc.magnitudes_inside(amax) if case == "inside" else adc.magnitudes_beyond(amax)
        if case == "inside" and amax == WIDE_AMAX:      # the magnitudes the wider kernels take, saturated
            mags = sorted(set(mags + adc.magnitudes_inside(1 << 23)))
        act, signed = adc.big_tiles(mags, hmax, E, N, steps, seed=2000 * N + hmax)
        fed = adc.saturated(act, hmax, amax)
        cash0, shares0 = adc.env_books(E, N, seed=N)
        kw = dict(hmax=hmax, initial_amount=cash0, num_stock_shares=shares0)
    kw["turbulence_threshold"] = float(np.median(risk)) if use_turbulence else None
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    out = [orc.reset()]
    trace, n_done = [], 0
    for s in range(steps):
        obs, rew, done, real = orc.step(fed[s], want_realised=True)
        assert done.all() or not done.any()               # lock-step: one whole-panel episode each
        term = obs
        if done.all():
            n_done += 1
            obs = orc.reset()                              # what vec_step does per env
        st = orc.state()
        trace.append(dict(obs=obs, term=term, rew=rew, done=done, real=real,
                          **{k: st[k].copy() for k in ("cash", "shares", "cost", "trades")}))
    assert n_done == 2
    assert max(t["shares"].max() for t in trace) < 2 ** 31 - 1     # the device keeps holdings as int32
    real = np.stack([t["real"] for t in trace])
    want = adc.scaled(fed, hmax)
    if case == "boundary":
        assert (real != 0).any(axis=(1, 2)).sum() == steps - 2
    elif not use_turbulence:
        adc.assert_both_bind(want, real, np.clip(signed, -amax, amax))
    return (close, tech, risk), kw, act, out[0], trace


def _run_leaf(trace_args, desync_hint, windows, track_stats=True):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    (close, tech, risk), kw, act, obs0, trace = _oracle_trace(*trace_args)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, track_stats=track_stats, **kw)
    env.enable_terminal_obs()
    env.enable_realised()
    if desync_hint:
        env.hint_desynchronised()
    if windows:
        env.set_windows(0, T)       # the WIN kernels; one whole-panel oracle stays the exact reference
    np.testing.assert_array_equal(env.reset().cpu().numpy(), obs0.astype(np.float32))
    for s, exp in enumerate(trace):
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(act[s]).cuda())
        msg = f"step {s}"
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), exp["done"], err_msg=msg)
        np.testing.assert_array_equal(env.realised.cpu().numpy(), exp["real"], err_msg=msg)
        st = env.state_numpy()
        for k in ("shares", "cash", "cost", "trades"):
            np.testing.assert_array_equal(st[k], exp[k], err_msg=f"{k} {msg}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), exp["rew"].astype(np.float32), err_msg=msg)
        np.testing.assert_array_equal(g_obs.cpu().numpy(), exp["obs"].astype(np.float32), err_msg=msg)
        if exp["done"].any():
            np.testing.assert_array_equal(env.term_obs.cpu().numpy(), exp["term"].astype(np.float32))


# (a) is a property of (N, launch form, hmax): the leaves without their own hmax
_FORMS = sorted({(N, d, w) for N, _, d, w in _LEAVES})


@pytest.mark.parametrize("hmax", [100, 255, 256])
@pytest.mark.parametrize("N,desync_hint,windows", _FORMS)
def test_truncation_boundaries(N, desync_hint, windows, hmax):
    """(a) k / hmax and both float32 neighbours for every integer k in [-hmax, hmax], +-0.0, +-1.0,
    the smallest normal, a denormal, |a * hmax| < 1 -- every value in both full blocks on every step,
    over two episode ends.  255 is the last hmax the N = 100 fast kernel takes, 256 the first that
    goes to the generic kernel."""
    _run_leaf(("boundary", N, hmax, _amax(N, hmax), False), desync_hint, windows)


@pytest.mark.parametrize("use_turbulence", [False, True])
@pytest.mark.parametrize("N,hmax,desync_hint,windows", _LEAVES)
def test_beyond_unit_interval(N, hmax, desync_hint, windows, use_turbulence):
    """(b) scaled magnitudes 255 .. amax, both signs, in one row with in-range actions and exact ties;
    per-env holdings and cash such that the action binds in some envs and holdings or cash in others
    (asserted from the oracle's `realised` for every magnitude).  The N = 100 fast kernel is also given
    the magnitudes up to 2^23 and must saturate them at 255.  With turbulence on (the TURB
    instantiations, here without the Sharpe sums) the turbulent steps sell everything instead."""
    h = adc.pow2_hmax(hmax)
    _run_leaf(("inside", N, h, _amax(N, h), use_turbulence), desync_hint, windows,
              track_stats=not use_turbulence)


@pytest.mark.parametrize("N,hmax,desync_hint,windows", _LEAVES)
def test_past_the_clamp(N, hmax, desync_hint, windows):
    """(c) amax + 1, 2 * amax, 2^30 and 2^31 - 128, both signs: the oracle on saturated actions."""
    h = adc.pow2_hmax(hmax)
    _run_leaf(("beyond", N, h, _amax(N, h), False), desync_hint, windows)


@pytest.mark.parametrize("N,hmax,desync_hint,windows", _LEAVES)
def test_floor_division_at_large_quotients(N, hmax, desync_hint, windows):
    """(d) one buy per env, bound by cash, at k = cash // unit in [10^6, amax): cash is fl(k * unit) or a
    float64 neighbour, and every env is a case where Python's exact `//` differs from
    floor(cash / unit) or from floor(cash * (1 / unit)).  The N = 100 fast kernel saturates at 255, so
    no such k exists for it: there k runs over [1, 255) with the same three-neighbour construction and
    without the "differs" requirement."""
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    h = adc.pow2_hmax(hmax)
    amax = _amax(N, h)
    wide = amax == WIDE_AMAX
    close, tech, risk = _panel(N, 3)
    tick, cash, q = adc.floordiv_cases(close[0], 1e-3, E, 1 if wide else 10 ** 6, amax, not wide,
                                       seed=N + h)
    act = np.zeros((E, N), np.float32)
    act[np.arange(E), tick] = amax / h                     # scaled: amax > k, so cash binds
    assert (adc.scaled(act, h)[np.arange(E), tick] == amax).all() and (q < amax).all()
    kw = dict(hmax=h, initial_amount=cash)
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    env.enable_realised()
    if desync_hint:
        env.hint_desynchronised()
    if windows:
        env.set_windows(0, 3)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    o_obs, o_rew, o_done, o_real = orc.step(act, want_realised=True)
    np.testing.assert_array_equal(o_real[np.arange(E), tick], q)      # the oracle's floordiv_exact == `//`
    g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(act).cuda())
    np.testing.assert_array_equal(env.realised.cpu().numpy(), o_real)
    st, os_ = env.state_numpy(), orc.state()
    for k in ("shares", "cash", "cost", "trades"):
        np.testing.assert_array_equal(st[k], os_[k], err_msg=k)
    np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done)
    np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32))
    np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32))
