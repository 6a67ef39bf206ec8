"""The stock step kernels on the part of the panel domain no other test enters (include/finenv.h,
"Panel domain"): zero closes -- unflagged (+0.0) and flagged (-0.0 on the device: the sign bit of
`panel.close` is the untradable flag) --, price levels from 1e-4 to 3e5 with per-env cash from 1e2 to
1e9 (floor-division quotients from 0 to beyond 2^40), the flag compare `tech_0 == 1.0` at the fp64 and
f32 neighbours of 1.0, and `turbulence >= threshold` at the threshold, its fp64 neighbours and +-0.0.
HIP (VecStockTradingEnv, so through the C ABI) vs oracle.stock.StockOracle with tolerance 0 on obs,
reward, done, `realised`, cash, shares, cost, trades, the terminal observation and the episode
summary, at every step over two episode ends, through every leaf of the step launcher's choice of
instantiation (`_LEAVES` of tests/test_gpu_stock_edges.py) on two full 64-env blocks and a partial
one.  tests/test_oracle_panel_domain.py pins the oracle to oracle/pandas_env.py on the same builders.

Every case first asserts, from the oracle trace alone (panel_domain_cases.require_stock_events), that
the events it exists for occur: a case cannot pass vacuously."""
import ctypes as C
import functools

import numpy as np
import pytest

import panel_domain_cases as pdc
from test_gpu_stock_edges import _LEAVES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E, T, K = 130, 8, pdc.K
STEPS = 2 * T + 2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _kw(case, hmax, use_turbulence):
    return dict(hmax=hmax, initial_amount=case.cash0, num_stock_shares=case.shares0,
                turbulence_threshold=case.threshold if use_turbulence else None)


@functools.lru_cache(maxsize=None)
def _oracle_trace(name, N, hmax, use_turbulence):
    """(case, actions [S, E, N], reset obs, per-step oracle outputs): computed once per distinct
    (case, N, hmax, turbulence) and shared by the leaves that differ in the launch form only."""
    from oracle.stock import StockOracle
    case = pdc.STOCK_CASES[name](N, T, E, seed=100 * N + hmax)
    acts = pdc.actions(E, N, STEPS, seed=7 * N + hmax)
    kw = _kw(case, hmax, use_turbulence)
    obs0, trace = pdc.stock_trace(case, hmax, use_turbulence, acts,
                                  lambda: StockOracle(case.close, case.tech, case.risk, n_envs=E, **kw))
    assert sum(bool(t["done"].all()) for t in trace) == 2
    assert max(t["shares"].max() for t in trace) < 2 ** 31 - 1     # the device keeps holdings as int32
    ev = pdc.stock_events(case, hmax, use_turbulence, acts, [t["pre"] for t in trace],
                          [t["real"] for t in trace], [t["post"] for t in trace])
    pdc.require_stock_events(name, ev, use_turbulence)
    return case, kw, acts, obs0, trace


_CASES = [(n, t) for n in pdc.STOCK_CASES for t in (False, True) if t or n != "threshold_zero"]


@pytest.mark.parametrize("name,use_turbulence", _CASES)
@pytest.mark.parametrize("N,hmax,desync_hint,windows", _LEAVES)
def test_panel_domain_leaf(N, hmax, desync_hint, windows, name, use_turbulence):
    """Every builder of panel_domain_cases, turbulence off and on (the threshold cases differ from a
    plain panel only with it on; `threshold_zero` runs only so), through every launch leaf."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    case, kw, acts, obs0, trace = _oracle_trace(name, N, hmax, use_turbulence)
    env = VecStockTradingEnv(StockPanel(case.close, case.tech, case.risk), E,
                             track_stats=not use_turbulence, **kw)
    env.enable_terminal_obs()
    env.enable_realised()
    if desync_hint:
        env.hint_desynchronised()
    if windows:
        env.set_windows(0, T)       # the WIN kernels; one whole-panel oracle stays the exact reference
    np.testing.assert_array_equal(env.reset().cpu().numpy(), obs0.astype(np.float32))
    for s, exp in enumerate(trace):
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(acts[s]).cuda())
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
        np.testing.assert_array_equal(env.episode_stats().cpu().numpy()[:, :5], exp["stats"][:, :5],
                                      err_msg=f"stats {msg}")


@pytest.mark.parametrize("N,hint", [(30, True), (30, False), (50, False), (100, False)])
def test_zero_closes_desynchronised(N, hint):
    """Envs on different days inside one wave (masked resets mid-episode) over `zero_closes` with
    turbulence on: the lock-step leaves share one price row in LDS, while the per-lane gathers
    (`price_signed`, the loops taken when the days differ) have their own copies of the zero-close
    and flag rules and are reached only this way."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle, lib, _p
    hmax, steps = 100, 3 * T
    case = pdc.zero_closes(N, T, E, seed=11 * N)
    acts = pdc.actions(E, N, steps, seed=N + 1)
    kw = _kw(case, hmax, True)
    orc = StockOracle(case.close, case.tech, case.risk, n_envs=E, **kw)
    env = VecStockTradingEnv(StockPanel(case.close, case.tech, case.risk), E, **kw)
    env.enable_realised()
    env.hint_desynchronised(hint)
    rng = np.random.default_rng(N)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    keys = ("cash", "shares", "cost", "trades", "day", "price_day", "turbulence")
    pre, post, real, mixed = [], [], [], 0
    for s in range(steps):
        pre.append({k: v.copy() for k, v in orc.state().items() if k in keys})
        mixed += len(np.unique(pre[-1]["price_day"])) > 1
        o_obs, o_rew, o_done, o_real = orc.step(acts[s], want_realised=True)
        post.append({k: v.copy() for k, v in orc.state().items() if k in keys})
        real.append(o_real)
        for e in np.nonzero(o_done)[0]:
            lib().stock_oracle_reset_env(orc._h, C.c_int(int(e)), _p(o_obs[e]))
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(acts[s]).cuda())
        msg = f"step {s}"
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done, err_msg=msg)
        np.testing.assert_array_equal(env.realised.cpu().numpy(), o_real, err_msg=msg)
        st, os_ = env.state_numpy(), orc.state()
        for k in ("shares", "cash", "cost", "trades", "day", "price_day"):
            np.testing.assert_array_equal(st[k], os_[k], err_msg=f"{k} {msg}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32), err_msg=msg)
        np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32), err_msg=msg)
        if s in (1, 2, 4, 9):
            m = rng.random(E) < 0.3
            exp = o_obs.astype(np.float32)
            for e in np.nonzero(m)[0]:
                row = np.empty(orc.D)
                lib().stock_oracle_reset_env(orc._h, C.c_int(int(e)), _p(row))
                exp[e] = row.astype(np.float32)
            g = env.reset(torch.from_numpy(m.astype(np.uint8)).cuda()).cpu().numpy()
            np.testing.assert_array_equal(g, exp)
    assert mixed >= steps - 4
    ev = pdc.stock_events(case, hmax, True, acts, pre, real, post)
    pdc.require_stock_events("zero_closes", ev, True)
