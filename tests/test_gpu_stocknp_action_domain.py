"""The array-state stock step on the action domain stated in include/finenv.h (array-state section,
"Action domain": any finite float32; the float32 product, truncated toward zero; strict compares against
min_action; both min() ties to the float32 operand; the reference exactly up to |a| = S = 2^31 - 128 and
the trade of +-S beyond).  HIP (VecStockTradingEnvNP, so through the C ABI) vs
oracle.stocknp.StockNpOracle at tolerance 0, on every step and for all 130 envs -- two full waves, one on
the kernel's all-float64 trade loops and one on the tagged loops throughout, and a 2-lane tail -- over two
episode ends.  The cases, their run shape and what each must reach are in tests/stocknp_action_cases.py;
tests/test_oracle_stocknp_action_domain.py holds the oracle to them without a GPU, and the oracle itself
is pinned to the unmodified reference on this domain by tests/golden/stocknp_actdom_*.npz.

On the parent of the commit that added this file 15 of its 56 tests failed
(profiles/stocknp_action_domain.md).  Every `past` test (plain at N = 1, 5, 30, 32; windows and history at
N = 5, 30): the float32 product was not bounded ahead of the cast, a product at or below -2^31 became
int32's minimum, whose negation is itself, and the "sale" of -2^31 shares added 2^31 shares to the holdings
and took their price out of the cash.  Every `quotient` test and `beyond` at max_stock 1e6 (N = 1, 5, 32): a
float32 `amount // price` of 2^22 or more is not the exact floor in NumPy, and the kernel bought the floor
wherever such a quotient cut a larger action short."""
import functools
import os
import sys

import numpy as np
import pytest

import stocknp_action_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E, T = sc.E, sc.T
STATE_KEYS = ("stocks", "cool_down", "amount", "amount_tag", "total_asset", "ta_tag", "gamma_reward", "g_tag",
              "episode_return")
PLAIN = [(c, N, ms, r) for c, ms, r in sc.CONFIGS for N in sc.NS]
FORMS = [(c, N) for c in sc.FORM_CASES for N in sc.FORM_NS]


def _id(p):
    return f"{p[0]}-N{p[1]}" + (f"-ms{p[2]:g}-rate{p[3]:g}" if len(p) > 2 else "")


@functools.lru_cache(maxsize=None)
def _oracle_trace(name, N, max_stock=128, rate=0.1, windowed=False):
    """One oracle run per parametrisation, shared by the launch forms; it reaches what the case exists for."""
    tr = sc.trace(name, N, max_stock, rate, windowed)
    sc.require_events(tr)
    return tr


def _env(tr, windowed=False):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    case = tr.case
    rows = T + sc.PAD if windowed else T
    price, tech, turb = (a[:rows] for a in case.arrays)
    cfg = {"price_array": price, "tech_array": tech, "turbulence_array": turb, "if_train": False}
    windows = (tr.starts_at, tr.starts_at + T) if windowed else None
    env = VecStockTradingEnvNP(cfg, E, max_stock=case.max_stock, min_stock_rate=case.rate, windows=windows,
                               **sc.KW)
    assert env.max_step == T - 1
    env.enable_terminal_obs()
    env.set_start_state(*case.starts)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), tr.obs0)
    return env


def _run(env, tr, after_step=None):
    for s, exp in enumerate(tr.steps):
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(tr.acts[s]).cuda())
        msg = f"step {s}"
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), exp["done"], err_msg=msg)
        st = env.state_numpy()
        for k in STATE_KEYS:
            np.testing.assert_array_equal(st[k], exp["state"][k], err_msg=f"{k} {msg}")
        # state["day"] is the panel row, the oracle's day counts from its window's start
        np.testing.assert_array_equal(st["day"] - tr.starts_at, exp["state"]["day"], err_msg=f"day {msg}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), exp["rew"].astype(np.float32), err_msg=msg)
        np.testing.assert_array_equal(g_obs.cpu().numpy(), exp["obs"], err_msg=msg)
        if exp["done"].any():
            np.testing.assert_array_equal(env.term_obs.cpu().numpy(), exp["term"], err_msg=msg)
        if after_step is not None:
            after_step(s, exp)


@pytest.mark.parametrize("param", PLAIN, ids=_id)
def test_stocknp_action_domain(param):
    tr = _oracle_trace(*param)
    _run(_env(tr), tr)


@pytest.mark.parametrize("param", FORMS, ids=_id)
def test_stocknp_action_domain_on_windows(param):
    """windows=: per-env windows of differing starts, so the envs of a wave stand on different panel rows
    (the WIN instantiation, per-env price loads); one oracle per window on its slice."""
    tr = _oracle_trace(*param, windowed=True)
    assert len(np.unique(tr.starts_at[:sc.WAVE])) == sc.PAD + 1
    env = _env(tr, windowed=True)
    np.testing.assert_array_equal(env.active_windows.cpu().numpy(), np.stack([tr.starts_at, tr.starts_at + T]))
    _run(env, tr)


@pytest.mark.parametrize("param", FORMS, ids=_id)
def test_stocknp_action_domain_with_history(param):
    """enable_history(): the recording instantiation returns the same step, and what it records is the
    oracle's total_asset, its tag and the holdings, by the header's recording rule."""
    import test_gpu_stocknp_history as hh
    tr = _oracle_trace(*param)
    env = _env(tr)
    hist = env.enable_history()
    assert hist.capacity == T
    trk = hh._Tracker(E, tr.case.N, T, T)
    trk.asset[:], trk.tag[:], trk.stocks[:], trk.start[:] = 0.0, 0, 0.0, 0     # (zero-initialised tensors)
    trk.arm(np.ones(E, bool), tr.steps[0]["pre"])
    trk.assert_equals(hist, "armed")

    def after_step(s, exp):
        trk.step(exp["post"], exp["done"])                  # the step's own values, before the auto-reset
        trk.assert_equals(hist, f"history step {s}")

    _run(env, tr, after_step)
    assert (trk.flags == hh.COMPLETE).all() and (trk.length == T).all()
