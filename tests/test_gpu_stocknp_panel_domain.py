"""The array-state stock step on the panel values no other test feeds it (include/finenv.h,
`finenv_stocknp_panel`: a trade needs `price > 0`): zero prices in every position but row 0, price
levels from 1e-3 to 1e5 against start amounts from 1e2 to 1e9, turbulent days and a day exactly on
the threshold.  HIP (VecStockTradingEnvNP, so through the C ABI) vs oracle.stocknp.StockNpOracle,
exact, on two full 64-env waves and a partial one over two episode ends.  The kernel trades on plain
doubles once every env of a wave carries a float64 cash and on tagged values before that; env 70 is
fed zero actions, so its wave stays on the tagged loops throughout.  Each case first asserts from the
oracle trace that both forms meet zero-priced sell and buy requests."""
import functools

import numpy as np
import pytest

import panel_domain_cases as pdc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E, T = 130, 10
STEPS = 2 * (T - 1) + 2
IDLE = 70                           # this env never trades: its cash keeps the tag it started with
KW = dict(gamma=0.98, buy_cost_pct=0.0012, sell_cost_pct=0.0008)


@functools.lru_cache(maxsize=None)
def _oracle_trace(name, N):
    from oracle.stocknp import StockNpOracle
    arrays, stocks0, amount0, tag0 = pdc.np_case(name, N, T, E, seed=31 * N + len(name))
    acts = pdc.actions(E, N, STEPS, seed=N)
    acts[:, IDLE, :] = 0.0
    orc = StockNpOracle(arrays["price_array"], arrays["tech_array"], arrays["turbulence_array"],
                        n_envs=E, **KW)
    orc.set_initial(stocks0, amount0, tag0)
    obs0 = orc.reset()
    trace, pre, post = [], [], []
    for s in range(STEPS):
        pre.append(orc.state())
        obs, rew, done = orc.step(acts[s])
        assert done.all() or not done.any()
        post.append(orc.state())
        term = obs
        if done.all():
            obs = orc.reset()
        trace.append(dict(obs=obs, term=term, rew=rew, done=done, state=orc.state()))
    assert sum(bool(t["done"].all()) for t in trace) == 2
    ev = pdc.np_events(orc.price, orc.turb_bool, 100, 10, acts, pre, post)
    assert orc.turb_bool[4] == 0.0 and orc.turb_bool[6] == 1.0
    assert ev["steady_wave_steps"] > 0 and ev["mixed_wave_steps"] >= STEPS, dict(ev)
    if name == "zero_closes":
        for k in ("sell_at_zero_steady", "sell_at_zero_mixed", "buy_at_zero_steady", "buy_at_zero_mixed",
                  "turbulent_zero_liquidated"):
            assert ev[k] > 0, (k, dict(ev))
    else:
        assert ev["buy_action_binds"] > 0 and ev["buy_cash_binds"] > 0, dict(ev)
    return arrays, stocks0, amount0, tag0, acts, obs0, trace


@pytest.mark.parametrize("N", [5, 30])
@pytest.mark.parametrize("name", ["zero_closes", "price_scales"])
def test_stocknp_panel_domain(name, N):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    from finrl_amd.vec_stocknp import VecStockTradingEnvNP
    arrays, stocks0, amount0, tag0, acts, obs0, trace = _oracle_trace(name, N)
    env = VecStockTradingEnvNP(arrays, E, **KW)
    env.enable_terminal_obs()
    env.set_start_state(stocks0, amount0, tag0)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), obs0)
    for s, exp in enumerate(trace):
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(acts[s]).cuda())
        msg = f"step {s}"
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), exp["done"], err_msg=msg)
        st = env.state_numpy()
        for k in ("stocks", "cool_down", "amount", "amount_tag", "total_asset", "ta_tag", "gamma_reward",
                  "g_tag", "episode_return", "day"):
            np.testing.assert_array_equal(st[k], exp["state"][k], err_msg=f"{k} {msg}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), exp["rew"].astype(np.float32), err_msg=msg)
        np.testing.assert_array_equal(g_obs.cpu().numpy(), exp["obs"], err_msg=msg)
        if exp["done"].any():
            np.testing.assert_array_equal(env.term_obs.cpu().numpy(), exp["term"])
