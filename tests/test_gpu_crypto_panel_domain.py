"""The crypto step on the panel values no other test feeds it (include/finenv.h,
`finenv_crypto_panel`: a trade needs `price > 0`): zero prices in every row but the one
action_norm_vector reads, and price levels from 1e-8 to 1e5 against an initial capital of 1e2, 3e4 and
1e9 -- `cash // price` from 0 to beyond 2^40, where the kernel's reciprocal-based floor division
relies on min() returning the action.  HIP (VecCryptoEnv, so through the C ABI) vs
oracle.crypto.CryptoOracle, exact, on two full 64-env waves and a partial one over two episode ends,
in the 8-, 16- and 32-wide builds (N = 1, 10, 17) with and without indicator columns; one run resets
part of the batch mid-episode, so that `time` differs inside a wave."""
import numpy as np
import pytest

import panel_domain_cases as pdc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E, T = 130, 12
KW = dict(lookback=1, buy_cost_pct=0.0012, sell_cost_pct=0.0008, gamma=0.98)
STATE = ("cash", "total_asset", "gamma_return", "episode_return", "time", "stocks")


def _run(name, N, W, capital, masked):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    from finrl_amd.vec_crypto import VecCryptoEnv
    from oracle.crypto import CryptoOracle
    price, tech = pdc.crypto_case(name, N, T, W, seed=17 * N + W)
    assert (price[0] > 0).all()
    steps = 2 * (T - 1) + 2
    acts = pdc.actions(E, N, steps, seed=N + W)
    orc = CryptoOracle(price, tech, n_envs=E, initial_capital=capital, **KW)
    env = VecCryptoEnv({"price_array": price, "tech_array": tech}, E, initial_capital=capital, **KW)
    env.enable_terminal_obs()
    np.testing.assert_array_equal(env.action_norm_vector, orc.norm)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset())
    rng = np.random.default_rng(N)
    pre, post, nd = [], [], 0
    for s in range(steps):
        pre.append(orc.state())
        o_obs, o_rew, o_done = orc.step(acts[s])
        post.append(orc.state())
        o_term = o_obs.copy()
        if o_done.any():
            nd += 1
            o_obs[o_done] = orc.reset_masked(o_done)[o_done]
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(acts[s]).cuda())
        msg = f"step {s}"
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done, err_msg=msg)
        st, os_ = env.state_numpy(), orc.state()
        for k in STATE:
            np.testing.assert_array_equal(st[k], os_[k], err_msg=f"{k} {msg}")
        np.testing.assert_array_equal(g_rew.cpu().numpy(), o_rew.astype(np.float32), err_msg=msg)
        np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs, err_msg=msg)
        if o_done.any():
            np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done], o_term[o_done])
        if masked and s in (2, 5, 7):
            m = rng.random(E) < 0.3
            exp = np.where(m[:, None], orc.reset_masked(m), o_obs)
            g = env.reset(torch.from_numpy(m.astype(np.uint8)).cuda()).cpu().numpy()
            np.testing.assert_array_equal(g, exp)
    assert nd >= 2
    return pdc.crypto_events(price, orc.norm, acts, pre, post)


@pytest.mark.parametrize("W", [40, 0])
@pytest.mark.parametrize("N", [1, 10, 17])
def test_crypto_zero_prices(N, W):
    """N = 1: the only asset is zero on the scattered days and the whole-row day (asset 1 does not
    exist)."""
    ev = _run("zero_closes", N, W, 3e4, masked=False)
    assert ev["sell_at_zero"] > 0 and ev["buy_at_zero"] > 0, dict(ev)
    assert ev["buy_action_binds"] > 0 and ev["buy_cash_binds"] > 0, dict(ev)


@pytest.mark.parametrize("capital", [1e2, 3e4, 1e9])
@pytest.mark.parametrize("W", [40, 0])
@pytest.mark.parametrize("N", [1, 10, 17])
def test_crypto_price_scales(N, W, capital):
    ev = _run("price_scales", N, W, capital, masked=False)
    assert ev["buy_action_binds"] + ev["buy_cash_binds"] > 0, dict(ev)
    if capital == 1e9:                      # asset 0 sits at 2e-8: 1e9 // 2e-8 = 5e16 > 2^40
        assert ev["buy_quotient_over_2p40"] > 0, dict(ev)
        assert ev["buy_action_binds"] > 0, dict(ev)
    if capital == 1e2 and N > 1:            # asset 1 sits at 9e4
        assert ev["buy_cash_binds"] > 0, dict(ev)


@pytest.mark.parametrize("name", ["zero_closes", "price_scales"])
def test_crypto_panel_domain_desynchronised(name):
    """Masked resets mid-episode: envs of one wave read different price rows."""
    ev = _run(name, 10, 40, 3e4, masked=True)
    assert ev["steps_with_mixed_time"] >= 10, dict(ev)
    if name == "zero_closes":
        assert ev["sell_at_zero"] > 0 and ev["buy_at_zero"] > 0, dict(ev)
