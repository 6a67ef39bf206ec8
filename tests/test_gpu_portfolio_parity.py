"""HIP StockPortfolioEnv (through the C ABI) vs the reference fixtures and the CPU oracle.

Exact: observation rows, done, day.  Portfolio value / reward: rel 1e-6 vs the reference
fixture and vs the oracle (float32 expf implementations differ by <= 1 ulp; north-star bound
1e-5); f32 reward output compared with rtol 1e-6."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[len("portfolio_"):-4]
               for p in glob.glob(os.path.join(GOLDEN, "portfolio_*.npz")))
NAMES.remove("domain")      # NaN / inf values: checked with derived bounds by the *_portfolio_domain tests


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.mark.parametrize("name", NAMES)
def test_portfolio_hip_matches_reference_fixture(name):
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    z = np.load(os.path.join(GOLDEN, f"portfolio_{name}.npz"), allow_pickle=False)
    T, N, K, S = z["cfg_int"].tolist()
    E = 70
    env = VecStockPortfolioEnv(PortfolioPanel(z["close"], z["cov"], z["tech"]), E,
                               initial_amount=z["cfg_float"][0], auto_reset=False)
    env.enable_weights()
    resets = dict(zip(z["reset_step"].tolist(), z["reset_obs"]))
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(obs, np.broadcast_to(resets[-1].astype(np.float32), obs.shape))
    nd = 0
    for s in range(S):
        a = torch.from_numpy(np.broadcast_to(z["actions"][s], (E, N)).copy()).cuda()
        obs, rew, done, _ = env.step(a)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        st = env.state_numpy()
        for e in (0, 31, 32, 63, 64, E - 1):
            assert bool(done[e]) == bool(z["done"][s]) and st["day"][e] == z["day"][s], (s, e)
            np.testing.assert_array_equal(obs[e], z["obs"][s].astype(np.float32))
            assert st["value"][e] == pytest.approx(z["value"][s], rel=1e-6)
            assert rew[e] == pytest.approx(z["reward"][s], rel=1e-6)
        if not z["done"][s]:
            np.testing.assert_allclose(env.weights[0].cpu().numpy(), z["weights"][s], rtol=1e-6)
        if z["done"][s]:
            nd += 1
            obs = env.reset().cpu().numpy()
            np.testing.assert_array_equal(
                obs, np.broadcast_to(resets[s].astype(np.float32), obs.shape))
    assert nd == 2


@pytest.mark.parametrize("cfg", [dict(E=1000, T=30, N=30, K=8, steps=70),
                                 dict(E=130, T=12, N=7, K=3, steps=30),
                                 dict(E=65, T=9, N=64, K=2, steps=20),
                                 dict(E=64, T=9, N=1, K=1, steps=20)])
def test_portfolio_hip_matches_oracle_random_batch(cfg):
    _need_gpu()
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    from oracle.portfolio import PortfolioOracle
    E, T, N, K = cfg["E"], cfg["T"], cfg["N"], cfg["K"]
    rng = np.random.default_rng(E)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    cov = rng.normal(0, 1e-4, (T, N, N))
    tech = rng.normal(0, 1, (T, K, N))
    orc = PortfolioOracle(close, cov, tech, n_envs=E, initial_amount=1e6)
    env = VecStockPortfolioEnv(PortfolioPanel(close, cov, tech), E, initial_amount=1e6)
    env.enable_terminal_obs()
    np.testing.assert_array_equal(env.reset().cpu().numpy(), orc.reset().astype(np.float32))
    nd = 0
    for s in range(cfg["steps"]):
        a = rng.uniform(0, 1, (E, N)).astype(np.float32)
        o_obs, o_rew, o_done, o_term = orc.vec_step(a)
        g_obs, g_rew, g_done, _ = env.step(torch.from_numpy(a).cuda())
        np.testing.assert_array_equal(g_done.cpu().numpy().astype(bool), o_done)
        np.testing.assert_array_equal(g_obs.cpu().numpy(), o_obs.astype(np.float32))
        np.testing.assert_allclose(g_rew.cpu().numpy(), o_rew, rtol=1e-6)
        st, os_ = env.state_numpy(), orc.state()
        np.testing.assert_array_equal(st["day"], os_["day"])
        np.testing.assert_allclose(st["value"], os_["value"], rtol=1e-6)
        if o_done.any():
            nd += 1
            np.testing.assert_array_equal(env.term_obs.cpu().numpy()[o_done],
                                          o_term[o_done].astype(np.float32))
    assert nd >= 2
