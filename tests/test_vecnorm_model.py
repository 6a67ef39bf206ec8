"""The NumPy restatement of VecNormalize (tests/vecnorm_model.py) against closed forms: successive
updates equal the moments of all rows seen, combined with the 1e-4 pseudo-count prior (mean 0, var 1),
and the step order on a hand-worked 2-env, 3-step case with a `done` in the middle."""
import numpy as np

import vecnorm_model as vm


def with_prior(rows):
    """(mean, var, count) of the prior (0, 1, 1e-4) merged once with the moments of all `rows`."""
    rows = np.asarray(rows, np.float64).reshape(len(rows), -1)
    n = rows.shape[0]
    bm = rows.mean(axis=0)
    bv = ((rows - bm) ** 2).mean(axis=0)
    tot = 1e-4 + n
    return bm * n / tot, (1e-4 + bv * n + bm * bm * 1e-4 * n / tot) / tot, tot


def test_three_updates_equal_the_concatenated_moments():
    rng = np.random.default_rng(3)
    batches = [rng.normal(3.0, 2.0, (n, 5)).astype(np.float32) for n in (7, 130, 41)]
    rms = vm.RunningMeanStd(5)
    assert rms.count == 1e-4 and (rms.mean == 0).all() and (rms.var == 1).all()
    for b in batches:
        rms.update(b)
    mean, var, count = with_prior(np.concatenate(batches))
    np.testing.assert_allclose(rms.mean, mean, rtol=1e-12)
    np.testing.assert_allclose(rms.var, var, rtol=1e-12)
    assert rms.count == count == 1e-4 + 178
    np.testing.assert_allclose(rms.scale, 1 / np.sqrt(var + 1e-8), rtol=1e-12)


def test_apply_formula():
    x = np.array([0.0, 1.0, 100.0, -100.0, np.nan, np.inf, -np.inf], np.float32)
    y = vm.apply(x, 1.0, 0.5, 10.0)
    np.testing.assert_array_equal(y, np.array([-0.5, 0.0, 10.0, -10.0, np.nan, 10.0, -10.0], np.float32))
    y = vm.apply(x, 1.0, 0.5, 10.0, center=False)
    np.testing.assert_array_equal(y, np.array([0.0, 0.5, 10.0, -10.0, np.nan, 10.0, -10.0], np.float32))


def test_step_order_hand_worked():
    """gamma = 0.5 keeps the return arithmetic exact.  Rewards [1, 2], [3, -1] (env 0 done), [0.5, 4]:
    returns [1, 2] -> [3.5, 0] -> zeroed to [0, 0] -> [0.5, 4]; the return stats after step k are the
    prior merged with every return seen so far (taken BEFORE the zeroing); each reward is scaled by the
    stats that already hold its own step; the observation is normalised by the NEW obs stats."""
    norm = vm.VecNormalize(2, 1, gamma=0.5, clip_obs=10.0, clip_reward=1.25)
    first = norm.reset(np.array([[4.0], [6.0]], np.float32))
    m, v, _ = with_prior([4.0, 6.0])
    np.testing.assert_allclose(first[:, 0], (np.array([4.0, 6.0]) - m) / np.sqrt(v + 1e-8), rtol=1e-6)
    obs = [np.array([[5.0], [9.0]], np.float32), np.array([[1.0], [2.0]], np.float32),
           np.array([[7.0], [7.0]], np.float32)]
    rew = [np.array([1.0, 2.0], np.float32), np.array([3.0, -1.0], np.float32), np.array([0.5, 4.0], np.float32)]
    done = [np.array([0, 0], np.uint8), np.array([1, 0], np.uint8), np.array([0, 0], np.uint8)]
    seen_obs, seen_ret = [4.0, 6.0], []
    want_returns = [[1.0, 2.0], [0.0, 0.0], [0.5, 4.0]]
    pre_zero = [[1.0, 2.0], [3.5, 0.0], [0.5, 4.0]]
    for k in range(3):
        o, r = norm.step(obs[k], rew[k], done[k])
        seen_obs += obs[k][:, 0].tolist()
        seen_ret += pre_zero[k]
        m, v, c = with_prior(seen_obs)
        np.testing.assert_allclose(norm.obs_rms.mean, m, rtol=1e-12)
        np.testing.assert_allclose(norm.obs_rms.var, v, rtol=1e-12)
        assert norm.obs_rms.count == c
        np.testing.assert_array_equal(o, vm.apply(obs[k], norm.obs_rms.mean, norm.obs_rms.scale, 10.0))
        np.testing.assert_allclose(o[:, 0], np.clip((obs[k][:, 0] - m) / np.sqrt(v + 1e-8), -10, 10), rtol=1e-6)
        m, v, c = with_prior(seen_ret)
        np.testing.assert_allclose(norm.ret_rms.mean, m, rtol=1e-12)
        np.testing.assert_allclose(norm.ret_rms.var, v, rtol=1e-12)
        assert norm.ret_rms.count == c
        np.testing.assert_allclose(r, np.clip(rew[k] / np.sqrt(v + 1e-8), -1.25, 1.25), rtol=1e-6)
        np.testing.assert_array_equal(norm.returns, want_returns[k])
    assert r[1] == np.float32(1.25)                       # 4 / std of the returns seen is past the clip

    frozen = vm.VecNormalize(2, 1, training=False, gamma=0.5)
    frozen.step(obs[0], rew[0], done[0])
    assert frozen.obs_rms.count == 1e-4 and frozen.ret_rms.count == 1e-4 and (frozen.returns == 0).all()
    off = vm.VecNormalize(2, 1, norm_obs=False, norm_reward=False)
    o, r = off.step(obs[0], rew[0], done[0])
    assert (o == obs[0]).all() and (r == rew[0]).all() and off.ret_rms.count == 1e-4
