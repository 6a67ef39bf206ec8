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


# ------------------------------------------------------------------------------------ the model's own error
def model_vs_exact(batches, sigma):
    """The float64 model and exact_stats after every update of `batches` -> the worst error, as a
    fraction of a TENTH of the GPU tests' tolerances (var rtol 1e-8, mean atol 1e-8 * sigma, or
    1e-8 * |mean| where sigma is 0, scale rtol 1e-8 as var's; count within one rounding per update)."""
    dim = np.asarray(batches[0]).reshape(len(batches[0]), -1).shape[1]
    model, worst = vm.RunningMeanStd(dim), 0.0
    for k in range(len(batches)):
        model.update(batches[k])
        if k not in (0, len(batches) // 2, len(batches) - 1):           # (exact_stats restarts: three looks)
            continue
        mean, var, count, scale = vm.exact_stats(batches[:k + 1], model.epsilon)
        unit = np.where(np.asarray(sigma) > 0, sigma, np.abs(mean))
        worst = max(worst, (np.abs(model.mean - mean) / (1e-9 * unit)).max(),
                    (np.abs(model.var - var) / (1e-9 * var)).max(),
                    (np.abs(model.scale - scale) / (1e-9 * scale)).max())
        assert abs(model.count - count) <= (k + 1) * 2.0 ** -53 * count
    return worst


def exact_cases():
    from vecnorm_cases import gaussian_columns
    x, sigma = gaussian_columns(259, 3)
    rng = np.random.default_rng(60)
    many, many_sigma = gaussian_columns(60 * 7, 3)
    cuts = np.cumsum(np.concatenate([[0], rng.integers(1, 8, 60)]))
    pm = (1e6 + np.where(np.arange(70) % 2, 1.0, -1.0)).astype(np.float32)[:, None]
    const = np.full((70, 1), 123456.0, np.float32)
    return {"gaussian_columns(259, 3), one update": ([x], sigma),
            "gaussian_columns(259, 3), prefix and suffix too": ([x, x[:130], x[86:]], sigma),
            "60 updates of 1..7 rows": ([many[a:b] for a, b in zip(cuts[:-1], cuts[1:])], many_sigma),
            "1e6 +- 1": ([pm, pm[:36], pm[23:]], [1.0]),
            "constant": ([const, const[:36], const[23:]], [0.0])}


def test_model_stays_within_a_tenth_of_the_gpu_tolerances_of_exact_arithmetic():
    """The model is float64, two-pass; the recurrences in rational arithmetic over the same float32
    inputs (vm.exact_stats) are what it approximates.  Its error has to stay below a tenth of what the
    GPU tests allow the kernel against the model, so that the kernel keeps 90 % of that budget.
    Measured (fraction of the tenth, worst over mean, var and scale): 0.116 on gaussian_columns(259, 3)
    after one update and after three, and on 60 updates of 1..7 rows -- in each the mean of the 1e6
    column, one float64 ulp (2^-33) off the rounded exact value, which no float64 model can avoid; every
    other figure there is below 1e-3.  The 1e6 +- 1 column 1.6e-7, a constant column 1.7e-7."""
    for name, (batches, sigma) in exact_cases().items():
        worst = model_vs_exact(batches, sigma)
        print(f"model vs exact, {name}: {worst:.3g} of a tenth of the tolerance")
        assert worst <= 1.0, name


def test_exact_stats_on_a_hand_worked_case():
    """Rows 1, 2, 3 then 5 (dim 1) with the prior written out: c = float64(1e-4) exactly."""
    from fractions import Fraction as F
    c = F(1e-4)
    m1 = F(2) * 3 / (c + 3)
    v1 = (c + F(2, 3) * 3 + F(4) * c * 3 / (c + 3)) / (c + 3)
    d = 5 - m1
    m2 = m1 + d / (c + 4)
    v2 = (v1 * (c + 3) + d * d * (c + 3) / (c + 4)) / (c + 4)
    mean, var, count, scale = vm.exact_stats([np.array([1, 2, 3], np.float32), np.array([5], np.float32)], 0.25)
    assert (mean[0], var[0], count) == (float(m2), float(v2), float(c + 4))
    np.testing.assert_allclose(scale[0], 1 / np.sqrt(float(v2) + 0.25), rtol=4e-16)


def test_tiling_restates_the_host_rule():
    """Hand-worked from layout_for / tiles_for / finalize: the shapes the GPU tests name their paths by."""
    T, A = vm.Tiling, vm.ApplyTiling
    assert vm.tiling(259, 291, 304) == T(True, 4, 5, 64, 64, 5, 3, 2, 1)       # 73 units, 16 side by side
    assert vm.tiling(259, 291, 291) == T(False, 6, 5, 16, 16, 17, 3, 6, 1)     # the pitch forbids 16 bytes
    assert vm.tiling(259, 291, 304, aligned=False) == vm.tiling(259, 291, 291)
    assert vm.tiling(70001, 1001, 1001) == T(False, 6, 16, 16, 560, 126, 1, 126, 1)
    assert vm.tiling(259, 3, 4) == T(False, 2, 1, 256, 256, 2, 2, 1, 1)        # dim < 4: dwords
    assert vm.tiling(259, 1140, 1140) == T(True, 4, 18, 64, 64, 5, 1, 5, 2)
    assert vm.tiling(8192, 64, 64) == T(True, 4, 1, 64, 64, 128, 16, 8, 1)
    assert vm.tiling(8193, 64, 64) == T(True, 4, 1, 64, 128, 65, 13, 5, 1)     # past 128 tiles: taller tiles
    assert vm.tiling(131073, 1, 1) == T(False, 0, 1, 1024, 2048, 65, 13, 5, 1)
    assert vm.tiling(1, 1, 1) == T(False, 0, 1, 1024, 1024, 1, 1, 1, 1)
    assert vm.apply_tiling(4097, 1, 1, 1) == A(False, 0, 1, 4096, 2)
    assert vm.apply_tiling(300, 1140, 1140, 1144) == A(True, 4, 18, 256, 2)
    assert vm.apply_tiling(300, 1140, 1140, 1141) == A(False, 6, 18, 64, 5)    # either pitch decides
