"""NumPy restatement of finrl_amd's VecNormalize (include/finenv.h, "Running observation / return
statistics"): stable-baselines3's documented RunningMeanStd / VecNormalize formulas in float64 -- a
two-pass batch mean and population variance, Chan's merge, the apply formula and the step order.

Two more restatements serve the tests only: `tiling` / `apply_tiling` repeat the host's choice of lane
layout, row tiles and merge runs (finenv_vecnorm.hip: layout_for, tiles_for, finalize), so that a test
can assert which path its shape takes, and `exact_stats` evaluates the documented recurrences in
rational arithmetic, which is what this float64 model is itself checked against."""
import collections
import decimal
import fractions

import numpy as np

MB, AB, APPLY_ROWS = 1024, 256, 16        # threads of a moments / an apply block; rows per apply lane
MAX_TILES = 128                           # FINENV_VECNORM_MAX_TILES
FIN_GROUPS, FIN_DEPTH = 16, 16            # merge runs per column at most; tiles in flight per run

Tiling = collections.namedtuple("Tiling", "vec lg chunks rl tile_rows tiles runs per column_blocks")
ApplyTiling = collections.namedtuple("ApplyTiling", "vec lg chunks tile_rows tiles")


def _layout(dim, pitches_ok, aligned):
    vec = bool(aligned and pitches_ok and dim >= 4)
    units, cap = ((dim + 3) // 4, 16) if vec else (dim, 64)
    lg = 0
    while (1 << lg) < cap and (1 << lg) < units:
        lg += 1
    return vec, lg, (units + (1 << lg) - 1) >> lg


def tiling(n_rows, dim, pitch, aligned=True):
    """The moments launch of an [n_rows, dim] batch with rows `pitch` floats apart (`aligned`: its base
    is 16-byte aligned): 16-byte units or dwords, log2 of the unit-lanes side by side, column chunks,
    row-lanes of a block, rows per tile, tiles, then the last block's merge: runs per column, tiles per
    run, and the blocks of 1024 columns it walks."""
    vec, lg, chunks = _layout(dim, pitch % 4 == 0, aligned)
    rl = MB >> lg
    tile_rows = -(-n_rows // (rl * MAX_TILES)) * rl
    tiles = -(-n_rows // tile_rows)
    runs = min(MB // dim if dim <= MB else 1, FIN_GROUPS)
    per = -(-tiles // runs)
    runs = -(-tiles // per)
    return Tiling(vec, lg, chunks, rl, tile_rows, tiles, runs, per, -(-dim // MB))


def apply_tiling(n_rows, dim, pitch_in, pitch_out, aligned=True):
    """The matrix part of an apply launch: the layout both tensors allow, rows per tile, row tiles."""
    vec, lg, chunks = _layout(dim, (pitch_in | pitch_out) % 4 == 0, aligned)
    tile_rows = (AB >> lg) * APPLY_ROWS
    return ApplyTiling(vec, lg, chunks, tile_rows, -(-n_rows // tile_rows))


def exact_stats(batches, epsilon=1e-8):
    """The documented recurrences over float32 batches ([n, dim] each) in rational arithmetic, from
    mean 0, var 1 and the float64 value of 1e-4 as the count -> (mean, var, count, scale): float64
    roundings of the exact mean / var / count, and of 1 / sqrt(var + epsilon) taken at 50 digits.
    Cost grows with every update (the denominators do): for small inputs only."""
    F = fractions.Fraction
    first = np.asarray(batches[0], np.float32)
    dim = first.reshape(len(first), -1).shape[1]
    mean, var, count = [F(0)] * dim, [F(1)] * dim, F(1e-4)
    for x in batches:
        x = np.asarray(x, np.float32).reshape(len(x), -1)
        n = x.shape[0]
        tot = count + n
        for d in range(dim):
            col = [F(float(v)) for v in x[:, d]]
            bm = sum(col) / n
            bv = sum((v - bm) ** 2 for v in col) / n
            delta = bm - mean[d]
            var[d] = (var[d] * count + bv * n + delta * delta * count * n / tot) / tot
            mean[d] = mean[d] + delta * n / tot
        count = tot
    ctx = decimal.Context(prec=50)
    eps = F(float(epsilon))
    scale = []
    for v in var:
        v = v + eps
        root = ctx.sqrt(ctx.divide(decimal.Decimal(v.numerator), decimal.Decimal(v.denominator)))
        scale.append(float(ctx.divide(decimal.Decimal(1), root)))
    as_f64 = lambda q: np.array([float(v) for v in q], np.float64)      # Fraction -> float rounds once
    return as_f64(mean), as_f64(var), float(count), np.array(scale, np.float64)


class RunningMeanStd:
    def __init__(self, dim, epsilon=1e-8, clip=10.0):
        self.mean = np.zeros(dim, np.float64)
        self.var = np.ones(dim, np.float64)
        self.count = 1e-4
        self.epsilon, self.clip = float(epsilon), float(clip)

    @property
    def scale(self):
        return 1.0 / np.sqrt(self.var + self.epsilon)

    def update(self, x):
        """x: [n, dim] (or [n] for dim 1).  Two passes: the mean, then the mean of squared deviations."""
        x = np.asarray(x, np.float64).reshape(len(x), -1)
        n = x.shape[0]
        bm = x.sum(axis=0) / n
        bv = ((x - bm) ** 2).sum(axis=0) / n
        delta = bm - self.mean
        tot = self.count + n
        self.mean = self.mean + delta * n / tot
        self.var = (self.var * self.count + bv * n + delta * delta * self.count * n / tot) / tot
        self.count = tot


def apply(x, mean, scale, clip, center=True):
    """y = (double(x) - mean) * scale, clipped to [-clip, clip], one rounding to float32; a NaN stays.
    mean / scale: the float64 values (the kernel's own, read back, for a tolerance-0 comparison)."""
    y = np.asarray(x, np.float32).astype(np.float64)
    if center:
        y = y - mean
    y = y * scale
    with np.errstate(invalid="ignore"):
        y = np.where(y < -clip, -clip, np.where(y > clip, clip, y))
    return y.astype(np.float32)


class VecNormalize:
    """The step order on raw (obs, reward, done) of the wrapped env."""

    def __init__(self, num_envs, obs_dim, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0,
                 clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        self.obs_rms = RunningMeanStd(obs_dim, epsilon, clip_obs)
        self.ret_rms = RunningMeanStd(1, epsilon, clip_reward)
        self.returns = np.zeros(num_envs, np.float64)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.gamma = float(gamma)

    def reset(self, obs):
        self.returns[:] = 0.0
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def normalize_obs(self, obs):
        if not self.norm_obs:
            return np.asarray(obs, np.float32).copy()
        return apply(obs, self.obs_rms.mean, self.obs_rms.scale, self.obs_rms.clip)

    def normalize_reward(self, reward):
        if not self.norm_reward:
            return np.asarray(reward, np.float32).copy()
        return apply(reward, 0.0, self.ret_rms.scale[0], self.ret_rms.clip, center=False)

    def step(self, obs, reward, done):
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)                                    # 1
        obs_out = self.normalize_obs(obs)                               # 2
        if self.training and self.norm_reward:
            self.returns = self.returns * self.gamma + np.asarray(reward, np.float32).astype(np.float64)   # 3
            self.ret_rms.update(self.returns)                           # 4
        reward_out = self.normalize_reward(reward)                      # 5
        if self.training and self.norm_reward:
            self.returns = np.where(np.asarray(done).astype(bool), 0.0, self.returns)      # 6
        return obs_out, reward_out
