"""NumPy restatement of finrl_amd's VecNormalize (include/finenv.h, "Running observation / return
statistics"): stable-baselines3's documented RunningMeanStd / VecNormalize formulas in float64 -- a
two-pass batch mean and population variance, Chan's merge, the apply formula and the step order."""
import numpy as np


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
