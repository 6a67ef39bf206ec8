"""Shared inputs of the VecNormalize GPU tests: the column generator, and a scripted stand-in for a
batched env, so that a step test chooses its env count, width, row pitch and value range freely and
feeds the model the very arrays the wrapper sees."""
import functools

import numpy as np


@functools.lru_cache(maxsize=2)
def gaussian_columns(n, dim):
    """float32 [n, dim]: column 0 has mean 1e6 and sigma 1, the last column (dim > 1) is constant, the
    others have means and sigmas over six orders of magnitude -> (x, sigma per column, 0 = constant)."""
    rng = np.random.default_rng(1000 * dim + n % 997)
    mean = rng.uniform(-1, 1, dim) * 10.0 ** rng.integers(-2, 5, dim)
    sigma = 10.0 ** rng.uniform(-2, 3, dim)
    mean[0], sigma[0] = 1e6, 1.0
    if dim > 1:
        mean[-1], sigma[-1] = 123456.0, 0.0
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x *= sigma.astype(np.float32)
    x += mean.astype(np.float32)
    return x, sigma


class ScriptedEnv:
    """What VecNormalize touches of a batched env, played back from NumPy arrays: `obs` float32
    [F, E, D], `reward` float32 [F, E], `done` uint8 [F, E].  Frame 0 is what ``reset()`` shows; every
    ``step`` copies the next frame into the persistent ``obs`` (a view with rows `pitch` floats apart,
    NaN in the pad), ``reward`` and ``done``, and past the last frame the script starts over.  The
    frame counter lives on the device (``state["frame"]``), so a captured ``step`` advances on replay.
    The actions are checked for shape and otherwise ignored."""

    def __init__(self, obs, reward, done, pitch=None, action_dim=2, device="cuda"):
        import torch
        obs = np.ascontiguousarray(obs, np.float32)
        F, E, D = obs.shape
        assert reward.shape == (F, E) and done.shape == (F, E) and F >= 1
        self.device = torch.device("cuda", torch.cuda.current_device()) if device == "cuda" else torch.device(device)
        self.num_envs, self.action_dim, self.auto_reset = E, int(action_dim), True
        pitch = D if pitch is None else int(pitch)
        assert pitch >= D
        self._frames = F
        self._obs_script = torch.from_numpy(obs).to(self.device)
        self._reward_script = torch.from_numpy(np.ascontiguousarray(reward, np.float32)).to(self.device)
        self._done_script = torch.from_numpy(np.ascontiguousarray(done, np.uint8)).to(self.device)
        self._obs_buf = torch.full((E, pitch), float("nan"), dtype=torch.float32, device=self.device)
        self.obs = self._obs_buf[:, :D]
        self.reward = torch.zeros(E, dtype=torch.float32, device=self.device)
        self.done = torch.zeros(E, dtype=torch.uint8, device=self.device)
        self.state = {"frame": torch.zeros(1, dtype=torch.int64, device=self.device)}

    def _show(self):
        frame = self.state["frame"]
        self.obs.copy_(self._obs_script.index_select(0, frame)[0])
        self.reward.copy_(self._reward_script.index_select(0, frame)[0])
        self.done.copy_(self._done_script.index_select(0, frame)[0])

    def step(self, actions, out=None):
        assert out is None and tuple(actions.shape) == (self.num_envs, self.action_dim)
        self.state["frame"].add_(1).remainder_(self._frames)
        self._show()
        return self.obs, self.reward, self.done, None

    def reset(self, mask=None):
        """All envs: back to frame 0.  Under a mask the shown rows stay (nothing here depends on them)."""
        if mask is None:
            self.state["frame"].zero_()
            self._show()
        return self.obs
