"""Running observation / return normalisation on the device: stable-baselines3's ``VecNormalize`` over
any ``BatchedEnv`` (finenv_vecnorm_* in include/finenv.h).  A training step costs two launches beside
the env's own, a frozen one (``training=False``) one; nothing allocates or reads back after
construction, so a ``step`` sits inside ``torch.cuda.graph``.

Out of scope: merging statistics across ranks, dict observations, and normalising the packed terminal
observations (``enable_terminal_obs`` of the wrapped env stays raw)."""
from __future__ import annotations

import ctypes as C

from . import _native as nat
from .vec_base import _checked_out_pitch


class RunningMeanStd:
    """One stats block on the device: ``mean`` / ``var`` / ``scale`` float64 [dim] and ``count``
    float64 [1] (0, 1, 1 / sqrt(1 + epsilon) and 1e-4 to begin with), with the partials buffer and the
    ticket word of its update launch.  ``update(x)`` merges a float32 [n, dim] batch (one launch),
    ``apply(x, out, center)`` normalises one with the stats as they are (one launch)."""

    def __init__(self, dim, epsilon=1e-8, clip=10.0, device="cuda"):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.FinenvError("finrl_amd has no CPU path: device must be a HIP GPU")
        if self.device.index is None:       # "cuda": the current device, as tensors report it
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dim, self.epsilon, self.clip = int(dim), float(epsilon), float(clip)
        if self.dim < 1:
            raise ValueError("RunningMeanStd needs dim >= 1")
        D, cap = self.dim, 2 * nat.VECNORM_MAX_TILES * self.dim
        self._block = torch.zeros(3 * D + 1 + cap, dtype=torch.float64, device=self.device)
        self.mean, self.var, self.scale = (self._block[k * D:(k + 1) * D] for k in range(3))
        self.count = self._block[3 * D:3 * D + 1]
        self._partials = self._block[3 * D + 1:]
        self._ticket = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.var.fill_(1.0)
        self.count.fill_(1e-4)
        self._lib = nat.lib()
        self.struct = nat.VecNormPtrs(
            self.mean.data_ptr(), self.var.data_ptr(), self.scale.data_ptr(), self.count.data_ptr(),
            self._partials.data_ptr(), self._ticket.data_ptr(), D, cap, self.epsilon, self.clip)
        self.ref = C.byref(self.struct)
        self.refresh()

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def refresh(self):
        """Recompute ``scale`` from ``var`` (after writing the statistics by hand)."""
        nat.check(self._lib.finenv_vecnorm_refresh(self.ref, self._stream()), None, "finenv_vecnorm_refresh")

    def _rows(self, x, what):
        """(n, row pitch in floats) of a float32 [n, dim] device tensor with unit column stride."""
        import torch
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.device != self.device or \
                x.dim() != 2 or x.shape[1] != self.dim or x.shape[0] < 1:
            raise ValueError(f"{what} must be [n >= 1, {self.dim}] float32 on {self.device}")
        n = x.shape[0]
        if self.dim > 1 and x.stride(1) != 1:
            raise ValueError(f"{what} needs unit column stride")
        pitch = self.dim if n == 1 else x.stride(0)
        if pitch < self.dim:
            raise ValueError(f"{what}: rows overlap (row stride smaller than {self.dim})")
        return n, pitch

    def update(self, x):
        n, pitch = self._rows(x, "update: x")
        rc = self._lib.finenv_vecnorm_update(self.ref, C.c_void_p(x.data_ptr()), n, pitch, self._stream())
        if rc:
            nat.check(rc, None, "finenv_vecnorm_update")

    def apply(self, x, out=None, center=True):
        import torch
        n, pitch = self._rows(x, "apply: x")
        if out is None:
            out = torch.empty(n, self.dim, dtype=torch.float32, device=self.device)
        no, pitch_out = self._rows(out, "apply: out")
        if no != n:
            raise ValueError("apply: out must have as many rows as x")
        rc = self._lib.finenv_vecnorm_apply(self.ref, C.c_void_p(x.data_ptr()), n, pitch,
                                            C.c_void_p(out.data_ptr()), pitch_out, int(bool(center)),
                                            self._stream())
        if rc:
            nat.check(rc, None, "finenv_vecnorm_apply")
        return out


class VecNormalize:
    """stable-baselines3's ``VecNormalize`` over a ``BatchedEnv``, following its documented formulas
    (tests/vecnorm_model.py restates them; SB3 itself is not a dependency).

    It presents the env surface the buffers use -- ``num_envs``, ``action_dim``, ``obs``, ``reward``,
    ``done``, ``device``, ``auto_reset``, ``step(actions, out=None)`` -- so
    ``RolloutBuffer.collect(norm, policy, first_obs)``, ``RolloutBuffer.step`` and ``ReplayBuffer.start`` /
    ``step`` work unchanged; any other attribute is the wrapped env's.

    ``step`` lets the env kernel write its raw outputs into the env's own persistent tensors, then
    normalises from those into the wrapper's persistent ``obs`` / ``reward`` or into ``out`` (any row
    pitch of ``out[0]``), in SB3's order: update the obs stats, normalise with the NEW stats, advance
    ``returns = returns * gamma + reward`` (float64), update the return stats, scale and clip the reward
    (no mean subtraction), zero ``returns`` where ``done``.  ``done`` is passed through: the env's tensor,
    or one copy inside the launches when ``out`` is given.  ``training=False`` (an attribute: flip it for
    evaluation) applies the frozen stats in one launch; ``norm_obs=False`` / ``norm_reward=False`` make
    that output a plain copy.

    Normalised values differ from SB3's ``(x - mean) / sqrt(var + epsilon)`` by at most one rounding
    before the cast to float32: the kernel multiplies by the stored ``1 / sqrt(var + epsilon)``.

    ``reset()`` resets the env, zeroes ``returns``, updates the obs stats (in training) and returns the
    normalised observation.  ``reset(mask)`` -- SB3 has no masked reset -- zeroes ``returns`` under the
    mask and normalises WITHOUT an update: the rows outside the mask were already counted."""

    supports_record = False
    _pitched = True             # step(out=...) honours any row pitch of out[0]

    def __init__(self, env, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0,
                 clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        import torch
        self.env = env
        self.training, self.norm_obs, self.norm_reward = bool(training), bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward = float(clip_obs), float(clip_reward)
        self.gamma, self.epsilon = float(gamma), float(epsilon)
        self.device = env.device
        self.num_envs, self.action_dim = env.num_envs, env.action_dim
        E, D = env.obs.shape
        self.obs_dim = D
        self.obs_rms = RunningMeanStd(D, self.epsilon, self.clip_obs, self.device)
        self.ret_rms = RunningMeanStd(1, self.epsilon, self.clip_reward, self.device)
        pitch = D if E == 1 else env.obs.stride(0)          # the wrapped env's own row pitch
        self._obs_buf = torch.zeros(E, pitch, dtype=torch.float32, device=self.device)
        self.obs = self._obs_buf[:, :D]
        self.reward = torch.zeros(E, dtype=torch.float32, device=self.device)
        self.returns = torch.zeros(E, dtype=torch.float64, device=self.device)
        self._pitch = pitch
        self._lib = nat.lib()
        self._ptrs = None

    def __getattr__(self, name):            # whatever the wrapper does not define is the env's
        if name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def done(self):
        return self.env.done

    @property
    def auto_reset(self):
        return self.env.auto_reset

    @auto_reset.setter
    def auto_reset(self, value):
        self.env.auto_reset = value

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ env protocol
    def _normalise_step(self, out):
        env = self.env
        if self._ptrs is None:              # the pointers of the persistent tensors, made once
            self._ptrs = tuple(C.c_void_p(t.data_ptr()) for t in
                               (env.obs, env.reward, env.done, self.returns, self.obs, self.reward))
        raw_obs, raw_rew, raw_done, returns, o, r = self._ptrs
        E, D = env.obs.shape
        pitch_out, d = self._pitch, None
        if out is not None:
            pitch_out = _checked_out_pitch(out, self.obs, self.reward, env.done)
            o, r, d = (C.c_void_p(t.data_ptr()) for t in out)
        rc = self._lib.finenv_vecnorm_step(
            self.obs_rms.ref, self.ret_rms.ref, raw_obs, D if E == 1 else env.obs.stride(0), raw_rew,
            raw_done, returns, self.gamma, o, pitch_out, r, d, E, int(self.training), int(self.norm_obs),
            int(self.norm_reward), self._stream())
        if rc:
            nat.check(rc, None, "finenv_vecnorm_step")

    def step(self, actions, out=None):
        """``BatchedEnv.step``'s contract: (obs, reward, done, None), views of persistent device tensors
        that the next call overwrites, or ``out`` = (obs [E, D] f32, reward [E] f32, done [E] u8)."""
        self.env.step(actions)
        self._normalise_step(out)
        if out is not None:
            return out[0], out[1], out[2], None
        return self.obs, self.reward, self.env.done, None

    def reset(self, mask=None):
        raw = self.env.reset(mask)
        if mask is None:
            self.returns.zero_()
            if self.training and self.norm_obs:
                self.obs_rms.update(raw)
        else:
            import torch
            self.returns.masked_fill_(mask.to(device=self.device, dtype=torch.bool), 0.0)
        if self.norm_obs:
            self.obs_rms.apply(raw, self.obs)
        else:
            self.obs.copy_(raw)
        return self.obs

    def get_original_obs(self):
        """The env's raw observation of the last step / reset (the env's own tensor)."""
        return self.env.obs

    def get_original_reward(self):
        """The env's raw reward of the last step (the env's own tensor)."""
        return self.env.reward

    # ------------------------------------------------------------------ caller tensors
    def normalize_obs(self, x, out=None):
        """Normalise any float32 [n, D] device tensor (rows may be pitched) with the current stats,
        never updating them: the off-policy use -- store raw transitions, normalise at sample time."""
        if not self.norm_obs:
            return x if out is None else out.copy_(x)
        return self.obs_rms.apply(x, out)

    def normalize_reward(self, r, out=None):
        """Scale and clip any float32 [n] device tensor of rewards with the current return stats."""
        import torch
        if not self.norm_reward:
            return r if out is None else out.copy_(r)
        if not torch.is_tensor(r) or r.dim() != 1 or not r.is_contiguous():
            raise ValueError("normalize_reward: r must be a contiguous [n] float32 device tensor")
        if out is None:
            out = torch.empty_like(r)
        elif out.shape != r.shape or not out.is_contiguous():
            raise ValueError("normalize_reward: out must be contiguous and shaped like r")
        self.ret_rms.apply(r.unsqueeze(1), out.unsqueeze(1), center=False)
        return out

    def unnormalize_obs(self, y):
        """The inverse of ``normalize_obs`` short of the clip (torch ops, float64 inside)."""
        import torch
        if not self.norm_obs:
            return y
        return (y.double() * torch.sqrt(self.obs_rms.var + self.epsilon) + self.obs_rms.mean).float()

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        """The statistics and ``returns`` as CPU tensors (synchronises)."""
        out = {}
        for tag, rms in (("obs", self.obs_rms), ("ret", self.ret_rms)):
            for name in ("mean", "var", "count"):
                out[f"{tag}_{name}"] = getattr(rms, name).detach().cpu().clone()
        out["returns"] = self.returns.detach().cpu().clone()
        return out

    def load_state_dict(self, state):
        """Load ``state_dict()``'s tensors; ``scale`` is recomputed on the device."""
        for tag, rms in (("obs", self.obs_rms), ("ret", self.ret_rms)):
            for name in ("mean", "var", "count"):
                getattr(rms, name).copy_(state[f"{tag}_{name}"])
            rms.refresh()
        self.returns.copy_(state["returns"])
