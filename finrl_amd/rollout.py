"""Device-resident PPO rollout buffers filled by the env kernels without copies
(BASELINE.json configs[4]), plus the GAE scan kernel and the shuffled minibatches of
an update epoch, each drawn and gathered in one launch (finenv_rollout_minibatch)."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from . import _native as nat
from .vec_base import obs_pitch_for

# stable-baselines3's RolloutBufferSamples: the same field order; the four scalar fields are [B]
RolloutBufferSamples = namedtuple(
    "RolloutBufferSamples",
    ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns"))


class RolloutBuffer:
    """[n_steps, E, ...] tensors on the env's device.  ``collect(env, policy)`` steps the env
    n_steps times writing observations / rewards / dones directly into slice t (the C ABI
    takes output pointers per step, so no staging copy exists).

    ``get(batch_size)`` / ``minibatch(k, batch_size)`` yield the shuffled minibatches of an update
    epoch (SB3's ``RolloutBuffer.get``): the order is a stateless permutation of the
    ``n_steps * num_envs`` rows, a pure function of (``seed``, epoch number) computed inside the one
    launch that also gathers the six fields (include/finenv.h, "Shuffled minibatches").  ``epoch``
    (int64 [1]) is the device word the kernel reads and ``epochs`` its host mirror; ``next_epoch()``
    bumps both, the device word in-stream, so a captured epoch of minibatches plus ``next_epoch()``
    draws a fresh permutation at every replay (the host mirror does not follow replays).

    ``obs_pitch`` is the row pitch of ``obs`` in floats: "packed" (the default: ``obs_dim``), "aligned",
    or an int >= ``obs_dim``; with a pitch above ``obs_dim`` ``obs`` is the view without the pad."""

    def __init__(self, n_steps, num_envs, obs_dim, action_dim, device="cuda", seed=0, obs_pitch="packed"):
        import torch
        self.n_steps, self.num_envs = int(n_steps), int(num_envs)
        self.obs_dim, self.action_dim = int(obs_dim), int(action_dim)
        self.obs_pitch = obs_pitch_for(self.obs_dim, obs_pitch)
        self.seed = int(seed) & (2 ** 64 - 1)
        kw = dict(device=device, dtype=torch.float32)
        self._obs_buf = torch.zeros(n_steps + 1, num_envs, self.obs_pitch, **kw)
        # obs[t] seen before step t
        self.obs = self._obs_buf if self.obs_pitch == self.obs_dim else self._obs_buf[:, :, :self.obs_dim]
        self.actions = torch.zeros(n_steps, num_envs, action_dim, **kw)
        self.rewards = torch.zeros(n_steps, num_envs, **kw)
        self.dones = torch.zeros(n_steps, num_envs, device=device, dtype=torch.uint8)
        self.values = torch.zeros(n_steps, num_envs, **kw)
        self.log_probs = torch.zeros(n_steps, num_envs, **kw)
        self.advantages = torch.zeros(n_steps, num_envs, **kw)
        self.returns = torch.zeros(n_steps, num_envs, **kw)
        self.epoch = torch.zeros(1, device=device, dtype=torch.int64)
        self.epochs = 0
        self.last_rows = None       # int32 [B]: the flat rows t * E + e of the last minibatch
        self._view = None
        self._batches = {}          # batch size -> (samples, rows)
        self._structs = {}          # (batch size, rows of the minibatch) -> (samples, struct, rows)

    def put(self, t, actions, values, log_probs):
        """Store the policy's outputs of step t (one launch: finenv_rollout_put)."""
        import torch
        L = nat.lib()
        dev = self.rewards.device
        a = actions.to(dev, torch.float32).contiguous()
        v = values.to(dev, torch.float32).contiguous()
        lp = log_probs.to(dev, torch.float32).contiguous()
        if a.numel() != self.actions[t].numel() or v.numel() != self.num_envs or lp.numel() != self.num_envs:
            raise ValueError("put: expected actions [E, A], values [E], log_probs [E]")
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nat.check(L.finenv_rollout_put(
            C.c_void_p(a.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(lp.data_ptr()),
            C.c_void_p(self.actions[t].data_ptr()), C.c_void_p(self.values[t].data_ptr()),
            C.c_void_p(self.log_probs[t].data_ptr()), self.num_envs,
            self.actions.shape[2], stream), None, "finenv_rollout_put")

    def step(self, env, t, actions, values, log_probs):
        """Store the policy's outputs of step t and step the env into slice t: one launch where the
        env can record them itself (`supports_record`: finenv_crypto_step_record), else two."""
        import torch
        out = (self.obs[t + 1], self.rewards[t], self.dones[t])
        dev, E, A = self.rewards.device, self.num_envs, self.actions.shape[2]
        # anything the one-launch form cannot take (other device, dtype, layout, size, alignment)
        # goes through put(), which converts, + a plain step
        fused = getattr(env, "supports_record", False) and E % 4 == 0 and (E * A) % 4 == 0 and \
            all(torch.is_tensor(x) and x.device == dev and x.dtype == torch.float32 and
                x.is_contiguous() and x.data_ptr() % 16 == 0 and x.numel() == n
                for x, n in ((actions, E * A), (values, E), (log_probs, E)))
        if fused:
            env.step(actions, out=out, record=(values, log_probs, self.actions[t], self.values[t],
                                               self.log_probs[t]))
        else:
            self.put(t, actions, values, log_probs)
            env.step(self.actions[t], out=out)

    def collect(self, env, policy, first_obs):
        """policy(obs) -> (actions [E,A] f32, values [E], log_probs [E]) on device."""
        self.obs[0].copy_(first_obs)
        for t in range(self.n_steps):
            a, v, lp = policy(self.obs[t])
            self.step(env, t, a, v, lp)
        return self.obs[self.n_steps]

    def compute_returns_and_advantage(self, last_values, gamma=0.99, gae_lambda=0.95):
        import torch
        L = nat.lib()
        lv = last_values.to(self.rewards.device, torch.float32).contiguous()
        stream = C.c_void_p(torch.cuda.current_stream(self.rewards.device).cuda_stream)
        nat.check(L.finenv_gae_scan(
            C.c_void_p(self.rewards.data_ptr()), C.c_void_p(self.values.data_ptr()),
            C.c_void_p(self.dones.data_ptr()), C.c_void_p(lv.data_ptr()),
            C.c_void_p(self.advantages.data_ptr()), C.c_void_p(self.returns.data_ptr()),
            self.n_steps, self.num_envs, float(gamma), float(gae_lambda), stream), None,
            "finenv_gae_scan")
        return self.advantages, self.returns

    # ------------------------------------------------------------------ shuffled minibatches
    def _shape(self):
        return (f"n_steps={self.n_steps}, num_envs={self.num_envs} ({self.n_steps * self.num_envs} rows), "
                f"obs_dim={self.obs_dim}, action_dim={self.action_dim}")

    def _persistent(self, B, n):
        """(samples, finenv_rollout_batch, rows) of the n leading rows of batch size B's outputs."""
        import torch
        if (B, n) not in self._structs:
            if B not in self._batches:
                kw = dict(dtype=torch.float32, device=self.epoch.device)
                o = torch.zeros(B, self.obs_pitch, **kw)
                self._batches[B] = (RolloutBufferSamples(
                    o[:, :self.obs_dim], torch.zeros(B, self.action_dim, **kw),
                    *(torch.zeros(B, **kw) for _ in range(4))),
                    torch.zeros(B, dtype=torch.int32, device=self.epoch.device))
            full, rows = self._batches[B]
            smp = full if n == B else RolloutBufferSamples(*(x[:n] for x in full))
            self._structs[B, n] = (smp, self._batch_struct(smp, n, self.obs_pitch), rows[:n])
        return self._structs[B, n]

    def _check_out(self, out, n):
        """Validate a caller's six output tensors for a minibatch of n rows -> (samples, row pitch)."""
        import torch
        if len(out) != 6:
            raise ValueError("out must be the 6 tensors of RolloutBufferSamples")
        smp = RolloutBufferSamples(*out)
        shapes = ((n, self.obs_dim), (n, self.action_dim), (n,), (n,), (n,), (n,))
        for what, t, shape in zip(smp._fields, smp, shapes):
            if t.dtype != torch.float32 or t.device != self.epoch.device or tuple(t.shape) != shape:
                raise ValueError(f"out.{what} must be {shape} float32 on {self.epoch.device} "
                                 f"(buffer: {self._shape()})")
        if not all(t.is_contiguous() for t in smp[1:]):
            raise ValueError("out." + " / ".join(smp._fields[1:]) + " must be contiguous")
        o = smp.observations
        pitch = self.obs_dim if n == 1 else o.stride(0)
        if o.stride(1) != 1 or pitch < self.obs_dim:
            raise ValueError("out.observations needs unit column stride and a row stride >= obs_dim")
        return smp, pitch

    @staticmethod
    def _batch_struct(smp, n, pitch):
        return nat.RolloutBatchPtrs(*(t.data_ptr() for t in smp), n, pitch)

    def minibatch(self, k, batch_size, out=None):
        """Minibatch ``k`` of the current epoch: positions ``k * batch_size ..`` of the epoch's
        permutation, drawn and gathered in one launch (finenv_rollout_minibatch).  Returns a
        ``RolloutBufferSamples`` of persistent tensors per batch size (overwritten by the next call of
        that size) or of ``out``, the caller's six tensors in the same order.  The last minibatch of
        an epoch holds ``M - k * batch_size`` rows (M = n_steps * num_envs): views of the leading rows
        of the persistent outputs, or ``out`` tensors of that many rows.  ``buf.last_rows`` is the
        int32 [B] block of flat rows ``t * E + e`` the kernel drew.  ``k`` and ``batch_size`` are
        by-value launch arguments; the epoch number is read from the device word at each replay."""
        import torch
        M = self.n_steps * self.num_envs
        B, k = int(batch_size), int(k)
        if self.epoch.device.type != "cuda":
            raise nat.FinenvError("finrl_amd has no CPU path: the buffer must live on a HIP GPU")
        if not 1 <= M < 2 ** 31:
            raise ValueError(f"minibatch: needs 1 <= n_steps * num_envs < 2**31 ({self._shape()})")
        if not 1 <= B <= M:
            raise ValueError(f"minibatch: batch_size must be in [1, {M}] ({self._shape()})")
        if not 0 <= k * B < M:
            raise ValueError(f"minibatch: k must be in [0, {-(-M // B)}) at batch_size {B} ({self._shape()})")
        first, n = k * B, min(B, M - k * B)
        if out is None:
            smp, bs, rows = self._persistent(B, n)
        else:
            smp, pitch = self._check_out(out, n)
            bs, rows = self._batch_struct(smp, n, pitch), torch.empty(n, dtype=torch.int32,
                                                                      device=self.epoch.device)
        if self._view is None:
            self._lib = nat.lib()
            self._view = nat.RolloutViewPtrs(
                self._obs_buf.data_ptr(), self.actions.data_ptr(), self.values.data_ptr(),
                self.log_probs.data_ptr(), self.advantages.data_ptr(), self.returns.data_ptr(),
                self.n_steps, self.num_envs, self.obs_dim, self.obs_pitch, self.action_dim, 0)
        stream = C.c_void_p(torch.cuda.current_stream(self.epoch.device).cuda_stream)
        rc = self._lib.finenv_rollout_minibatch(
            C.byref(self._view), C.c_void_p(self.epoch.data_ptr()), self.seed, first, C.byref(bs),
            C.c_void_p(rows.data_ptr()), stream)
        if rc:
            nat.check(rc, None, "finenv_rollout_minibatch")
        self.last_rows = rows
        return smp

    def next_epoch(self):
        """Bump the epoch word in-stream and its host mirror: the next minibatches come from a fresh
        permutation."""
        self.epoch.add_(1)
        self.epochs += 1

    def get(self, batch_size=None):
        """Generator over one epoch of minibatches (SB3's ``RolloutBuffer.get``), the last one short
        when ``batch_size`` does not divide the row count; it ends by calling ``next_epoch()`` (a
        generator abandoned before its end does not).  ``None``: a single batch of all rows, A2C's
        use.  The samples are the persistent tensors of ``minibatch``: consume each before the next."""
        M = self.n_steps * self.num_envs
        B = M if batch_size is None else int(batch_size)
        if not 1 <= B <= M:
            raise ValueError(f"get: batch_size must be in [1, {M}] ({self._shape()})")
        for k in range(-(-M // B)):
            yield self.minibatch(k, B)
        self.next_epoch()
