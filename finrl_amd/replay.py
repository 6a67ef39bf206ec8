"""Device-resident replay buffer for the off-policy agents (DDPG / TD3 / SAC): a ring the env
kernels fill through ``step(out=...)`` without a copy, and a one-launch sampler that draws
(slot, env) pairs and gathers the batch (finenv_replay_* in include/finenv.h)."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from . import _native as nat
from .vec_base import obs_pitch_for

# stable-baselines3's ReplayBufferSamples: the same field order and shapes
ReplayBufferSamples = namedtuple(
    "ReplayBufferSamples", ("observations", "actions", "next_observations", "dones", "rewards"))
# the n-step batch: the same five, then the bootstrap discount gamma^m [B, 1]
NStepReplayBufferSamples = namedtuple(
    "NStepReplayBufferSamples", ReplayBufferSamples._fields + ("discounts",))
# the prioritised batches: the same, then the probability each transition was drawn with [B, 1]
PrioritizedReplayBufferSamples = namedtuple(
    "PrioritizedReplayBufferSamples", ReplayBufferSamples._fields + ("probabilities",))
PrioritizedNStepReplayBufferSamples = namedtuple(
    "PrioritizedNStepReplayBufferSamples", NStepReplayBufferSamples._fields + ("probabilities",))


class ReplayBuffer:
    """Ring of ``n_slots`` time steps of ``num_envs`` envs on the env's device, in the layout of SB3's
    ``ReplayBuffer(optimize_memory_usage=True, handle_timeout_termination=False)``: ``obs[s]`` is what
    the policy saw before the step stored in slot ``s`` and its next observation is
    ``obs[(s + 1) % n_slots]``, so every observation is stored once.

    ``obs_pitch`` is the env's: ``None`` / "aligned" / an int for the pitched envs
    (VecStockTradingEnv, VecStockTradingEnvNP: rows ``obs_pitch_for(obs_dim, obs_pitch)`` floats
    apart), "packed" for every other env, whose kernels write packed rows.

    Under the envs' in-kernel auto-reset the next observation of a ``done`` transition is the first
    observation of the next episode (what SB3 stores in that mode); the TD target masks it with
    ``1 - dones``.

    After ``n`` steps ``len(buf) = min(n, n_slots - 1)`` slots hold a complete transition: the slots
    ``(pos - 1 - j) % n_slots``, ``j < len(buf)``.  Slot ``pos`` of a full ring is not among them --
    its observation has been overwritten by the newest next observation.

    ``head`` (int32 [2] = pos, n_valid) and ``draw`` (int64 [1]) are the device words the sampler
    reads; ``pos``, ``len(buf)`` and ``draws`` mirror them on the host.  ``step`` SETS the head to the
    values of the host mirror, so a replayed capture of ``step`` publishes the head that belongs to
    the slots it writes, and a captured ``sample`` sees ring and draw number as they are at each
    replay (the host mirror does not follow replays).

    ``sample_nstep`` / ``gather_nstep`` return n-step batches (discounted reward sum, the observation
    m steps later, ``gamma^m``) from the same ring, head and draw, also in one launch."""

    _drawn_kinds = (ReplayBufferSamples, NStepReplayBufferSamples)     # what sample / sample_nstep return

    def __init__(self, n_slots, num_envs, obs_dim, action_dim, obs_pitch=None, device="cuda", seed=0):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise nat.FinenvError("finrl_amd has no CPU path: device must be a HIP GPU")
        S, E, D, A = int(n_slots), int(num_envs), int(obs_dim), int(action_dim)
        if S < 2 or E < 1 or D < 1 or A < 1:
            raise ValueError("ReplayBuffer needs n_slots >= 2 and num_envs, obs_dim, action_dim >= 1")
        P = obs_pitch_for(D, obs_pitch)
        self.n_slots, self.num_envs, self.obs_dim, self.action_dim, self.obs_pitch = S, E, D, A, P
        self.device, self.seed = dev, int(seed) & (2 ** 64 - 1)
        self._obs_buf = torch.zeros(S, E, P, dtype=torch.float32, device=dev)
        self.obs = self._obs_buf[:, :, :D]
        self.actions = torch.zeros(S, E, A, dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(S, E, dtype=torch.float32, device=dev)
        self.dones = torch.zeros(S, E, dtype=torch.uint8, device=dev)
        self.head = torch.zeros(2, dtype=torch.int32, device=dev)
        self.draw = torch.zeros(1, dtype=torch.int64, device=dev)
        self.pos = self._n_valid = self.draws = 0
        self.last_indices = None
        self.last_steps = None      # int32 [B]: the lengths m of the last n-step batch
        self._view = nat.ReplayViewPtrs(self._obs_buf.data_ptr(), self.actions.data_ptr(),
                                        self.rewards.data_ptr(), self.dones.data_ptr(), S, E, D, P, A, 0)
        self._batches = {}          # (namedtuple, batch size) -> (samples, ctypes struct, indices, steps)
        self._slots = {}            # pos -> (actions[pos], the env's out tuple of that slot)
        self._lib = nat.lib()

    def __len__(self):
        return self._n_valid

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ filling
    def start(self, env, first_obs):
        """Begin collecting: the reset observation goes to ``obs[pos]`` (slot 0 of a fresh buffer)."""
        self.obs[self.pos].copy_(first_obs)
        return self.obs[self.pos]

    def step(self, env, actions):
        """Store ``actions`` [E, A] in slot ``pos`` and publish the head after this step (one launch,
        finenv_replay_put), then step the env from that slot straight into the ring:
        obs -> ``obs[(pos + 1) % S]``, reward and done -> slot ``pos``.  Returns the env's tuple."""
        import torch
        if not env.auto_reset:
            raise ValueError("ReplayBuffer.step needs env.auto_reset: a masked reset() writes into "
                             "the env's own output, not into the ring")
        S, E, A = self.n_slots, self.num_envs, self.action_dim
        if not getattr(env, "_pitched", False) and self.obs_pitch != self.obs_dim:
            raise ValueError(f"{type(env).__name__} writes packed observation rows: build the "
                             "ReplayBuffer with obs_pitch=\"packed\"")
        a = actions.to(self.device, torch.float32).contiguous()
        if a.numel() != E * A:
            raise ValueError(f"step: expected actions [{E}, {A}]")
        pos, nxt = self.pos, (self.pos + 1) % S
        n_valid = min(self._n_valid + 1, S - 1)
        if pos not in self._slots:      # the slot's views, made once: slicing is host time per step
            self._slots[pos] = (self.actions[pos], (self.obs[nxt], self.rewards[pos], self.dones[pos]))
        slot, out = self._slots[pos]
        rc = self._lib.finenv_replay_put(
            C.c_void_p(a.data_ptr()), C.c_void_p(slot.data_ptr()), E * A,
            C.c_void_p(self.head.data_ptr()), nxt, n_valid, self._stream())
        if rc:
            nat.check(rc, None, "finenv_replay_put")
        ret = env.step(slot, out=out)
        self.pos, self._n_valid = nxt, n_valid
        return ret

    # ------------------------------------------------------------------ sampling
    def _batch(self, B, out, kind=ReplayBufferSamples):
        """(samples, finenv_replay_batch, index block, steps block or None) of batch size B as the
        namedtuple ``kind``: the persistent outputs of that kind, or ``out`` (its tensors in order) with
        a fresh steps block (n-step kinds) and no index block (a drawn call makes its own)."""
        import torch
        D, A = self.obs_dim, self.action_dim
        nstep = "discounts" in kind._fields
        i32 = dict(dtype=torch.int32, device=self.device)
        if out is None:
            if (kind, B) not in self._batches:
                kw = dict(dtype=torch.float32, device=self.device)
                o, n = (torch.zeros(B, self.obs_pitch, **kw) for _ in range(2))
                smp = kind(o[:, :D], torch.zeros(B, A, **kw), n[:, :D],
                           *(torch.zeros(B, 1, **kw) for _ in kind._fields[3:]))
                self._batches[kind, B] = (smp, self._batch_struct(smp, B, self.obs_pitch),
                                          torch.zeros(2, B, **i32),
                                          torch.zeros(B, **i32) if nstep else None)
            return self._batches[kind, B]
        if kind is not ReplayBufferSamples and len(out) != len(kind._fields):
            raise ValueError(f"out must be the {len(kind._fields)} tensors of {kind.__name__}")
        smp = kind(*out)
        pitch = self._check_out(smp, B)
        return smp, self._batch_struct(smp, B, pitch), None, torch.empty(B, **i32) if nstep else None

    def _check_out(self, smp, B):
        """Validate a caller's output tuple (either namedtuple) -> the common observation row pitch."""
        import torch
        D, A = self.obs_dim, self.action_dim
        fields = [(smp.observations, (B, D), "observations"), (smp.actions, (B, A), "actions"),
                  (smp.next_observations, (B, D), "next_observations"),
                  (smp.dones, (B, 1), "dones"), (smp.rewards, (B, 1), "rewards")]
        for what in smp._fields[5:]:                 # discounts, probabilities
            fields.append((getattr(smp, what), (B, 1), what))
        for t, shape, what in fields:
            if t.dtype != torch.float32 or t.device != self.head.device or tuple(t.shape) != shape:
                raise ValueError(f"out.{what} must be {shape} float32 on {self.head.device}")
        o, n = smp.observations, smp.next_observations
        if not all(t.is_contiguous() for t, _, what in fields[1:] if what != "next_observations"):
            raise ValueError("out." + " / ".join(("actions", "dones", "rewards") + smp._fields[5:]) +
                             " must be contiguous")
        pitch = D if B == 1 else o.stride(0)
        if o.stride(1) != 1 or n.stride(1) != 1 or pitch < D or (B > 1 and n.stride(0) != pitch):
            raise ValueError("out.observations / next_observations need unit column stride and one "
                             "common row stride >= obs_dim")
        return pitch

    @staticmethod
    def _batch_struct(smp, B, pitch):
        return nat.ReplayBatchPtrs(smp.observations.data_ptr(), smp.next_observations.data_ptr(),
                                   smp.actions.data_ptr(), smp.rewards.data_ptr(), smp.dones.data_ptr(),
                                   B, pitch)

    def sample(self, batch_size, out=None):
        """Draw ``batch_size`` transitions uniformly from the valid slots x envs and gather them: one
        launch (finenv_replay_sample), plus the in-stream bump of the draw word.  Returns a
        ``ReplayBufferSamples`` of persistent tensors per batch size (overwritten by the next call
        of that size) or of ``out``, the caller's five tensors in the same order;
        ``buf.last_indices`` is the int32 [2, B] block of (slots, envs) the kernel drew.  The draw is
        a pure function of (seed, draw number, ring head): Philox4x32-10, include/finenv.h."""
        return self._drawn("sample", batch_size, out)

    def _drawn(self, name, batch_size, out, nstep=None):
        """The drawn call ``name`` (``nstep``: the (n_steps, gamma) of the n-step form): its checks, the
        launch finenv_replay_<name>, the bump of the draw word, ``last_indices`` / ``last_steps``."""
        if self._n_valid == 0:
            raise ValueError(f"{name}: the buffer holds no complete transition yet")
        B = int(batch_size)
        if B < 1:
            raise ValueError(f"{name}: batch_size must be >= 1")
        smp, bs, idx, steps = self._batch(B, out, self._drawn_kinds[nstep is not None])
        if idx is None:
            import torch
            idx = torch.empty(2, B, dtype=torch.int32, device=self.device)
        ns = () if nstep is None else (C.byref(self._nstep_struct(smp, steps, *nstep)),)
        self._launch_drawn(name, smp, bs, ns, idx)
        self.draw.add_(1)
        self.draws += 1
        self.last_indices = idx
        if nstep is not None:
            self.last_steps = steps
        return smp

    def _launch_drawn(self, name, smp, bs, ns, idx):
        """The launch of the drawn call ``name`` into ``smp``: the uniform draw from the head words."""
        fn = "finenv_replay_" + name
        nat.check(getattr(self._lib, fn)(
            C.byref(self._view), C.c_void_p(self.head.data_ptr()), C.c_void_p(self.draw.data_ptr()),
            self.seed, C.byref(bs), *ns, C.c_void_p(idx.data_ptr()), self._stream()), None, fn)

    def _index_block(self, name, indices):
        """The caller's ``indices`` of ``name`` as the contiguous int32 [2, B] block the kernel reads."""
        import torch
        idx = indices.to(device=self.device, dtype=torch.int32).contiguous()
        if idx.dim() != 2 or idx.shape[0] != 2 or idx.shape[1] < 1:
            raise ValueError(f"{name}: indices must be [2, B]")
        return idx

    def gather(self, indices, out=None):
        """The batch of caller-chosen transitions: ``indices`` int [2, B] on the device (row 0 slots,
        row 1 envs), clamped into the ring by the kernel.  One launch (finenv_replay_gather)."""
        return self._indexed("gather", indices, out)

    def _indexed(self, name, indices, out, nstep=None):
        """``name`` on the caller's ``indices`` (``nstep`` as in ``_drawn``): the launch and ``last_steps``."""
        idx = self._index_block(name, indices)
        smp, bs, _, steps = self._batch(int(idx.shape[1]), out, ReplayBuffer._drawn_kinds[nstep is not None])
        ns = () if nstep is None else (C.byref(self._nstep_struct(smp, steps, *nstep)),)
        fn = "finenv_replay_" + name
        nat.check(getattr(self._lib, fn)(
            C.byref(self._view), C.c_void_p(idx.data_ptr()), C.byref(bs), *ns, self._stream()), None, fn)
        if nstep is not None:
            self.last_steps = steps
        return smp

    # ------------------------------------------------------------------ n-step returns
    def _nstep_struct(self, smp, steps, n_steps, gamma):
        n, g = int(n_steps), float(gamma)
        if not 1 <= n <= self.n_slots - 1:
            raise ValueError(f"n_steps must be in [1, n_slots - 1 = {self.n_slots - 1}]")
        if not 0.0 <= g <= 1.0:                  # refuses NaN too
            raise ValueError("gamma must be in [0, 1]")
        return nat.ReplayNStepPtrs(self.head.data_ptr(), smp.discounts.data_ptr(), steps.data_ptr(),
                                   n, g)

    def sample_nstep(self, batch_size, n_steps, gamma, out=None):
        """``sample`` with n-step returns, in one launch (finenv_replay_sample_nstep) plus the
        in-stream bump of the draw word.  The pairs are the ones ``sample`` draws for the same seed,
        draw number and head.  From each start (s, e) the kernel walks up to ``n_steps`` stored steps
        forward, stopping after the first ``done`` or at the ring's newest step (a start close to the
        head yields a shorter return; it is not excluded): with m the steps taken,
        ``rewards = sum_{i<m} gamma^i r_i`` (float32 powers, float64 sum), ``dones`` is that of the
        last step, ``next_observations`` the observation m steps later and ``discounts = gamma^m``,
        so the TD target is ``rewards + (1 - dones) * discounts * Q'(next_observations)``.  Returns an
        ``NStepReplayBufferSamples`` of persistent tensors per batch size (separate from those of
        ``sample``) or of ``out``, the caller's six tensors; ``buf.last_indices`` is as for
        ``sample`` and ``buf.last_steps`` (int32 [B]) holds m.  ``n_steps`` and ``gamma`` are
        by-value launch arguments: a captured call keeps the values it was captured with, while
        ring, head and draw number are read at each replay."""
        return self._drawn("sample_nstep", batch_size, out, (n_steps, gamma))

    def gather_nstep(self, indices, n_steps, gamma, out=None):
        """The n-step batch of caller-chosen starts: ``indices`` as for ``gather`` (clamped into the
        ring by the kernel; whether a slot is a valid start is the caller's business), the rule of
        ``sample_nstep`` with the horizon measured from the device head.  One launch
        (finenv_replay_gather_nstep); ``buf.last_steps`` holds m.  ``n_steps`` and ``gamma`` are
        by-value launch arguments, as in ``sample_nstep``."""
        return self._indexed("gather_nstep", indices, out, (n_steps, gamma))


class PrioritizedReplayBuffer(ReplayBuffer):
    """``ReplayBuffer`` with proportional prioritised replay on the device (include/finenv.h,
    "Prioritised replay"): one uint32 fixed-point *ticket* per transition beside the ring
    (``tickets`` int32 [S, E] holding the bit pattern), a fan-out-64 tree of exact uint64 sums
    (``tree`` int64 [words], ``tree[0]`` the total) and ``max_ticket`` (int32 [1]), the largest ticket
    seen, at which new transitions enter.  A ticket of 0 means the slot holds no complete transition,
    so the draw needs no head word; every stored transition keeps a ticket >= 1.

    ``sample`` / ``sample_nstep`` draw transition i with probability ticket_i / total, in the
    sampler's one launch, and return the parent's fields plus ``probabilities`` [B, 1];
    ``update_priorities`` writes TD errors back.  The shaped priority is ``(|p| + eps) ** alpha``,
    computed in torch (``powf`` is not bit-reproducible; the kernels are integer and exact), stored as
    ``rint(w * 2**frac_bits)`` clamped to [1, 2**32 - 1]: a priority below ``2**-frac_bits`` draws as
    if it were ``2**-frac_bits``.  ``gather`` / ``gather_nstep`` are the parent's."""

    _drawn_kinds = (PrioritizedReplayBufferSamples, PrioritizedNStepReplayBufferSamples)

    def __init__(self, n_slots, num_envs, obs_dim, action_dim, obs_pitch=None, device="cuda", seed=0,
                 alpha=0.6, eps=1e-6, frac_bits=16):
        import torch
        super().__init__(n_slots, num_envs, obs_dim, action_dim, obs_pitch, device, seed)
        F = int(frac_bits)
        if not 0 <= F <= 31:
            raise ValueError("frac_bits must be in [0, 31]")
        S, E = self.n_slots, self.num_envs
        words = int(self._lib.finenv_replay_per_tree_words(S * E))
        if words < 1:
            raise ValueError("PrioritizedReplayBuffer needs n_slots * num_envs <= 2**31 - 1")
        self.alpha, self.eps, self.frac_bits = float(alpha), float(eps), F
        self.tickets = torch.zeros(S, E, dtype=torch.int32, device=self.device)
        self.tree = torch.zeros(words, dtype=torch.int64, device=self.device)
        one = 1 << F                                              # the ticket of 1.0
        self.max_ticket = torch.tensor([one - (1 << 32) if one >= 1 << 31 else one],
                                       dtype=torch.int32, device=self.device)
        self._per = nat.ReplayPerPtrs(self.tickets.data_ptr(), self.tree.data_ptr(),
                                      self.max_ticket.data_ptr(), F, 0)

    @property
    def total(self):
        """The sum of all tickets (``tree[0]``; reads the device)."""
        return int(self.tree[0].item()) & (2 ** 64 - 1)

    def step(self, env, actions):
        """The parent's step, plus finenv_replay_per_put: the stored slot's tickets take
        ``max_ticket``, those of the slot whose observation was just overwritten take 0, and the sums
        follow."""
        pos = self.pos
        ret = super().step(env, actions)
        nat.check(self._lib.finenv_replay_per_put(
            C.byref(self._per), self.n_slots, self.num_envs, pos, self.pos, self._stream()), None,
            "finenv_replay_per_put")
        return ret

    def _launch_drawn(self, name, smp, bs, ns, idx):
        fn = "finenv_replay_per_" + name
        nat.check(getattr(self._lib, fn)(
            C.byref(self._view), C.byref(self._per), C.c_void_p(self.draw.data_ptr()), self.seed,
            C.byref(bs), *ns, C.c_void_p(smp.probabilities.data_ptr()), C.c_void_p(idx.data_ptr()),
            self._stream()), None, fn)

    def update_priorities(self, indices, priorities, shaped=False):
        """Write priorities back for ``indices`` (int [2, B], e.g. ``buf.last_indices``):
        ``w = (priorities.abs() + eps) ** alpha`` in torch, or ``priorities`` itself with
        ``shaped=True``, then finenv_replay_per_update -- tickets, ``max_ticket`` and the sums.  An
        entry for a slot that holds no complete transition (ticket 0) is dropped.  Duplicate indices
        with different priorities leave one of them, unspecified which."""
        import torch
        idx = self._index_block("update_priorities", indices)
        p = priorities.to(self.device, torch.float32).reshape(-1)
        w = (p if shaped else (p.abs() + self.eps) ** self.alpha).contiguous()
        if w.numel() != idx.shape[1]:
            raise ValueError("update_priorities: one priority per index pair")
        nat.check(self._lib.finenv_replay_per_update(
            C.byref(self._per), self.n_slots, self.num_envs, C.c_void_p(idx.data_ptr()),
            C.c_void_p(w.data_ptr()), int(w.numel()), self._stream()), None,
            "finenv_replay_per_update")

    def importance_weights(self, probabilities, beta):
        """``(n_valid * E * P) ** -beta`` divided by its batch maximum (float32, formed in float64), in
        torch from the device head word (so it is right inside a replayed graph)."""
        import torch
        n = self.head[1].to(torch.float64) * float(self.num_envs)
        w = (n * probabilities.to(torch.float64)) ** (-float(beta))
        return (w / w.max()).to(torch.float32)

    def find(self, u):
        """The pairs (int32 [2, B]) of the leaves selected by ``u``: uint64 values as a device tensor
        of dtype uint64 or int64 (the bit pattern), taken as ``min(u, total - 1)``."""
        import torch
        u = u.to(self.device).contiguous().reshape(-1)
        if u.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or u.numel() < 1:
            raise ValueError("find: u must be a non-empty uint64 / int64 tensor")
        out = torch.empty(2, u.numel(), dtype=torch.int32, device=self.device)
        nat.check(self._lib.finenv_replay_per_find(
            C.byref(self._per), self.n_slots, self.num_envs, C.c_void_p(u.data_ptr()), int(u.numel()),
            C.c_void_p(out.data_ptr()), self._stream()), None, "finenv_replay_per_find")
        return out

    def rebuild(self):
        """Recompute every tree node from ``tickets`` as they are (after restoring them)."""
        nat.check(self._lib.finenv_replay_per_rebuild(
            C.byref(self._per), self.n_slots, self.num_envs, self._stream()), None,
            "finenv_replay_per_rebuild")
