"""Host plumbing shared by the batched envs: one handle of the C ABI's ``finenv_<kind>_*`` family,
the ``[field][E]`` state blocks bound to it, and the reset / step launches.

A subclass names its kind, its ctypes structs and its state layout, then calls ``_open``,
``_alloc_state``, ``_bind`` and ``_alloc_outputs`` from its constructor.  All arithmetic is in
finrl_amd/csrc; this module only owns the torch tensors and hands their pointers over.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as nat


def _torch():
    import torch
    return torch


def obs_pitch_for(D, obs_pitch):
    """Row pitch (floats) of an observation buffer: "aligned" (the default, or FINENV_OBS_PITCH)
    starts every row on a 64-byte boundary (D rounded up to 16 floats); "packed" is D; an int is
    taken as given.  Packed rows of 4*D bytes share their first and last 64-byte segment with a
    neighbour row written microseconds apart -- two partial HBM writes instead of one (DESIGN.md
    4.1).  Values and shape are the reference's; only the row stride differs (obs.stride(0))."""
    if obs_pitch is None:
        obs_pitch = os.environ.get("FINENV_OBS_PITCH", "aligned")
    if obs_pitch == "aligned":
        return (D + 15) // 16 * 16
    if obs_pitch == "packed":
        return D
    pitch = int(obs_pitch)
    if pitch < D:
        raise ValueError("obs_pitch must be >= the observation dimension")
    return pitch


def _checked_out_pitch(out, obs, reward, done):
    """Validate step(out=(obs, reward, done)) against the env's own output tensors and return the row
    pitch (floats) of out[0].  The kernel writes float32 rows of D columns `pitch` floats apart."""
    o, r, d = out
    E, D = obs.shape
    for t, ref, what in ((o, obs, "out[0]"), (r, reward, "out[1]"), (d, done, "out[2]")):
        if t.dtype != ref.dtype or t.device != ref.device or tuple(t.shape) != tuple(ref.shape):
            raise ValueError(f"{what} must be {tuple(ref.shape)} {ref.dtype} on {ref.device}")
    if o.stride(-1) != 1 or not r.is_contiguous() or not d.is_contiguous():
        raise ValueError("out[0] needs unit column stride; out[1] / out[2] must be contiguous")
    if E == 1:                  # (torch reports an arbitrary row stride for a single row)
        return D
    if o.stride(0) < D:
        raise ValueError("out[0]: rows overlap (row stride smaller than the observation dimension)")
    return o.stride(0)


class BatchedEnv:
    """Base of the batched envs.  Class attributes of a subclass:

    ``_kind``: the ``finenv_<kind>_*`` family; ``_panel_cls`` / ``_state_cls``: its ctypes
    pointer structs; ``_layout``: ``{"f64" | "i32" | "f32": (fields, books)}``, the rows of each
    state block -- one per field, then N per book ([N][E], viewed as ``state[book]`` and transposed
    to [E, N] by ``state_numpy``); ``_step_extras``: the optional step outputs after ``done``, in
    the order ``finenv_<kind>_step`` takes them; ``_pitched``: obs rows have a settable pitch
    (``finenv_<kind>_set_obs_pitch``) and ``step(out=...)`` is validated."""

    _kind = ""
    _panel_cls = _state_cls = None
    _layout = {}
    _step_extras = ("term_obs",)
    _pitched = False
    _h = None
    _f64 = _i32 = _f32 = None
    _step_args = None           # (step function, output pointers): see step()

    # ------------------------------------------------------------------ construction
    def _set_device(self, device):
        self.device = _torch().device(device)
        if self.device.type != "cuda":
            raise nat.FinenvError("finrl_amd has no CPU path: device must be a HIP GPU")

    def _fn(self, name):
        return getattr(nat.lib(), f"finenv_{self._kind}_{name}")

    def _call(self, name, *args, what=None):
        """finenv_<kind>_<name>(handle, *args), raising FinenvError with the handle's last error."""
        nat.check(self._fn(name)(self._h, *args), self._h, what or name, self._kind)

    def _open(self, cfg):
        """Create the handle for ``cfg`` (the kind's ctypes config struct)."""
        self._cfg = cfg
        self._h = C.c_void_p()
        nat.check(self._fn("create")(C.byref(cfg), C.byref(self._h)), None,
                  f"finenv_{self._kind}_create")

    def _alloc_state(self, E, N):
        """Zeroed ``_f64`` / ``_i32`` / ``_f32`` blocks per ``_layout`` (None where it has none) and
        their named views in ``self.state``: every block's fields, then every block's books."""
        torch = _torch()
        self.state, books = {}, {}
        for name, dtype in (("f64", torch.float64), ("i32", torch.int32), ("f32", torch.float32)):
            if name not in self._layout:
                continue
            fields, bk = self._layout[name]
            t = torch.zeros(len(fields) + len(bk) * N, E, dtype=dtype, device=self.device)
            setattr(self, "_" + name, t)
            self.state.update({k: t[j] for j, k in enumerate(fields)})
            books.update({k: t[len(fields) + b * N:len(fields) + (b + 1) * N] for b, k in enumerate(bk)})
        self.state.update(books)
        self._books = tuple(books)

    def _bind(self, *panel):
        """Bind the panel's device tensors (in ``_panel_cls`` order) and the state blocks."""
        pp = self._panel_cls(*(t.data_ptr() for t in panel))
        sp = self._state_cls(*(t.data_ptr() for t in (self._f64, self._i32, self._f32) if t is not None))
        self._call("bind", C.byref(pp), C.byref(sp))

    def _alloc_outputs(self, E, D, obs_pitch=None):
        """The persistent step outputs: obs [E, D] f32 (pitched envs: a view of ``_obs_buf``, rows
        ``obs_pitch_for(D, obs_pitch)`` floats apart), reward [E] f32, done [E] u8; the optional
        ones (``_step_extras``) stay None until enabled."""
        torch = _torch()
        if self._pitched:
            pitch = obs_pitch_for(D, obs_pitch)
            self._obs_buf = torch.zeros(E, pitch, dtype=torch.float32, device=self.device)
            self.obs = self._obs_buf[:, :D]
            self._pitch = self._pitch_set = pitch
            self._call("set_obs_pitch", pitch)
        else:
            self.obs = torch.zeros(E, D, dtype=torch.float32, device=self.device)
        self.reward = torch.zeros(E, dtype=torch.float32, device=self.device)
        self.done = torch.zeros(E, dtype=torch.uint8, device=self.device)
        for name in self._step_extras:
            setattr(self, name, None)

    def _enable_output(self, name, cols, dtype):
        """Allocate the optional step output ``name`` ([E, cols]) once; step() then passes it."""
        if getattr(self, name) is None:
            setattr(self, name, _torch().zeros(self.num_envs, cols, dtype=dtype, device=self.device))
            self._step_args = None
        return getattr(self, name)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def _use_pitch(self, pitch):
        if pitch != self._pitch_set:
            self._call("set_obs_pitch", int(pitch))
            self._pitch_set = pitch

    def _actions(self, actions):
        """actions as the kernel reads them: contiguous float32 [E, action_dim] on the env's device."""
        torch = _torch()
        if actions.dtype != torch.float32 or not actions.is_contiguous() or \
                actions.device != self.obs.device or \
                tuple(actions.shape) != (self.num_envs, self.action_dim):
            actions = actions.to(device=self.device, dtype=torch.float32).reshape(
                self.num_envs, self.action_dim).contiguous()
        return actions

    def enable_terminal_obs(self):
        return self._enable_output("term_obs", self.obs.shape[1], _torch().float32)

    # ------------------------------------------------------------------ env protocol
    def _before_reset(self):
        """Hook: runs before every reset launch."""

    def reset(self, mask=None):
        """Reset every env (or those with mask[e] != 0) -> obs [E, D] f32 (device)."""
        self._before_reset()
        mptr = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=_torch().uint8).contiguous()
            mptr = C.c_void_p(mask.data_ptr())
        if self._pitched:
            self._use_pitch(self._pitch)
        self._call("reset", mptr, C.c_void_p(self.obs.data_ptr()), self._stream())
        return self.obs

    def step(self, actions, out=None):
        """One step of every env, asynchronously on the current stream.

        actions: float32 [E, action_dim] device tensor.  Returns (obs, reward, done, None), views
        of persistent device tensors that the next call overwrites (clone them to keep); no host
        synchronisation happens here.  out = (obs [E, D] f32, reward [E] f32, done [E] u8): write
        there instead (rollout buffers: the kernel writes straight into slice t, no staging copy).
        """
        actions = self._actions(actions)
        # the step function and the pointers of the persistent outputs are cached (the Python side
        # of a launch is most of what a step call costs on the host); an enable_* drops the cache
        if self._step_args is None:
            self._step_args = (self._fn("step"), tuple(
                None if t is None else C.c_void_p(t.data_ptr()) for t in
                (self.obs, self.reward, self.done) + tuple(getattr(self, n) for n in self._step_extras)))
        fn, outs = self._step_args
        ret = (self.obs, self.reward, self.done)
        if out is not None:
            ret = out
            if self._pitched:
                self._use_pitch(_checked_out_pitch(out, self.obs, self.reward, self.done))
            outs = tuple(C.c_void_p(t.data_ptr()) for t in out) + outs[3:]
        elif self._pitched and self._pitch_set != self._pitch:
            self._use_pitch(self._pitch)
        rc = fn(self._h, C.c_void_p(actions.data_ptr()), *outs, int(self.auto_reset), self._stream())
        if rc:
            nat.check(rc, self._h, "step", self._kind)
        return ret[0], ret[1], ret[2], None

    def as_sb3_vec_env(self):
        """stable-baselines3 VecEnv-shaped view (numpy in / out, auto-reset, terminal_observation)."""
        from .vec_env import SB3VecEnvAdapter
        return SB3VecEnvAdapter(self)

    def state_numpy(self):
        """Host copy of the per-env state (synchronises); books as [E, N]."""
        out = {k: v.detach().cpu().numpy() for k, v in self.state.items()}
        for k in self._books:
            out[k] = np.ascontiguousarray(out[k].T)
        return out


class WindowedEnv(BatchedEnv):
    """Per-env episode windows over one shared panel: the host side of ``finenv_<kind>_set_windows``,
    shared by VecStockTradingEnv, VecStockPortfolioEnv, VecCryptoEnv, VecStockTradingEnvNP,
    VecCashPenaltyEnv and VecStopLossEnv (``num_envs`` and ``max_step`` are theirs).  What differs
    between the kinds is named by hooks:
    ``_window_rows`` (the panel's row count), ``_window_min`` (the shortest window that makes an
    episode), ``_window_max_step`` (``max_step`` of the longest window), ``_window_active`` (the
    kernel keeps the running episodes' windows apart from the pending ones) and
    ``_new_window_block`` (the device block the kernel reads; ``self.windows`` is its [2, E]
    start / end view)."""

    windows = None
    active_windows = None       # _window_active kinds: the running episodes' windows, kernel-owned
    _window_min = 1
    _window_active = False

    @property
    def _window_rows(self):
        return self.panel.T

    def _window_max_step(self, longest):
        return longest - 1

    def _new_window_block(self):
        """Allocate the block the kernel reads -> its [2, E] view of starts and ends, every env on
        the whole panel.  ``_window_active`` kinds: int32 [4, E], rows 0, 1 the pending windows
        (``self.windows``, what the caller edits), rows 2, 3 the active ones
        (``self.active_windows``, kernel-owned); both start on the whole panel, which is what an
        env without windows is running."""
        torch = _torch()
        block = torch.zeros(4 if self._window_active else 2, self.num_envs, dtype=torch.int32,
                            device=self.device)
        block[1::2].fill_(self._window_rows)
        if self._window_active:
            self.active_windows = block[2:]
        return block[:2]

    def _attach_windows(self, ptr):
        self._call("set_windows", ptr)

    def _check_window_starts(self, start):
        """Hook: kind-specific host validation of the start rows (int64 [E])."""

    def _check_windows(self, start, end):
        """Host validation of (start, end) -> two int64 [E] arrays (ValueError when a window is too
        short to make an episode or leaves the panel)."""
        torch = _torch()
        E, T = self.num_envs, self._window_rows
        out = []
        for x, what in ((start, "start"), (end, "end")):
            if torch.is_tensor(x):
                x = x.detach().cpu().numpy()
            a = np.asarray(x)
            if a.dtype.kind not in "iu":
                raise ValueError(f"windows: {what} must be integer panel rows")
            try:
                out.append(np.broadcast_to(a.astype(np.int64), (E,)))
            except ValueError:
                raise ValueError(f"windows: {what} must be one value or [{E}] values") from None
        s, t = out
        if (s < 0).any() or (t > T).any():
            raise ValueError(f"windows must lie in [0, {T}] (the panel's rows)")
        if (t <= s).any():
            raise ValueError("windows must not be empty (start < end)")
        if (t - s < self._window_min).any():
            raise ValueError(f"windows must span at least {self._window_min} panel rows")
        self._check_window_starts(s)
        return s, t

    def set_windows(self, start, end=None, mask=None):
        """Per-env episode windows [start, end) of panel rows (finenv_<kind>_set_windows);
        ``set_windows(None)`` detaches them (every env runs the whole panel again).

        The windows live in ``self.windows``, an int32 [2, E] device tensor (row 0 starts, row 1
        ends) whose address the step kernel takes as an argument; this call copies into it in place.
        The stock and portfolio step kernels read an env's END on every step and its START only when
        they reset the env, so an edited end applies from the next step and an edited start at the
        env's next reset (auto-reset or ``reset()``); nothing moves an env that is mid-episode.  To
        start the envs that just finished on new windows: ``set_windows(s, t, mask=done)`` then
        ``reset(done)``.  (VecCryptoEnv takes both at the env's next reset: see
        its own ``set_windows``.)

        Host values (ints, arrays) are validated (ValueError on empty or out-of-range windows).
        Device tensors are copied without a host synchronisation, so windows can be redrawn with
        torch ops -- ``mask`` (bool [E]) limits the update to those envs, e.g. the ones that just
        reported ``done`` -- even inside a captured graph (the graph sees the block's contents as
        they are at each replay).  Those are NOT validated: the kernel clamps every window into
        the panel, so a bad one gives wrong results, never a fault.  Attach windows before capturing
        a graph: a graph keeps the pointer it was captured with.  ``max_step`` follows the windows
        passed here (that of the longest), except device tensors passed during a capture."""
        torch = _torch()
        if start is None:
            self._attach_windows(None)
            self.windows = self.active_windows = None
            self.max_step = self._window_max_step(self._window_rows)
            return None
        if end is None:
            raise ValueError("set_windows needs start and end")
        on_device = all(torch.is_tensor(x) and x.device.type == "cuda" for x in (start, end))
        if self.windows is None:
            self.windows = self._new_window_block()
        new = torch.empty_like(self.windows)
        if on_device:
            new[0].copy_(start.to(device=self.device, dtype=torch.int32).expand(self.num_envs))
            new[1].copy_(end.to(device=self.device, dtype=torch.int32).expand(self.num_envs))
        else:
            s_np, t_np = self._check_windows(start, end)
            new.copy_(torch.from_numpy(np.stack([s_np, t_np]).astype(np.int32)))
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.bool) if torch.is_tensor(mask) else \
                torch.from_numpy(np.asarray(mask, dtype=bool)).to(self.device)
            new = torch.where(m, new, self.windows)
        self.windows.copy_(new)
        self._attach_windows(C.c_void_p(self.windows.data_ptr()))
        if not (on_device and torch.cuda.is_current_stream_capturing()):
            self.max_step = self._window_max_step(
                int((self.windows[1] - self.windows[0]).max().item()))
        return self.windows
