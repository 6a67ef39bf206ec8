"""Device-resident batch of the reference's multi-crypto env
(finrl/meta/env_cryptocurrency_trading/env_multiple_crypto.py:10-111), one HIP launch per step
through the C ABI (finenv_crypto_*)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as nat
from .spaces import Box
from .vec_base import WindowedEnv


def action_norm_vector(price0):
    """_generate_action_normalizer, :103-111 (host-side, Python's own math.log / pow)."""
    out = []
    for price in np.asarray(price0, dtype=np.float64):
        x = math.floor(math.log(price, 10))
        out.append(1 / ((10) ** x))
    return np.asarray(out) * 10000


def action_norm_table(price_array):
    """``action_norm_vector`` of every row of ``price_array`` [T, N] -> f64 [T, N]: the table the
    windowed step kernel indexes by an env's window start (finenv_crypto_set_windows).  Row r
    equals ``action_norm_vector(price_array[r])`` bit for bit: the exponent is taken by the same
    ``math.floor(math.log(price, 10))`` -- NOT ``np.log10``, which floors 1000.0 to 3 where
    ``math.log(1000.0, 10)`` gives 2.9999999999999996 -- and the scale by the same Python
    expression of that exponent.  A row with a price that is not positive and finite is all NaN,
    with no exception: the reference raises on such a first row, and an env whose window starts
    there makes no trades.  T * N calls of ``math.log``: about half a second for a month of
    one-minute bars of ten pairs (43,200 x 10); built once per env."""
    price = np.asarray(price_array, dtype=np.float64)
    out = np.full(price.shape, np.nan)
    scale = {}                                  # exponent -> 1 / 10 ** x * 10000, evaluated as above
    ok = (np.isfinite(price) & (price > 0)).all(axis=1)
    for r in np.flatnonzero(ok):
        row = out[r]
        for i, p in enumerate(price[r].tolist()):
            x = math.floor(math.log(p, 10))
            v = scale.get(x)
            if v is None:
                v = scale[x] = (np.asarray([1 / ((10) ** x)]) * 10000)[0]
            row[i] = v
    return out


class VecCryptoEnv(WindowedEnv):
    """E parallel CryptoEnv.  Constructor mirrors the reference: ``config`` holds
    ``price_array`` [T,N] and ``tech_array`` [T,W] (float64).

    ``windows=(start, end)`` gives every env its own episode window of panel rows ``[start, end)``
    (one pair for all envs, or [E] arrays / tensors): env e then equals the reference env built on
    ``{'price_array': price_array[s:t], 'tech_array': tech_array[s:t]}`` -- the tutorial's train and
    test slices, or random training windows, in ONE batch over one panel -- including its action
    normaliser, which the reference derives from the first row of the array it is given.
    ``state["time"]`` stays the panel row; ``window_time()`` is the reference's ``self.time``.
    See ``set_windows``."""

    env_name = "MulticryptoEnv-MI355X"
    if_discrete = False
    target_return = 10
    _kind = "crypto"
    _panel_cls, _state_cls = nat.CryptoPanelPtrs, nat.CryptoStatePtrs
    _layout = {"f64": (nat.CRYPTO_F64_FIELDS, ()), "i32": (nat.CRYPTO_I32_FIELDS, ()),
               "f32": ((), ("stocks",))}

    def __init__(self, config, num_envs, *, lookback=1, initial_capital=1e6, buy_cost_pct=1e-3,
                 sell_cost_pct=1e-3, gamma=0.99, auto_reset=True, device="cuda", windows=None):
        import torch
        self._set_device(device)
        self.price_array = np.ascontiguousarray(config["price_array"], dtype=np.float64)
        self.tech_array = np.ascontiguousarray(config["tech_array"], dtype=np.float64)
        T, N = self.price_array.shape
        W = self.tech_array.shape[1]
        E = int(num_envs)
        self.num_envs = self.env_num = E
        self.crypto_num = self.action_dim = N
        self.lookback = lookback
        self.max_step = T - lookback - 1                                         # :24
        self.obs_dim = 1 + N + W * lookback
        self.state_dim = 1 + (N + W) * lookback                                  # as declared, :40
        self.gamma = gamma
        self.initial_cash = initial_capital
        self.auto_reset = bool(auto_reset)
        self._window_min = lookback + 2                   # the n_steps rule of finenv_crypto_create
        self._norm_table = self._norm_rows = None
        # (the handle-wide normaliser is that of panel row 0, where the reference raises on a price
        #  <= 0; with windows nobody need start there, and row 0 of the table says the same or NaN)
        self.action_norm_vector = action_norm_vector(self.price_array[0]) if windows is None \
            else self.norm_table()[0].copy()
        self.observation_space = Box(-3000, 3000, (self.obs_dim,), np.float32)
        self.action_space = Box(-1, 1, (N,), np.float32)
        self._open(nat.CryptoConfig(E, N, W, T, lookback, 0, float(initial_capital),
                                    float(buy_cost_pct), float(sell_cost_pct), float(gamma)))
        dev = self.device
        self._price = torch.from_numpy(self.price_array).to(dev)
        self._tech = torch.from_numpy((self.tech_array * 2 ** -15).astype(np.float32)).to(dev)
        self._norm = torch.from_numpy(np.ascontiguousarray(self.action_norm_vector)).to(dev)
        self._alloc_state(E, N)
        self.state["cash"].fill_(float(initial_capital))                         # __init__ :26-35
        self.state["total_asset"].fill_(float(initial_capital))
        self.state["time"].fill_(lookback - 1)
        self._bind(self._price, self._tech, self._norm)
        self._alloc_outputs(E, self.obs_dim)
        if windows is not None:                       # the constructor's episode: each on its own window
            self.set_windows(*self._check_windows(*windows))
            self.active_windows.copy_(self.windows)
            self.state["time"].copy_(self.windows[0] + (lookback - 1))

    # ------------------------------------------------------------------ episode windows
    _window_active = True
    _window_rows = property(lambda self: self.price_array.shape[0])

    def _window_max_step(self, longest):
        return longest - self.lookback - 1                                       # :24

    def norm_table(self):
        """``action_norm_table(price_array)``, f64 [T, N] on the host; built on first use."""
        if self._norm_table is None:
            self._norm_table = action_norm_table(self.price_array)
        return self._norm_table

    def _attach_windows(self, ptr):
        import torch
        if ptr is not None and self._norm_rows is None:
            self._norm_rows = torch.from_numpy(self.norm_table()).to(self.device)
        self._call("set_windows", ptr,
                   C.c_void_p(self._norm_rows.data_ptr()) if ptr is not None else None)

    def _check_window_starts(self, start):
        bad = np.isnan(self.norm_table()[start, 0])
        if bad.any():
            raise ValueError(f"windows: start row {int(start[np.argmax(bad)])} holds a price <= 0 "
                             "(the reference's action normaliser raises there)")

    def set_windows(self, start, end=None, mask=None):
        """Per-env episode windows [start, end) of panel rows (finenv_crypto_set_windows), with the
        arguments, validation and device-tensor rules of ``WindowedEnv.set_windows``; a window
        needs ``lookback + 2`` rows and a start row whose prices are all positive (host values are
        checked for both).  ``set_windows(None)`` detaches.

        ``self.windows`` holds the PENDING windows: an env takes its pair at its next reset
        (``reset()`` or the auto-reset inside ``step``) and runs the whole episode on it -- start,
        end and the action normaliser of the start row -- whatever is written here meanwhile; the
        running episodes' windows are in ``self.active_windows`` (kernel-owned, read-only for the
        caller).  So windows can be redrawn for the envs that just finished with torch ops alone,
        also inside a captured graph, with no reset launch::

            obs, rew, done, _ = env.step(actions)          # auto-reset: took the pending windows
            env.set_windows(*random_windows(T, E, L, device=dev), mask=done)   # for the one after

        As in the reference's ``reset()``, ``gamma_return`` and ``episode_return`` survive a reset:
        for "a fresh env object on a new slice" zero ``state["gamma_return"]`` of those envs.
        Attaching windows to a running batch leaves every env on the whole panel until its next
        reset.  ``max_step`` is that of the longest pending window."""
        return super().set_windows(start, end, mask)

    def window_time(self):
        """The reference's ``self.time`` of every env (int32 [E] device tensor): ``state["time"]``
        minus the start row of the window its episode runs on."""
        if self.active_windows is None:
            return self.state["time"].clone()
        return self.state["time"] - self.active_windows[0]

    def close(self):
        pass

    supports_record = True      # step(..., record=...) stores the policy's outputs in the same launch

    def step(self, actions, out=None, record=None):
        """actions f32 [E,N] (NOT modified: the reference scales its input in place, :63-65).
        out=(obs, reward, done) optionally directs the outputs into caller tensors, e.g. slice t
        of rollout buffers [n_steps, E, ...] -- collecting a rollout needs no copy.
        record=(values, log_probs, actions_out, values_out, log_probs_out): also copy this step's
        policy outputs into the rollout tensors, in the same launch (finenv_crypto_step_record;
        contiguous float32, 16-byte aligned, E % 4 == 0 -- else use RolloutBuffer.put)."""
        if record is None:
            return super().step(actions, out)
        import torch
        actions = self._actions(actions)
        obs, rew, done = out if out is not None else (self.obs, self.reward, self.done)
        v, lp, a_out, v_out, lp_out = record
        for t_ in (v, lp, a_out, v_out, lp_out):
            if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.device != self.obs.device:
                raise ValueError("record tensors must be contiguous float32 on the env's device")
        if a_out.numel() != actions.numel() or v.numel() != self.num_envs or \
                lp.numel() != self.num_envs or v_out.numel() != self.num_envs or \
                lp_out.numel() != self.num_envs:
            raise ValueError("record: expected values / log_probs [E] and actions_out [E, N]")
        self._call("step_record", C.c_void_p(actions.data_ptr()), C.c_void_p(obs.data_ptr()),
                   C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()),
                   C.c_void_p(self.term_obs.data_ptr()) if self.term_obs is not None else None,
                   int(self.auto_reset), C.c_void_p(v.data_ptr()), C.c_void_p(lp.data_ptr()),
                   C.c_void_p(a_out.data_ptr()), C.c_void_p(v_out.data_ptr()),
                   C.c_void_p(lp_out.data_ptr()), self._stream())
        return obs, rew, done, None

    history = None              # enable_history()

    def enable_history(self, capacity=None, stocks=True):
        """Record every env's episode on the device: ``total_asset`` and the value of the holdings
        after every step and (with ``stocks``) the holdings themselves, written by the step kernel
        itself (finenv_crypto_set_history) -- no ``state_numpy()`` per step, no host loop, and it sits
        in a captured graph.  Returns the ``finrl_amd.history.CryptoEpisodeHistory`` (also
        ``self.history``), whose ``episode_total_assets(e)`` is the list the reference's
        DRL_prediction_load_from_file returns and ``account_values(e)`` the true equity curve;
        idempotent: a second call returns the same object whatever its arguments.

        ``capacity``: entries per env, by default the longest episode (``max_step - lookback + 2``
        entries: the armed one and one per step; ``L - 2 * lookback + 1`` for the longest pending
        window of ``L`` rows) AS IT IS AT THIS CALL: windows made longer by a later ``set_windows`` do
        not grow the tensors, and the longer episodes then end with ``overflow`` set and their first
        ``capacity`` entries recorded -- pass ``capacity`` for the longest window to come.  Every env
        is armed from its current state; ``reset(mask)`` re-arms the envs it resets, an auto-reset
        does not (the finished record stays readable).

        Memory: ``E * (16 * capacity + 12) + 4 * E * N * capacity`` bytes: 262,144 envs on 1,440-row
        windows of 10 pairs are 6 GB without and 21 GB with ``stocks``, which is why it is optional.

        Enable it before capturing a graph (the tensors' addresses are launch arguments)."""
        if self.history is None:
            from .history import CryptoEpisodeHistory
            self.history = CryptoEpisodeHistory(
                self, self.max_step - self.lookback + 2 if capacity is None else capacity, stocks)
        return self.history

    def episode_return(self):
        """total_asset / initial cash of each env's last finished episode (:89), f32."""
        import torch
        return self.state["episode_return"].to(torch.float32)
