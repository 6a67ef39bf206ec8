"""Device-resident batch of the reference's array-state StockTradingEnv
(finrl/meta/env_stock_trading/env_stocktrading_np.py:8-169; ElegantRL / RLlib-facing),
one HIP launch per step through the C ABI (finenv_stocknp_*)."""
from __future__ import annotations

import numpy as np

from . import _native as nat
from .spaces import Box
from .vec_base import WindowedEnv

TAG_PY, TAG_F32, TAG_F64 = 0, 1, 2


def derive_arrays(price_array, tech_array, turbulence_array, turbulence_thresh=99):
    """Host-side array preparation of __init__ (:27-35) and sigmoid_sign (:164-169)."""
    price = np.asarray(price_array).astype(np.float32)
    tech = np.asarray(tech_array).astype(np.float32)
    tech = tech * 2 ** -7
    turb = np.asarray(turbulence_array)
    turb_bool = (turb > turbulence_thresh).astype(np.float32)

    def sigmoid(x):
        return 1 / (1 + np.exp(-x * np.e)) - 0.5
    turb_ary = (sigmoid(turb / turbulence_thresh) * turbulence_thresh * 2 ** -5).astype(np.float32)
    return price, tech, turb_ary, turb_bool


class VecStockTradingEnvNP(WindowedEnv):
    """E parallel copies; constructor mirrors the reference (``config`` dict with
    price_array / tech_array / turbulence_array / if_train).

    ``windows=(start, end)`` gives every env its own episode window of panel rows ``[start, end)``
    (one pair for all envs, or [E] arrays / tensors): env e then equals the reference env built on
    ``{'price_array': price_array[s:t], 'tech_array': tech_array[s:t], 'turbulence_array':
    turbulence_array[s:t]}`` -- the train and test date ranges of finrl/train.py and finrl/test.py,
    or random training windows, in ONE batch over one panel.  ``state["day"]`` stays the panel row;
    ``window_day()`` is the reference's ``self.day``.  See ``set_windows``."""

    env_name = "StockEnv-MI355X"
    if_discrete = False
    target_return = 10.0
    _kind = "stocknp"
    _panel_cls, _state_cls = nat.StockNpPanelPtrs, nat.StockNpStatePtrs
    _layout = {"f64": (nat.STOCKNP_F64_FIELDS, ()), "i32": (nat.STOCKNP_I32_FIELDS, ()),
               "f32": ((), ("stocks", "cool_down", "stocks0"))}
    _pitched = True

    def __init__(self, config, num_envs, *, gamma=0.99, turbulence_thresh=99, min_stock_rate=0.1,
                 max_stock=1e2, initial_capital=1e6, buy_cost_pct=1e-3, sell_cost_pct=1e-3,
                 reward_scaling=2 ** -11, initial_stocks=None, auto_reset=True, device="cuda",
                 seed=0, obs_amount_floor=0.0, obs_pitch=None, windows=None):
        import torch
        self._set_device(device)
        price, tech, turb_ary, turb_bool = derive_arrays(
            config["price_array"], config["tech_array"], config["turbulence_array"],
            turbulence_thresh)
        self.price_ary, self.tech_ary = price, tech
        self.turbulence_ary, self.turbulence_bool = turb_ary, turb_bool
        self.if_train = bool(config.get("if_train", False))
        T, N = price.shape
        W = tech.shape[1]
        E = int(num_envs)
        self.num_envs = self.env_num = E
        self.action_dim = N
        self.state_dim = 1 + 2 + 3 * N + W                                        # :63
        self.max_step = T - 1                                                     # :67
        self.gamma, self.max_stock, self.initial_capital = gamma, max_stock, initial_capital
        self.auto_reset = bool(auto_reset)
        self.observation_space = Box(-3000, 3000, (self.state_dim,), np.float32)
        self.action_space = Box(-1, 1, (N,), np.float32)
        self.initial_stocks = np.zeros(N, np.float32) if initial_stocks is None else \
            np.asarray(initial_stocks, np.float32)
        self._stocks_dev = torch.from_numpy(self.initial_stocks).to(self.device)[:, None]
        self.generator = self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed)
        self._open(nat.StockNpConfig(E, N, W, T, int(max_stock * min_stock_rate), 0,
                                     float(max_stock), float(buy_cost_pct), float(sell_cost_pct),
                                     float(reward_scaling), float(gamma), float(obs_amount_floor)))
        D = self.state_dim
        tmpl = np.zeros((T, D), np.float32)
        tmpl[:, 1] = turb_ary
        tmpl[:, 2] = turb_bool
        tmpl[:, 3:3 + N] = price * np.array(2 ** -6, dtype=np.float32)           # :151, :157
        tmpl[:, 3 + 3 * N:] = tech
        dev = self.device
        self._price = torch.from_numpy(np.ascontiguousarray(price)).to(dev)
        self._tmpl = torch.from_numpy(tmpl).to(dev)
        self._tbool = torch.from_numpy(np.ascontiguousarray(turb_bool)).to(dev)
        self._alloc_state(E, N)
        self.set_start_state(self.initial_stocks, float(initial_capital), TAG_PY)
        self._bind(self._price, self._tmpl, self._tbool)
        # obs: [E, D] view of a buffer whose rows start on 64-byte boundaries (vec_base.obs_pitch_for)
        self._alloc_outputs(E, D, obs_pitch)
        if windows is not None:                       # the constructor's episode: each on its own window
            self.set_windows(*self._check_windows(*windows))
            self.active_windows.copy_(self.windows)
            self.state["day"].copy_(self.windows[0])

    # ------------------------------------------------------------------ episode windows
    _window_active = True                             # pending / active rows, as the crypto env
    _window_min = 2                                   # the n_days rule of finenv_stocknp_create
    _window_rows = property(lambda self: self.price_ary.shape[0])

    def set_windows(self, start, end=None, mask=None):
        """Per-env episode windows [start, end) of panel rows (finenv_stocknp_set_windows), with the
        arguments, validation and device-tensor rules of ``WindowedEnv.set_windows``; a window
        needs two rows (host values are checked).  ``set_windows(None)`` detaches.

        ``self.windows`` holds the PENDING windows: an env takes its pair at its next reset
        (``reset()`` or the auto-reset inside ``step``) and runs the whole episode on it, whatever
        is written here meanwhile; the running episodes' windows are in ``self.active_windows``
        (kernel-owned, read-only for the caller).  So windows can be redrawn for the envs that just
        finished with torch ops alone, also inside a captured graph, with no reset launch::

            obs, rew, done, _ = env.step(actions)          # auto-reset: took the pending windows
            env.set_windows(*random_windows(T, E, L, device=dev), mask=done)   # for the one after
            env.draw_train_start(mask=done)                # if_train: start states on the new rows

        Attaching windows to a running batch leaves every env on the whole panel until its next
        reset.  ``max_step`` is that of the longest pending window."""
        return super().set_windows(start, end, mask)

    def window_day(self):
        """The reference's ``self.day`` of every env (int32 [E] device tensor): ``state["day"]``
        minus the start row of the window its episode runs on."""
        if self.active_windows is None:
            return self.state["day"].clone()
        return self.state["day"] - self.active_windows[0]

    def set_start_state(self, stocks0, amount0, amount0_tag):
        """Per-env state that reset() restores: stocks0 [N] or [E,N], amount0 scalar or [E],
        dtype tag (TAG_PY for the eval-mode Python float, TAG_F32 for train-mode draws)."""
        import torch
        E, N = self.num_envs, self.action_dim
        s = np.broadcast_to(np.asarray(stocks0, np.float32), (E, N))
        self.state["stocks0"].copy_(torch.from_numpy(np.array(s.T, order="C", copy=True)))
        self.state["amount0"].copy_(torch.from_numpy(
            np.array(np.broadcast_to(np.asarray(amount0, np.float64), (E,)), copy=True)))
        self.state["amount0_tag"].copy_(torch.from_numpy(
            np.array(np.broadcast_to(np.asarray(amount0_tag, np.int32), (E,)), copy=True)))

    def draw_train_start(self, mask=None):
        """Train-mode start state (:85-92), drawn on device with this env's generator (the
        reference uses the global numpy RNG, so its draws are not reproducible elsewhere) -- for
        every env, or those with ``mask[e]`` set.  The cash left after the drawn holdings is priced
        on the first row of the env's slice: ``price[pending start]`` per env with windows, row 0
        without.  ``reset()`` calls this in train mode; call it yourself for the envs that were
        just given new windows (see ``set_windows``), so that their next episode starts on a draw
        priced on its own first row.  Torch ops only, no host synchronisation: it can be captured
        in a graph (register ``self.generator`` with the graph first:
        ``graph.register_generator_state(env.generator)``)."""
        import torch
        E, N = self.num_envs, self.action_dim
        st = self._stocks_dev + torch.randint(
            0, 64, (N, E), generator=self._gen, device=self.device).to(torch.float32)
        u = torch.rand(E, generator=self._gen, device=self.device, dtype=torch.float64) * 0.1 + 0.95
        if self.windows is None:
            first = self._price[0][:, None]
        else:                                         # [N, E]: the first row of every env's slice
            rows = self.windows[0].clamp(0, self._window_rows - 1).to(torch.int64)
            first = self._price.index_select(0, rows).T
        amount = ((self.initial_capital * u).to(torch.float32) - (st * first).sum(0)).to(torch.float64)
        if mask is None:
            self.state["stocks0"].copy_(st)
            self.state["amount0"].copy_(amount)
            self.state["amount0_tag"].fill_(TAG_F32)
            return
        m = mask.to(device=self.device, dtype=torch.bool)
        self.state["stocks0"].copy_(torch.where(m, st, self.state["stocks0"]))
        self.state["amount0"].copy_(torch.where(m, amount, self.state["amount0"]))
        self.state["amount0_tag"].masked_fill_(m, TAG_F32)

    def _before_reset(self):
        if self.if_train:
            self.draw_train_start()

    history = None              # enable_history()

    def enable_history(self, capacity=None, stocks=True, tags=True):
        """Record every env's episode on the device: ``total_asset`` after every step, with ``tags`` its
        NumPy scalar type and with ``stocks`` the holdings, written by the step kernel itself
        (finenv_stocknp_set_history) -- no ``state_numpy()`` per step, no host loop, it sits in a
        captured graph, and under ``auto_reset`` it keeps the terminal value the state no longer
        holds.  Returns the ``finrl_amd.history.StockNpEpisodeHistory`` (also ``self.history``), whose
        ``episode_total_assets(e)`` is the list the reference's DRLAgent.DRL_prediction returns;
        idempotent: a second call returns the same object whatever its arguments.

        ``capacity``: entries per env, by default the longest episode (``max_step + 1``: the armed
        entry and one per step; ``L`` for the longest pending window of ``L`` rows, ``T`` without
        windows) AS IT IS AT THIS CALL: windows made longer by a later ``set_windows`` do not grow the
        tensors, and the longer episodes then end with ``overflow`` set and their first ``capacity``
        entries recorded -- pass ``capacity`` for the longest window to come.  Every env is armed from
        its current state; ``reset(mask)`` re-arms the envs it resets, an auto-reset does not (the
        finished record stays readable).

        Memory: ``E * (8 * capacity + 12)`` bytes, ``E * capacity`` more with ``tags`` and
        ``4 * E * N * capacity`` more with ``stocks``: 65,536 envs on 504-row windows of the DOW30 are
        0.3 GB without and 4.3 GB with ``stocks``, which is why it is optional.

        Enable it before capturing a graph (the tensors' addresses are launch arguments)."""
        if self.history is None:
            from .history import StockNpEpisodeHistory
            self.history = StockNpEpisodeHistory(
                self, self.max_step + 1 if capacity is None else capacity, stocks, tags)
        return self.history

    def episode_return(self):
        """total_asset / initial_total_asset of each env's last finished episode (:145), f32."""
        import torch
        return self.state["episode_return"].to(torch.float32)

    def state_numpy(self):
        out = super().state_numpy()
        t = out["tags"]
        out["amount_tag"], out["ta_tag"], out["g_tag"] = t & 3, (t >> 2) & 3, (t >> 4) & 3
        out["reward_tag"] = (t >> 8) & 3
        return out
