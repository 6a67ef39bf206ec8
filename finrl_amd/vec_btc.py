"""Device-resident batch of the reference's single-asset BitcoinEnv
(finrl/meta/env_cryptocurrency_trading/env_btc_ccxt.py:6-215), one HIP launch per step through the
C ABI (finenv_btc_*).  Not VecCryptoEnv with one asset: this env may go short, buys fractional
amounts and adds the discounted return to the terminal reward (include/finenv.h)."""
from __future__ import annotations

import numpy as np

from . import _native as nat
from .spaces import Box
from .vec_base import WindowedEnv

TAG_PY, TAG_F32, TAG_F64 = 0, 1, 2
TAG_TYPES = (float, np.float32, np.float64)              # the scalar type of `stocks` by its tag
MODES = ("train", "test", "trade")
# the observation's scale of tech_ary[:, 0..7) (:62-70)
TECH_SCALE = (2 ** -1, 2 ** -15, 2 ** -15, 2 ** -6, 2 ** -6, 2 ** -15, 2 ** -15)


def checked_arrays(price_ary, tech_ary):
    """The contract of the inputs: float64 [T, P] and [T, W >= 7] arrays.  Other dtypes change the
    reference's own arithmetic (NumPy 2 promotes a float32 price differently), so they are refused,
    never converted."""
    for a, what in ((price_ary, "price_ary"), (tech_ary, "tech_ary")):
        if not isinstance(a, np.ndarray) or a.dtype != np.float64:
            raise TypeError(f"{what} must be a float64 numpy array "
                            f"(got {getattr(a, 'dtype', type(a).__name__)})")
        if a.ndim != 2:
            raise ValueError(f"{what} must be 2-D [rows, columns]")
    if price_ary.shape[0] != tech_ary.shape[0]:
        raise ValueError("price_ary and tech_ary must have the same number of rows")
    if price_ary.shape[0] < 2:
        raise ValueError("an episode needs at least two rows")
    if not 1 <= price_ary.shape[1] <= nat.BTC_MAX_PRICE_COLS:
        raise ValueError(f"price_ary needs 1 .. {nat.BTC_MAX_PRICE_COLS} columns")
    if tech_ary.shape[1] < 7:
        raise ValueError("tech_ary needs at least 7 columns (the observation shows the first seven)")
    return np.ascontiguousarray(price_ary), np.ascontiguousarray(tech_ary)


def obs_template(price_ary, tech_ary):
    """f32 [T, P + 7]: columns 1 .. D-2 of every row's observation -- the scaling expressions of
    :62-75 evaluated in float64, then the cast of :78."""
    mid = np.hstack((price_ary * 2 ** -15, tech_ary[:, :7] * np.asarray(TECH_SCALE)))
    return np.ascontiguousarray(mid.astype(np.float32))


def mode_arrays(price_ary, tech_ary, time_frequency, start, mid1, mid2, end):
    """load_data (:176-215) for all three modes -> {mode: (price, tech)}: the slices [start:mid1],
    [mid1:mid2], [mid2:end], each subsampled to its rows tf * i, i < n // tf."""
    tf = int(time_frequency)
    out = {}
    for mode, sl in zip(MODES, (slice(start, mid1), slice(mid1, mid2), slice(mid2, end))):
        p, t = price_ary[sl], tech_ary[sl]
        keep = tf * np.arange(p.shape[0] // tf)
        out[mode] = (p[keep], t[keep])
    return out


def mode_panel(price_ary, tech_ary, time_frequency=15, start=None, mid1=172197, mid2=216837, end=None):
    """The three modes' arrays concatenated into ONE panel -> (price, tech, windows), windows =
    {mode: (first row, end row)} of that panel: train, test and trade envs then run in one batch,

        price, tech, win = mode_panel(price_ary, tech_ary, 15, None, mid1, mid2, None)
        start = [win[m][0] for m in modes_of_envs]; end = [win[m][1] for m in modes_of_envs]
        env = VecBitcoinEnv(price, tech, E, windows=(np.array(start), np.array(end)))

    and env e equals the reference env built with ``mode=modes_of_envs[e]``."""
    parts = mode_arrays(price_ary, tech_ary, time_frequency, start, mid1, mid2, end)
    windows, at = {}, 0
    for mode in MODES:
        n = parts[mode][0].shape[0]
        windows[mode] = (at, at + n)
        at += n
    return (np.concatenate([parts[m][0] for m in MODES]), np.concatenate([parts[m][1] for m in MODES]),
            windows)


class VecBitcoinEnv(WindowedEnv):
    """E parallel BitcoinEnv over ``price_ary`` [T, P] and ``tech_ary`` [T, W >= 7] (float64, the
    arrays the reference's ``load_data`` ends up with; trades use price column 0).
    step(actions f32 [E, 1]) -> (obs f32 [E, P + 9], reward f32 [E], done u8 [E], None); the float64
    reward of the last step is ``state["last_reward"]``.

    ``windows=(start, end)`` gives every env its own episode window of panel rows ``[start, end)``
    (one pair for all envs, or [E] arrays / tensors): env e then equals the reference env whose
    arrays are those rows -- see ``mode_panel`` for the three modes in one batch.  ``state["day"]``
    stays the panel row; ``window_day()`` is the reference's ``self.day``.  As in VecStockTradingEnv
    an edited end applies from the next step and an edited start at the env's next reset
    (``set_windows``); ``window_day()`` counts from the start in ``self.windows``.

    ``state["stocks_tag"]`` is the NumPy scalar type the reference's ``stocks`` has (TAG_PY / TAG_F32
    / TAG_F64: its arithmetic depends on it); ``reset()`` leaves ``gamma_return`` and
    ``episode_return`` alone, as the reference's does.  An env stepped again on its terminal row
    (auto_reset off) makes no trade and reports reward 0, done 1 where the reference raises."""

    env_name = "BitcoinEnv4-MI355X"
    if_discrete = False
    target_return = 10
    _kind = "btc"
    _panel_cls, _state_cls = nat.BtcPanelPtrs, nat.BtcStatePtrs
    _layout = {"f64": (nat.BTC_F64_FIELDS, ()), "i32": (nat.BTC_I32_FIELDS, ())}
    _window_min = 2                                   # the n_rows rule of finenv_btc_create
    _window_rows = property(lambda self: self.price_ary.shape[0])
    mode_panel = staticmethod(mode_panel)

    def __init__(self, price_ary, tech_ary, num_envs, *, initial_account=1e6,
                 transaction_fee_percent=1e-3, gamma=0.99, auto_reset=True, device="cuda",
                 windows=None):
        import torch
        self._set_device(device)
        self.price_ary, self.tech_ary = checked_arrays(price_ary, tech_ary)
        T, P = self.price_ary.shape
        W = self.tech_ary.shape[1]
        E = int(num_envs)
        self.num_envs = self.env_num = E
        self.stock_dim = self.action_dim = 1
        self.obs_dim = P + 9
        self.state_dim = 1 + 1 + P + W                    # as declared, :47 (== obs_dim when W == 7)
        self.max_step = T                                 # :51 (an episode is T - 1 steps)
        self.initial_account = initial_account
        self.transaction_fee_percent = transaction_fee_percent
        self.gamma = gamma
        self.auto_reset = bool(auto_reset)
        self.observation_space = Box(-np.inf, np.inf, (self.obs_dim,), np.float32)
        self.action_space = Box(-1, 1, (1,), np.float32)
        self._open(nat.BtcConfig(E, P, W, T, 0, 0, float(initial_account),
                                 float(transaction_fee_percent), float(gamma)))
        dev = self.device
        self._price0 = torch.from_numpy(np.ascontiguousarray(self.price_ary[:, 0])).to(dev)
        self._tmpl = torch.from_numpy(obs_template(self.price_ary, self.tech_ary)).to(dev)
        self._alloc_state(E, 1)
        self.state["account"].fill_(float(initial_account))                      # __init__ :34-43
        self.state["total_asset"].fill_(float(initial_account))
        self._bind(self._price0, self._tmpl)
        self._alloc_outputs(E, self.obs_dim)
        if windows is not None:                       # the constructor's episode: day 0 of each window
            self.set_windows(*self._check_windows(*windows))
            self.state["day"].copy_(self.windows[0])

    def _window_max_step(self, longest):
        return longest                                                            # :51

    def _actions(self, actions):
        """float32 [E, 1] (or [E]) on the env's device; any other dtype is refused: the reference's
        arithmetic depends on the action's scalar type."""
        import torch
        if isinstance(actions, np.ndarray):
            if actions.dtype != np.float32:
                raise TypeError(f"actions must be float32 (got {actions.dtype})")
            actions = torch.from_numpy(np.ascontiguousarray(actions))
        if not torch.is_tensor(actions) or actions.dtype != torch.float32:
            raise TypeError("actions must be a float32 tensor "
                            f"(got {getattr(actions, 'dtype', type(actions).__name__)})")
        if actions.numel() != self.num_envs:
            raise ValueError(f"actions must hold one value per env ([{self.num_envs}, 1])")
        return actions.to(self.device).reshape(self.num_envs, 1).contiguous()

    def window_day(self):
        """The reference's ``self.day`` of every env (int32 [E] device tensor): ``state["day"]`` minus
        the env's window start in ``self.windows`` (``state["day"]`` without windows)."""
        if self.windows is None:
            return self.state["day"].clone()
        return self.state["day"] - self.windows[0]

    def episode_return(self):
        """total_asset / initial_account of each env's last finished episode (:128), latched by the
        step that reported done; f32."""
        import torch
        return self.state["episode_return"].to(torch.float32)

    def state_numpy(self):
        """Host copy of the per-env state; ``stocks_tag`` is the scalar type of ``stocks``
        (``TAG_TYPES[tag]``)."""
        out = super().state_numpy()
        out["window_day"] = self.window_day().cpu().numpy()
        return out

    def close(self):
        pass
