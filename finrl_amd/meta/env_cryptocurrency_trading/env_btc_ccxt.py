"""Drop-in for ``finrl.meta.env_cryptocurrency_trading.env_btc_ccxt.BitcoinEnv``
(env_btc_ccxt.py:6-215 in the reference tree): same constructor keywords (``data_cwd`` and its
``np.load`` included), attributes, ``reset() / step()`` protocol (``info`` is ``None``) and
``draw_cumulative_return``, one HIP launch per step through the C ABI (finenv_btc_*).  Single-env
facade over :class:`finrl_amd.vec_btc.VecBitcoinEnv`; use ``make_vec`` for throughput.

Values AND scalar types are the reference's under NumPy 2: ``stocks`` is a ``float``, ``np.float32``
or ``np.float64`` by what the trades so far made it, the reward an ``np.float64``.  The contract is
float64 arrays and float32 actions (what ElegantRL's ``act(...).cpu().numpy()[0]`` hands over);
anything else raises TypeError.  Stepping again after ``done`` makes no trade and returns reward 0,
done True, where the reference raises IndexError."""
from __future__ import annotations

import numpy as np

from ...vec_btc import MODES, TAG_TYPES, VecBitcoinEnv, mode_arrays, mode_panel
from .._single import to_action_tensor


class BitcoinEnv:
    def __init__(self, data_cwd=None, price_ary=None, tech_ary=None, time_frequency=15, start=None,
                 mid1=172197, mid2=216837, end=None, initial_account=1e6, max_stock=1e2,
                 transaction_fee_percent=1e-3, mode="train", gamma=0.99, device="cuda"):
        self.stock_dim = 1
        self.initial_account = initial_account
        self.transaction_fee_percent = transaction_fee_percent
        self.max_stock = 1                                # (whatever the keyword says, :26)
        self.gamma = gamma
        self.mode = mode
        self.load_data(data_cwd, price_ary, tech_ary, time_frequency, start, mid1, mid2, end)
        self._vec = VecBitcoinEnv(self.price_ary, self.tech_ary, 1, initial_account=initial_account,
                                  transaction_fee_percent=transaction_fee_percent, gamma=gamma,
                                  auto_reset=False, device=device)
        self.price_ary, self.tech_ary = self._vec.price_ary, self._vec.tech_ary
        self.initial_account__reset = self.initial_account
        self.episode_return = 0.0
        self.gamma_return = 0.0
        self.env_name = "BitcoinEnv4"
        self.state_dim = self._vec.state_dim              # as declared: 1 + 1 + P + W, :47
        self.action_dim = 1
        self.if_discrete = False
        self.target_return = 10
        self.max_step = self.price_ary.shape[0]
        self._sync(traded=False)

    @classmethod
    def make_vec(cls, price_ary, tech_ary, num_envs, **kw):
        return VecBitcoinEnv(price_ary, tech_ary, num_envs, **kw)

    mode_panel = staticmethod(mode_panel)

    def load_data(self, data_cwd, price_ary, tech_ary, time_frequency, start, mid1, mid2, end):
        if data_cwd is not None:
            try:
                price_ary = np.load(f"{data_cwd}/price_ary.npy")
                tech_ary = np.load(f"{data_cwd}/tech_ary.npy")
            except BaseException:
                raise ValueError("Data files not found!")
        if self.mode not in MODES:
            raise ValueError("Invalid Mode!")
        self.price_ary, self.tech_ary = mode_arrays(price_ary, tech_ary, time_frequency, start, mid1,
                                                    mid2, end)[self.mode]

    def _sync(self, traded):
        """The reference's attributes from the device state.  ``traded``: a trade has touched the
        account since reset(), which is what makes it an np.float64."""
        st = self._vec.state_numpy()
        self.day = int(st["day"][0])
        self.day_price = self.price_ary[self.day]
        self.day_tech = self.tech_ary[self.day]
        self.account = st["account"][0] if traded else self.initial_account__reset
        self.stocks = TAG_TYPES[int(st["stocks_tag"][0])](st["stocks"][0])
        self.total_asset = st["total_asset"][0]
        self._traded = traded
        return st

    def reset(self) -> np.ndarray:
        obs = self._vec.reset().cpu().numpy()[0]
        self.initial_account__reset = self.initial_account
        self._sync(traded=False)
        return obs

    def step(self, action) -> (np.ndarray, float, bool, None):
        if not isinstance(action, np.ndarray) or action.dtype != np.float32:
            raise TypeError("action must be a float32 numpy array (the reference's arithmetic depends "
                            f"on its scalar type); got {getattr(action, 'dtype', type(action).__name__)}")
        a = action.reshape(-1)[:1]
        over = self.day + 1 >= self.max_step              # stepped again after done: nothing happens
        obs, _, done, _ = self._vec.step(to_action_tensor(self._vec, a))
        st = self._sync(traded=self._traded or (not over and bool(a[0] < 0 or a[0] > 0)))
        d = bool(done.cpu().numpy()[0])
        reward = st["last_reward"][0]
        if not over:
            self.gamma_return = 0.0 if d else st["gamma_return"][0]               # :124-127
            if d:
                self.episode_return = st["episode_return"][0]                     # :128
        return obs.cpu().numpy()[0], reward, d, None

    def draw_cumulative_return(self, args, _torch) -> list:
        """One episode driven by ``args.agent`` -> (episode_returns, btc_returns), plotted to
        ``{args.cwd}/cumulative_return.jpg``.  As in the reference, the agent's curve is
        ``total_asset / 1e6`` whatever ``initial_account`` is."""
        agent, cwd = args.agent, args.cwd
        agent.init(args.net_dim, self.state_dim, self.action_dim)
        agent.save_load_model(cwd=cwd, if_save=False)
        state = self.reset()
        first_price = self.day_price[0]
        episode_returns, btc_returns = [1], []
        with _torch.no_grad():
            for _ in range(self.max_step):
                btc_returns.append(self.day_price[0] / first_price)
                s_tensor = _torch.as_tensor((state,), device=agent.device)
                action = agent.act(s_tensor).detach().cpu().numpy()[0]
                state, _, done, _ = self.step(action)
                episode_returns.append(self.total_asset / 1e6)
                if done:
                    break

        import matplotlib.pyplot as plt
        plt.plot(episode_returns, label="agent return")
        plt.plot(btc_returns, color="yellow", label="BTC return")
        plt.grid()
        plt.title("cumulative return")
        plt.xlabel("day")
        plt.ylabel("multiple of initial_account")
        plt.legend()
        plt.savefig(f"{cwd}/cumulative_return.jpg")
        return episode_returns, btc_returns

    def close(self):
        pass
