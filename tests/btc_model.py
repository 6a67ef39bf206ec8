"""Scalar CPU model of the single-asset BitcoinEnv (env_btc_ccxt.py in the reference tree), for the
tests of the batched env only -- the product never imports it.

An independent restatement, not a transcription: every number is a Python float (IEEE float64),
the NumPy scalar type the reference's ``stocks`` would have is carried as an explicit tag, and
float32 arithmetic is spelled out as "round the float64 result to float32" (for one +, -, * or / of
two float32 values that double rounding is exact: 53 >= 2 * 24 + 2).  No NumPy promotion rule is
relied on anywhere.  tests/test_btc_model.py pins it to the recorded reference runs under
tests/golden/btc_*.npz at tolerance 0.
"""
from __future__ import annotations

import json
import os
import struct

import numpy as np

PY, F32, F64 = 0, 1, 2                      # FINENV_NT_*: float, np.float32, np.float64
TAG_TYPES = (float, np.float32, np.float64)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TECH_SCALE = (2.0 ** -1, 2.0 ** -15, 2.0 ** -15, 2.0 ** -6, 2.0 ** -6, 2.0 ** -15, 2.0 ** -15)
OP_RESET, OP_STEP = 0, 1
# float32 actions outside uniform(-1, 1): zeros, denormals, the largest finite values, +-inf, NaN,
# values past +-1 and +-1 themselves (btc_domain, tests/test_gpu_btc_domain.py)
SPECIAL_ACTIONS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, 1e30, -1e30, 3.4e38, -3.4e38, np.inf, -np.inf,
                            np.nan, 2.5, -7.0, 1.0, -1.0], np.float32)


def r32(x):
    """x rounded to the nearest float32, as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def tag_of(x):
    """The tag of a reference scalar by its exact type."""
    return TAG_TYPES.index(type(x))


def subsample(n_rows, time_frequency):
    """Row indices load_data keeps of a slice of n_rows rows."""
    tf = int(time_frequency)
    return [tf * i for i in range(n_rows // tf)]


def mode_rows(n, time_frequency, start, mid1, mid2, end):
    """Raw row indices of the train / test / trade arrays of load_data, by Python's slice rules."""
    out = {}
    for mode, sl in (("train", slice(start, mid1)), ("test", slice(mid1, mid2)), ("trade", slice(mid2, end))):
        rows = list(range(n))[sl]
        out[mode] = [rows[i] for i in subsample(len(rows), time_frequency)]
    return out


class BtcModel:
    """One env on rows [start, end) of (price_ary [T, P], tech_ary [T, W]) float64 arrays."""

    def __init__(self, price_ary, tech_ary, *, initial_account=1e6, transaction_fee_percent=1e-3,
                 gamma=0.99, start=0, end=None):
        self.price = np.asarray(price_ary, dtype=np.float64)
        self.tech = np.asarray(tech_ary, dtype=np.float64)
        self.initial_account = float(initial_account)
        self.fee = float(transaction_fee_percent)
        self.gamma = float(gamma)
        self.set_window(start, self.price.shape[0] if end is None else end)
        self.gamma_return = 0.0
        self.episode_return = 0.0
        self._restart()

    def set_window(self, start, end):
        self.start, self.end = int(start), int(end)

    # ------------------------------------------------------------------ state
    def _restart(self):
        self.day = self.start                                # a panel row
        self.account = self.initial_account
        self.stocks, self.tag = 0.0, PY
        self.total_asset = self.account + float(self.price[self.day, 0]) * self.stocks

    def reset(self):
        self._restart()
        return self.obs()

    def obs(self):
        row = [self.account * 2.0 ** -18]
        row += [float(v) * 2.0 ** -15 for v in self.price[self.day]]
        row += [float(self.tech[self.day, j]) * TECH_SCALE[j] for j in range(7)]
        row += [self.stocks * 2.0 ** -4]
        return np.array(row, dtype=np.float64).astype(np.float32)

    def _hold(self, sign, q, q_tag):
        """stocks += sign * q in the type the two scalar types give."""
        self.tag = max(self.tag, q_tag)
        if self.tag == F32:
            self.stocks = r32(r32(self.stocks) + sign * r32(q))
        else:
            self.stocks = self.stocks + sign * q

    # ------------------------------------------------------------------ step
    def step(self, action):
        """action: one float32 value -> (obs, float64 reward, done)."""
        a = float(action)
        assert r32(a) == a or a != a, "actions are float32"
        last = self.end - 1
        if self.day >= last:                                 # defined here: no trade past the end
            return self.obs(), 0.0, True
        adj = float(self.price[self.day, 0])
        if a < 0:
            want, cap = -a, 0.5 * self.total_asset / adj + self.stocks
            q, q_tag = (cap, F64) if cap < want else (want, F32)
            if q > 0:
                self.account = self.account + adj * q * (1 - self.fee)
                self._hold(-1.0, q, q_tag)
            else:
                self.account = self.account + adj * 0.0 * (1 - self.fee)
        elif a > 0:
            most = self.account / adj
            q, q_tag = (most, F64) if most < a else (a, F32)
            self.account = self.account - adj * q * (1 + self.fee)
            self._hold(1.0, q, q_tag)
        self.day += 1
        worth = self.account + float(self.price[self.day, 0]) * self.stocks
        reward = (worth - self.total_asset) * 2.0 ** -16
        self.total_asset = worth
        self.gamma_return = self.gamma_return * self.gamma + reward
        done = self.day == last
        if done:
            reward = reward + self.gamma_return
            self.gamma_return = 0.0
            self.episode_return = worth / self.initial_account
        return self.obs(), reward, done

    def record(self):
        return dict(account=self.account, stocks=self.stocks, tag=self.tag, total_asset=self.total_asset,
                    gamma_return=self.gamma_return, episode_return=self.episode_return)


# ---------------------------------------------------------------------- fixtures
RECORDED = ("obs", "reward", "done", "account", "stocks", "tag", "total_asset", "gamma_return",
            "episode_return")


def load_fixture(name):
    """tests/golden/<name>.npz -> {case: dict}.  Every case has kwargs (the reference constructor's
    keywords, arrays aside), price_ary / tech_ary (the arrays the reference env ended up with), ops
    [n] (OP_RESET / OP_STEP), actions [n] f32 and one row per op of each RECORDED quantity (reward and
    done of a reset: NaN and 0); fixtures built through load_data also carry raw_price / raw_tech."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {}
    for case in json.loads(str(z["cases"])):
        d = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + ".")}
        d["kwargs"] = json.loads(str(d["kwargs"]))
        out[case] = d
    return out


def model_kwargs(kwargs):
    return {k: kwargs[k] for k in ("initial_account", "transaction_fee_percent", "gamma") if k in kwargs}


def check_against(case, i, obs, reward, done, state, what=""):
    """Entry i of a fixture case equals (obs, reward, done) and the state record, bit for bit."""
    msg = f"{what} op {i}"
    assert np.array_equal(np.asarray(obs, np.float32).view(np.uint32), case["obs"][i].view(np.uint32)), msg
    if case["ops"][i] == OP_STEP:
        assert np.float64(reward).view(np.uint64) == case["reward"][i].view(np.uint64), msg
        assert bool(done) == bool(case["done"][i]), msg
    for k in ("account", "stocks", "total_asset", "gamma_return", "episode_return"):
        assert np.float64(state[k]).view(np.uint64) == case[k][i].view(np.uint64), f"{msg}: {k}"
    assert int(state["tag"]) == int(case["tag"][i]), f"{msg}: tag"


def fixture_branches(case):
    """How often the recorded steps of a fixture case took each cap branch, from the recorded state in
    front of each step alone (a case starts with a reset): the counts make_golden_btc.py's Recorder
    kept when it ran."""
    n = dict(short_cap=0, zero_sell=0, buy_cap=0, negative_buy=0)
    day = 0
    for i, op in enumerate(case["ops"]):
        if op == OP_RESET:
            day = 0
            continue
        a, adj = float(case["actions"][i]), float(case["price_ary"][day, 0])
        if a < 0:
            cap = 0.5 * float(case["total_asset"][i - 1]) / adj + float(case["stocks"][i - 1])
            n["short_cap"] += 0 < cap < -a
            n["zero_sell"] += cap <= 0
        elif a > 0:
            n["buy_cap"] += float(case["account"][i - 1]) / adj < a
            n["negative_buy"] += float(case["account"][i - 1]) < 0
        day += 1
    return n


# ---------------------------------------------------------------------- draw_cumulative_return
class StubTensor:
    def __init__(self, a):
        self.a = a

    def detach(self):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class StubTorch:
    """What draw_cumulative_return asks of its ``_torch`` argument."""

    class no_grad:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    @staticmethod
    def as_tensor(x, device=None):
        return np.asarray(x)


class StubAgent:
    """A deterministic actor: the action depends on the observation it is shown and on the call count."""
    device = "cpu"

    def __init__(self):
        self.calls = 0
        self.inited = None

    def init(self, net_dim, state_dim, action_dim):
        self.inited = (net_dim, state_dim, action_dim)

    def save_load_model(self, cwd, if_save):
        self.loaded = (cwd, if_save)

    def act(self, s):
        self.calls += 1
        x = float(np.asarray(s)[0][1])
        return StubTensor(np.array([[np.sin(1e4 * x + self.calls)]], dtype=np.float32))


class StubArgs:
    def __init__(self, cwd):
        self.agent, self.net_dim, self.cwd = StubAgent(), 16, cwd


# ---------------------------------------------------------------------- a batch of models
STATE_F64 = ("account", "stocks", "total_asset", "gamma_return", "episode_return")


class ModelBatch:
    """One BtcModel per env over one panel, env e on rows [start[e], end[e]), stepped with the
    batched env's protocol: auto_reset resets a done env inside the step (DummyVecEnv semantics)."""

    def __init__(self, price, tech, E, start=None, end=None, **kw):
        T = price.shape[0]
        s = np.broadcast_to(np.asarray(0 if start is None else start), (E,))
        t = np.broadcast_to(np.asarray(T if end is None else end), (E,))
        self.m = [BtcModel(price, tech, start=int(a), end=int(b), **kw) for a, b in zip(s, t)]
        self.E, self.D = E, price.shape[1] + 9

    def reset(self, mask=None):
        """-> {e: obs} of the envs it reset."""
        return {e: m.reset() for e, m in enumerate(self.m) if mask is None or mask[e]}

    def step(self, actions, auto_reset):
        """actions f32 [E] -> obs [E, D] f32, reward [E] f64, done [E] bool, {e: terminal obs}."""
        obs = np.zeros((self.E, self.D), np.float32)
        reward, done, term = np.zeros(self.E), np.zeros(self.E, bool), {}
        for e, m in enumerate(self.m):
            obs[e], reward[e], done[e] = m.step(actions[e])
            if done[e]:
                term[e] = obs[e].copy()
                if auto_reset:
                    obs[e] = m.reset()
        return obs, reward, done, term

    def state(self):
        out = {k: np.array([getattr(m, k) for m in self.m], np.float64) for k in STATE_F64}
        out["stocks_tag"] = np.array([m.tag for m in self.m], np.int32)
        out["day"] = np.array([m.day for m in self.m], np.int32)
        return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_state_equal(env_state, model_state, what=""):
    """Every state field of the batched env equals the models', bit for bit (day: the panel row)."""
    for k in STATE_F64:
        np.testing.assert_array_equal(bits(env_state[k]), bits(model_state[k]), err_msg=f"{what}: {k}")
    for k in ("stocks_tag", "day"):
        np.testing.assert_array_equal(env_state[k], model_state[k], err_msg=f"{what}: {k}")


def assert_step_equal(env, got, want, what=""):
    """(obs, reward, done) tensors of a batched step vs ModelBatch.step's result, and the state."""
    obs, rew, done = (t.cpu().numpy() for t in got[:3])
    m_obs, m_rew, m_done, _ = want
    np.testing.assert_array_equal(done.astype(bool), m_done, err_msg=f"{what}: done")
    np.testing.assert_array_equal(bits(obs), bits(m_obs), err_msg=f"{what}: obs")
    np.testing.assert_array_equal(bits(rew), bits(m_rew.astype(np.float32)), err_msg=f"{what}: reward")
    st = env.state_numpy()
    np.testing.assert_array_equal(bits(st["last_reward"]), bits(m_rew), err_msg=f"{what}: last_reward")
    return st


def assert_terminal_rows(term, want, what=""):
    """The terminal-observation rows of the envs that ModelBatch.step reported done."""
    rows = term.cpu().numpy()
    for e, row in want[3].items():
        np.testing.assert_array_equal(bits(rows[e]), bits(row), err_msg=f"{what}: terminal obs of env {e}")


def replay_recording_with_auto_reset(env, case, to_device, what=""):
    """A fixture case that is one reset and one episode, on every env of a batched env with auto_reset
    on and terminal observations enabled: each env equals the recorded row after every op.  The step
    that ends the episode returns the recorded reward, latches the recorded returns, leaves the
    reference's last observation in the terminal rows, and shows the recorded reset: its observation,
    the initial account, no stocks, tag PY."""
    E = env.num_envs
    term = env.enable_terminal_obs()
    assert case["ops"][0] == OP_RESET and (case["ops"][1:] == OP_STEP).all()
    for i, op in enumerate(case["ops"]):
        msg = f"{what} op {i}"
        fresh = op == OP_RESET or bool(case["done"][i])
        if op == OP_RESET:
            obs = env.reset().cpu().numpy()
        else:
            obs, rew, done, _ = env.step(to_device(np.full((E, 1), case["actions"][i], np.float32)))
            obs = obs.cpu().numpy()
            assert (bits(rew.cpu().numpy()) == bits(np.float32(case["reward"][i]))).all(), msg
            assert (done.cpu().numpy() == case["done"][i]).all(), msg
        assert (bits(obs) == bits(case["obs"][0 if fresh else i])[None, :]).all(), msg
        st = env.state_numpy()
        if op == OP_STEP:
            assert (bits(st["last_reward"]) == bits(case["reward"][i])).all(), msg
        for k in STATE_F64:
            assert (bits(st[k]) == bits(case[k][0 if fresh and k in STATE_F64[:3] else i])).all(), f"{msg}: {k}"
        assert (st["stocks_tag"] == case["tag"][0 if fresh else i]).all(), msg
        assert (st["day"] == (0 if fresh else i)).all(), msg
    assert case["done"][-1] == 1 and case["done"].sum() == 1
    assert (bits(term.cpu().numpy()) == bits(case["obs"][-1])[None, :]).all(), f"{what}: terminal obs"
