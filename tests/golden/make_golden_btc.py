"""Records runs of the UNMODIFIED reference BitcoinEnv
(finrl/meta/env_cryptocurrency_trading/env_btc_ccxt.py) into tests/golden/btc_*.npz.

Runs only where the reference tree exists (FINRL_REFERENCE_ROOT names its checkout); the
module is loaded by path and needs nothing but NumPy (matplotlib for btc_draw).  The fixtures hold
data only -- inputs, constructor keywords, the NumPy version and, per reset() / step(), what the
reference returned and held -- no reference source.  Layout: tests/btc_model.py load_fixture.

    python tests/golden/make_golden_btc.py [fixture ...]
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from btc_model import (OP_RESET, OP_STEP, RECORDED, SPECIAL_ACTIONS, StubArgs, StubTorch,  # noqa: E402
                       bits, tag_of)

REFERENCE_ROOT = os.environ.get("FINRL_REFERENCE_ROOT")


def reference_class():
    if not REFERENCE_ROOT:
        sys.exit("set FINRL_REFERENCE_ROOT to a checkout of the reference tree")
    path = os.path.join(REFERENCE_ROOT, "finrl", "meta", "env_cryptocurrency_trading", "env_btc_ccxt.py")
    spec = importlib.util.spec_from_file_location("ref_env_btc_ccxt", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.BitcoinEnv


def panel(rng, T, P, W, price=300.0, vol=0.01):
    p0 = price * np.exp(np.cumsum(rng.normal(0, vol, T)))
    cols = [p0] + [p0 * (1 + 0.002 * (k + 1) + rng.normal(0, 0.001, T)) for k in range(P - 1)]
    tech = rng.normal(0, 1, (T, W)) * np.array([1.0, 3e4, 3e4, 50.0, 50.0, 3e4, 3e4] + [7.0] * (W - 7))
    return np.ascontiguousarray(np.stack(cols, 1)), np.ascontiguousarray(tech)


class Recorder:
    """Drives one reference env and keeps one row per op."""

    def __init__(self, env, kwargs):
        self.env, self.kwargs = env, kwargs
        self.rows = {k: [] for k in RECORDED + ("ops", "actions")}
        self.branches = dict(short_cap=0, zero_sell=0, buy_cap=0, negative_buy=0)

    def _keep(self, op, action, obs, reward, done):
        e = self.env
        assert obs.dtype == np.float32
        vals = dict(ops=op, actions=action, obs=obs, reward=reward, done=done, account=e.account,
                    stocks=e.stocks, tag=tag_of(e.stocks), total_asset=e.total_asset,
                    gamma_return=e.gamma_return, episode_return=e.episode_return)
        for k, v in vals.items():
            self.rows[k].append(v)

    def reset(self):
        self._keep(OP_RESET, np.float32(0), self.env.reset(), np.nan, False)

    def step(self, a):
        e = self.env
        a = np.float32(a)
        adj = e.day_price[0]                                  # which branch this step takes
        if a < 0:
            cap = 0.5 * e.total_asset / adj + e.stocks
            self.branches["short_cap"] += bool(0 < cap < -a)
            self.branches["zero_sell"] += bool(cap <= 0)
        elif a > 0:
            self.branches["buy_cap"] += bool(e.account / adj < a)
            self.branches["negative_buy"] += bool(e.account < 0)
        obs, reward, done, info = e.step(np.array([a], dtype=np.float32))
        assert info is None and type(reward) is np.float64 and type(e.account) is np.float64 and \
            type(e.total_asset) is np.float64
        self._keep(OP_STEP, a, obs, reward, done)
        return done

    def episode(self, actions):
        for a in actions:
            if self.step(a):
                return
        raise AssertionError("episode did not end")

    def arrays(self, prefix):
        e = self.env
        out = {f"{prefix}.kwargs": np.array(json.dumps(self.kwargs)),
               f"{prefix}.price_ary": e.price_ary, f"{prefix}.tech_ary": e.tech_ary,
               f"{prefix}.state_dim": np.int64(e.state_dim), f"{prefix}.max_step": np.int64(e.max_step)}
        dt = dict(ops=np.int8, actions=np.float32, obs=np.float32, done=np.uint8, tag=np.int8)
        for k, v in self.rows.items():
            out[f"{prefix}.{k}"] = np.asarray(v, dtype=dt.get(k, np.float64))
        return out


def make(Env, price, tech, **kwargs):
    return Recorder(Env(price_ary=price, tech_ary=tech, **kwargs), kwargs)


def reaches(recs, specials=()):
    """What a whole fixture (its Recorders) must contain: every cap branch at least twice, all three
    stocks tags, and every special action, by its bits, on a recorded step -- episode() stops at done,
    so no recorded step is past the end.  Every recorded number must be finite."""
    for r in recs:
        steps = np.asarray(r.rows["ops"]) == OP_STEP
        for k in RECORDED:
            v = np.asarray(r.rows[k], np.float64)
            assert np.isfinite(v[steps] if k == "reward" else v).all(), k
    applied = {int(bits(np.float32(a))[0]) for r in recs for a, op in zip(r.rows["actions"], r.rows["ops"])
               if op == OP_STEP}
    return min(sum(r.branches[k] for r in recs) for k in recs[0].branches) >= 2 and \
        set().union(*(r.rows["tag"] for r in recs)) == {0, 1, 2} and \
        all(int(bits(np.float32(s))[0]) in applied for s in specials)


def actions_for(rng, env, scale=1.0):
    return (rng.uniform(-1, 1, env.max_step - 1) * scale).astype(np.float32)


# the whole array as the train slice, no subsampling
WHOLE = dict(time_frequency=1, start=None, mid1=None, mid2=0, end=0, mode="train")


def btc_basic(Env):
    rng = np.random.default_rng(11)
    price, tech = panel(rng, 40, 1, 7, price=30000.0)
    r = make(Env, price, tech, **WHOLE)
    for _ in range(2):                                    # two episodes, reset() between
        r.reset()
        r.episode(actions_for(rng, r.env))
    assert not any(r.branches.values()), r.branches       # no cap binds ...
    assert set(r.rows["tag"]) == {0, 1}                   # ... and stocks stays float32
    return {"basic": r}


def btc_caps(Env):
    for seed in range(64):
        rng = np.random.default_rng(seed)
        price, tech = panel(rng, 60, 1, 7)
        r = make(Env, price, tech, initial_account=1e3, **WHOLE)
        r.reset()
        r.episode(actions_for(rng, r.env))
        tags = [t for i, t in enumerate(r.rows["tag"]) if i == 0 or t != r.rows["tag"][i - 1]]
        if min(r.branches[k] for k in ("short_cap", "zero_sell", "buy_cap")) >= 2 and \
                r.branches["negative_buy"] >= 1 and tags == [0, 1, 2]:
            print("  btc_caps: seed", seed, r.branches)
            return {"caps": r}
    raise AssertionError("no seed takes each cap branch twice")


def btc_wide(Env):
    rng = np.random.default_rng(5)
    out = {}
    for name, P, W in (("p3w9", 3, 9), ("p2w7", 2, 7)):
        price, tech = panel(rng, 30, P, W)
        r = make(Env, price, tech, initial_account=2e3, **WHOLE)
        r.reset()
        r.episode(actions_for(rng, r.env))
        assert r.env.state_dim == 2 + P + W
        out[name] = r
    return out


def btc_modes(Env):
    rng = np.random.default_rng(8)
    price, tech = panel(rng, 83, 2, 8)
    split = dict(time_frequency=3, start=4, mid1=37, mid2=59, end=-2)
    out, raw = {}, {}
    for mode in ("train", "test", "trade"):
        r = make(Env, price, tech, initial_account=5e3, mode=mode, **split)
        r.reset()
        r.episode(actions_for(rng, r.env))
        out[mode] = r
        raw[f"{mode}.raw_price"], raw[f"{mode}.raw_tech"] = price, tech
    try:
        Env(price_ary=price, tech_ary=tech, mode="live", **split)
        raise AssertionError("an invalid mode did not raise")
    except ValueError as e:
        assert str(e) == "Invalid Mode!"
    return out, raw


def btc_midreset(Env):
    rng = np.random.default_rng(21)
    price, tech = panel(rng, 32, 1, 7)
    r = make(Env, price, tech, initial_account=1e3, **WHOLE)
    r.reset()
    for a in actions_for(rng, r.env)[:11]:
        r.step(a)
    assert r.env.gamma_return != 0.0
    r.reset()                                             # mid-episode: gamma_return survives
    assert r.rows["gamma_return"][-1] == r.rows["gamma_return"][-2] != 0.0
    r.episode(actions_for(rng, r.env))
    return {"midreset": r}


def btc_draw(Env):
    rng = np.random.default_rng(3)
    price, tech = panel(rng, 36, 1, 7)
    r = make(Env, price, tech, initial_account=5e5, **WHOLE)
    r.reset()                                             # (one recorded row: the layout needs one)
    import matplotlib
    matplotlib.use("Agg")
    with tempfile.TemporaryDirectory() as cwd:
        args = StubArgs(cwd)
        episode_returns, btc_returns = r.env.draw_cumulative_return(args, StubTorch)
        assert os.path.exists(os.path.join(cwd, "cumulative_return.jpg"))
    assert args.agent.inited == (16, r.env.state_dim, 1)
    extra = {"draw.episode_returns": np.asarray(episode_returns, np.float64),
             "draw.btc_returns": np.asarray(btc_returns, np.float64)}
    return {"draw": r}, extra


# (P, W) of btc_widths: D = P + 9 = 62, 63, 126, 127, 254 -- both edges of the kernel's three launch
# forms; price level x initial account of btc_domain, both extremes of each
WIDTHS = ((53, 7), (54, 9), (117, 12), (118, 7), (245, 7))
DOMAIN = ((1e-4, 1e2), (1e-4, 1e12), (300.0, 1e3), (3e4, 1e6), (1e8, 1e2), (1e8, 1e12))


def btc_widths(Env):
    for seed in range(256):
        rng = np.random.default_rng(seed)
        out = {}
        for P, W in WIDTHS:
            price, tech = panel(rng, 8, P, W)
            r = make(Env, price, tech, initial_account=1e3, **WHOLE)
            r.reset()
            r.episode(actions_for(rng, r.env, scale=2.0))
            assert r.env.state_dim == 2 + P + W and r.rows["obs"][0].shape == (P + 9,)
            out[f"p{P}w{W}"] = r
        if reaches(list(out.values())):
            print("  btc_widths: seed", seed)
            return out
    raise AssertionError("no seed takes each cap branch twice")


def domain_actions(rng, n):
    """uniform(-1, 1) * 10^k, k in -3 .. 3 drawn per step, and every special value on one step."""
    a = (rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    a[rng.permutation(n)[:len(SPECIAL_ACTIONS)]] = SPECIAL_ACTIONS
    return a


def btc_domain(Env):
    for seed in range(256):
        rng = np.random.default_rng(seed)
        out = {}
        for level, account in DOMAIN:
            price, tech = panel(rng, 40, 1, 7, price=level)
            r = make(Env, price, tech, initial_account=account, **WHOLE)
            r.reset()
            with warnings.catch_warnings():               # the reference warns of nothing in the domain
                warnings.simplefilter("error")
                r.episode(domain_actions(rng, r.env.max_step - 1))
            out[f"price{level:g}_account{account:g}"] = r
        if reaches(list(out.values()), SPECIAL_ACTIONS):
            print("  btc_domain: seed", seed)
            return out
    raise AssertionError("no seed reaches every branch, tag and special action")


FIXTURES = dict(btc_basic=btc_basic, btc_caps=btc_caps, btc_wide=btc_wide, btc_modes=btc_modes,
                btc_midreset=btc_midreset, btc_draw=btc_draw, btc_widths=btc_widths, btc_domain=btc_domain)


def main(names):
    Env = reference_class()
    for name in names:
        got = FIXTURES[name](Env)
        cases, extra = got if isinstance(got, tuple) else (got, {})
        arrays = {"cases": np.array(json.dumps(list(cases))), "numpy_version": np.array(np.__version__)}
        for prefix, rec in cases.items():
            arrays.update(rec.arrays(prefix))
        arrays.update(extra)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {os.path.getsize(path)} bytes, cases {list(cases)}")


if __name__ == "__main__":
    main(sys.argv[1:] or list(FIXTURES))
