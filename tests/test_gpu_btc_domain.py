"""The value domain of the batched BitcoinEnv step (include/finenv.h, "Action and panel domain" of the
BitcoinEnv block) on the MI355X: finite positive prices from 1e-4 to 1e8, accounts from 1e2 to 1e12 and
ANY float32 action -- +-0, denormals, the largest finite values, +-inf, NaN, values far past +-1 --
against one tests/btc_model.py model per env and the recorded reference runs of btc_domain, bit for bit
(tolerance 0; tests/test_btc_model.py pins the model to the same recordings).

What the cases must contain is decided on the model's states and observations alone
(test_the_cases_contain_their_events, which needs no device): a case that loses its events fails
instead of testing less."""
import functools

import numpy as np
import pytest

import btc_model as bm

torch = pytest.importorskip("torch")

DEV = "cuda"
E, T = 70, 24
STEPS = 2 * (T - 1)                                   # two episode ends, in lock step
# (price level, initial account, P): the grid of btc_domain, and the widest row on everyday values
CASES = [(1e-4, 1e2, 1), (1e-4, 1e12, 1), (300.0, 1e3, 1), (3e4, 1e6, 1), (1e8, 1e2, 1), (1e8, 1e12, 1),
         (300.0, 1e3, 245)]
IDS = [f"price{p:g}-account{a:g}-P{P}" for p, a, P in CASES]
DOMAIN_CASES = list(bm.load_fixture("btc_domain"))
F32_MIN_NORMAL = 2.0 ** -126


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _panel(rng, level, P):
    p0 = level * np.exp(np.cumsum(rng.normal(0, 0.01, T)))
    cols = [p0] + [p0 * (1.003 + 0.002 * k) for k in range(P - 1)]
    return np.ascontiguousarray(np.stack(cols, 1)), rng.normal(0, 3e3, (T, 7))


def _streams(rng):
    """f32 [STEPS, E]: uniform(-1, 1) * 10^k, k in -3 .. 3, and every special value once per env at the
    env's own random steps; env e < 16 takes special e in its first step, fresh from reset()."""
    a = (rng.uniform(-1, 1, (STEPS, E)) * 10.0 ** rng.integers(-3, 4, (STEPS, E))).astype(np.float32)
    n = len(bm.SPECIAL_ACTIONS)
    for e in range(E):
        if e < n:
            at = np.concatenate(([0], 1 + rng.permutation(STEPS - 1)[:n - 1]))
            a[at, e] = np.roll(bm.SPECIAL_ACTIONS, -e)
        else:
            a[rng.permutation(STEPS)[:n], e] = bm.SPECIAL_ACTIONS
    return a


def _same(a, s):
    return bm.bits(a) == bm.bits(np.float32(s))[0]


@functools.lru_cache(maxsize=None)
def _expected(i):
    """Case i on the model alone -> (panel, actions, reset rows, per-step (want, state), events).  The
    model raises nothing and every state field, reward and observation is finite in every step: the
    precondition of comparing at tolerance 0 (include/finenv.h keeps non-finite values out of the
    domain)."""
    level, account, P = CASES[i]
    rng = np.random.default_rng(50 + i)
    price, tech = _panel(rng, level, P)
    actions = _streams(rng)
    kw = dict(initial_account=account, transaction_fee_percent=1e-3, gamma=0.99)
    mb = bm.ModelBatch(price, tech, E, **kw)
    first = np.stack(list(mb.reset().values()))
    ev = dict(tags=set(), short=False, overdrawn=False, short_cap=False, buy_cap=False, denormal_obs=False,
              denormal_stocks=False, ends=0, met=np.zeros((len(bm.SPECIAL_ACTIONS), 4), bool))
    steps = []
    for k in range(STEPS):
        a, pre = actions[k], mb.state()
        adj, a64 = price[pre["day"], 0], actions[k].astype(np.float64)
        cap = 0.5 * pre["total_asset"] / adj + pre["stocks"]
        ev["short_cap"] |= bool(((a64 < 0) & (cap > 0) & (cap < -a64)).any())
        ev["buy_cap"] |= bool(((a64 > 0) & (pre["account"] / adj < a64)).any())
        met = np.stack([pre["stocks"] > 0, pre["stocks"] < 0, pre["account"] < 0, pre["stocks_tag"] == bm.PY], 1)
        for j, s in enumerate(bm.SPECIAL_ACTIONS):
            ev["met"][j] |= met[_same(a, s)].any(0)
        want = mb.step(a, True)
        st = mb.state()
        for name in bm.STATE_F64:
            assert np.isfinite(st[name]).all(), f"{IDS[i]} step {k}: {name}"
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all(), f"{IDS[i]} step {k}"
        assert all(np.isfinite(row).all() for row in want[3].values())
        assert want[2].all() or not want[2].any()
        ev["ends"] += int(want[2].all())
        ev["tags"] |= set(st["stocks_tag"].tolist())
        ev["short"] |= bool((st["stocks"] < 0).any())
        ev["overdrawn"] |= bool((st["account"] < 0).any())
        ev["denormal_obs"] |= bool(((want[0] != 0) & (np.abs(want[0]) < F32_MIN_NORMAL)).any())
        ev["denormal_stocks"] |= bool(((st["stocks_tag"] == bm.F32) & (st["stocks"] != 0) &
                                       (np.abs(st["stocks"]) < F32_MIN_NORMAL)).any())
        steps.append((want, st))
    return price, tech, kw, actions, first, steps, ev


def test_the_cases_contain_their_events():
    """On the model alone.  Every case: two episode ends, and every special action in every env's
    stream.  Over the file: all three tags, short and overdrawn states, both caps binding, a nonzero
    float32 denormal in an observation and one held as `stocks` under tag F32 -- what a flush to zero in
    the float32 add of `stocks` or in the observation's double-to-float conversion would lose --, and
    every special action met by a long, a short, an overdrawn and a fresh-from-reset env."""
    evs = []
    for i in range(len(CASES)):
        actions, ev = _expected(i)[3], _expected(i)[6]
        assert ev["ends"] == 2, IDS[i]
        for s in bm.SPECIAL_ACTIONS:
            assert _same(actions, s).any(0).all(), (IDS[i], s)
        evs.append(ev)
    assert set().union(*(ev["tags"] for ev in evs)) == {bm.PY, bm.F32, bm.F64}
    for name in ("short", "overdrawn", "short_cap", "buy_cap", "denormal_obs", "denormal_stocks"):
        assert any(ev[name] for ev in evs), name
    met = np.logical_or.reduce([ev["met"] for ev in evs])
    assert met.all(), met


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_special_actions_over_price_levels_and_accounts(i):
    """70 envs, each on its own action stream, auto_reset on, two episode ends."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    price, tech, kw, actions, first, steps, _ = _expected(i)
    env = VecBitcoinEnv(price, tech, E, auto_reset=True, **kw)
    term = env.enable_terminal_obs()
    np.testing.assert_array_equal(bm.bits(env.reset().cpu().numpy()), bm.bits(first))
    for k, (want, state) in enumerate(steps):
        st = bm.assert_step_equal(env, env.step(_dev(actions[k][:, None])), want, f"step {k}")
        bm.assert_state_equal(st, state, f"step {k}")
        bm.assert_terminal_rows(term, want, f"step {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", DOMAIN_CASES)
def test_replays_the_recorded_domain(case):
    """70 envs on the recorded actions of the reference env at each price level and account,
    auto_reset on: every env equals the reference's recorded row after every op."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    c = bm.load_fixture("btc_domain")[case]
    env = VecBitcoinEnv(c["price_ary"], c["tech_ary"], 70, auto_reset=True, **bm.model_kwargs(c["kwargs"]))
    assert env.max_step == int(c["max_step"]) and env.obs_dim == c["obs"].shape[1]
    bm.replay_recording_with_auto_reset(env, c, _dev, f"btc_domain/{case}")
