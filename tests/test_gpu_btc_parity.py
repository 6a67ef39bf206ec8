"""The batched BitcoinEnv (VecBitcoinEnv, finenv_btc_*) on the MI355X against the recorded reference
runs (tests/golden/btc_*.npz) and against one tests/btc_model.py model per env, bit for bit
(tolerance 0) on observation, reward, done and every state field, the stocks tag included."""
import numpy as np
import pytest

import btc_model as bm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIXTURES = ("btc_basic", "btc_caps", "btc_wide", "btc_modes", "btc_midreset", "btc_draw", "btc_widths",
            "btc_domain")
CASES = [(f, c) for f in FIXTURES for c in bm.load_fixture(f)]
SMALL = dict(initial_account=1e3, transaction_fee_percent=1e-3, gamma=0.99)   # btc_caps: the caps bind


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _panel(rng, T, P, W, price=300.0):
    p0 = price * np.exp(np.cumsum(rng.normal(0, 0.01, T)))
    cols = [p0] + [p0 * (1.003 + 0.002 * k) for k in range(P - 1)]
    return np.ascontiguousarray(np.stack(cols, 1)), rng.normal(0, 3e3, (T, W))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("fixture,case", CASES)
def test_replays_reference_recording(fixture, case):
    """70 envs (one full wave and a 6-lane tail), all on the recorded actions: every env equals the
    reference's recorded row after every reset() and step()."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    c = bm.load_fixture(fixture)[case]
    E = 70
    env = VecBitcoinEnv(c["price_ary"], c["tech_ary"], E, auto_reset=False, **bm.model_kwargs(c["kwargs"]))
    assert env.max_step == int(c["max_step"]) and env.state_dim == int(c["state_dim"])
    assert env.obs_dim == c["obs"].shape[1]
    for i, op in enumerate(c["ops"]):
        what = f"{fixture}/{case} op {i}"
        if op == bm.OP_RESET:
            obs = env.reset().cpu().numpy()
        else:
            obs, rew, done, info = env.step(_dev(np.full((E, 1), c["actions"][i], np.float32)))
            assert info is None
            obs = obs.cpu().numpy()
            assert (bm.bits(rew.cpu().numpy()) == bm.bits(np.float32(c["reward"][i]))).all(), what
            assert (done.cpu().numpy() == c["done"][i]).all(), what
        assert (bm.bits(obs) == bm.bits(c["obs"][i])[None, :]).all(), what
        st = env.state_numpy()
        if op == bm.OP_STEP:
            assert (bm.bits(st["last_reward"]) == bm.bits(c["reward"][i])).all(), what
        for k in bm.STATE_F64:
            assert (bm.bits(st[k]) == bm.bits(c[k][i])).all(), f"{what}: {k}"
        assert (st["stocks_tag"] == c["tag"][i]).all(), what


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "manual"])
@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("E", [1, 70, 259])
def test_random_streams_through_two_episode_ends(E, P, auto_reset):
    """Per-env random actions, small accounts so that every cap binds somewhere in the batch, two
    episode ends: terminal observations, the episode_return latch, and (auto_reset off) the defined
    step past the end, which changes nothing."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    T, W = 13, 7 if P != 2 else 9
    rng = np.random.default_rng(1000 * E + 10 * P + auto_reset)
    price, tech = _panel(rng, T, P, W)
    env = VecBitcoinEnv(price, tech, E, auto_reset=auto_reset, **SMALL)
    term = env.enable_terminal_obs()
    mb = bm.ModelBatch(price, tech, E, **SMALL)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), np.stack(list(mb.reset().values())))
    ends, tags, short, overdrawn = 0, set(), False, False
    for k in range(2 * T + 3):
        a = rng.uniform(-1, 1, E).astype(np.float32)
        got = env.step(_dev(a[:, None]))
        want = mb.step(a, auto_reset)
        st = bm.assert_step_equal(env, got, want, f"step {k}")
        bm.assert_state_equal(st, mb.state(), f"step {k}")
        tags |= set(st["stocks_tag"].tolist())
        short, overdrawn = short or (st["stocks"] < 0).any(), overdrawn or (st["account"] < 0).any()
        obs_now = got[0].clone()
        if want[2].any():
            assert want[2].all()                                  # lock step: everyone ends together
            ends += 1
            np.testing.assert_array_equal(bm.bits(term.cpu().numpy()), bm.bits(np.stack(list(want[3].values()))))
            np.testing.assert_array_equal(env.episode_return().cpu().numpy(),
                                          mb.state()["episode_return"].astype(np.float32))
            if not auto_reset:
                before = {k_: v.clone() for k_, v in env.state.items()}
                again = env.step(_dev(a[:, None]))                # past the end: defined, no trade
                st2 = bm.assert_step_equal(env, again, mb.step(a, False), f"past the end {k}")
                assert (again[1] == 0).all() and again[2].all()
                np.testing.assert_array_equal(bm.bits(again[0].cpu().numpy()), bm.bits(obs_now.cpu().numpy()))
                for k_, v in before.items():
                    if k_ != "last_reward":
                        assert torch.equal(env.state[k_], v), k_
                assert (st2["last_reward"] == 0).all()
                obs = env.reset().cpu().numpy()
                np.testing.assert_array_equal(obs, np.stack(list(mb.reset().values())))
                bm.assert_state_equal(env.state_numpy(), mb.state(), "after reset")
    assert ends >= 2
    if E >= 70:                                                   # the rules were reached in the batch
        assert {bm.F32, bm.F64} <= tags and short and overdrawn


def test_masked_resets_leave_a_wave_on_different_days():
    """Masked resets in mid episode: the envs of one wave then stand on different panel rows, end
    their episodes in different steps, and gamma_return survives the reset."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    E, T, P = 70, 12, 1
    rng = np.random.default_rng(7)
    price, tech = _panel(rng, T, P, 7)
    env = VecBitcoinEnv(price, tech, E, auto_reset=True, **SMALL)
    term = env.enable_terminal_obs()
    mb = bm.ModelBatch(price, tech, E, **SMALL)
    env.reset()
    mb.reset()
    partial, spread = 0, 0
    for k in range(3 * T):
        a = rng.uniform(-1, 1, E).astype(np.float32)
        got = env.step(_dev(a[:, None]))
        want = mb.step(a, True)
        st = bm.assert_step_equal(env, got, want, f"step {k}")
        bm.assert_state_equal(st, mb.state(), f"step {k}")
        for e, row in want[3].items():
            np.testing.assert_array_equal(bm.bits(term[e].cpu().numpy()), bm.bits(row))
        partial += int(want[2].any() and not want[2].all())
        spread = max(spread, len(np.unique(st["day"][:64])))
        if k in (3, 8, 17):
            mask = rng.random(E) < 0.4
            keep = env.obs.clone()
            g_before = env.state["gamma_return"].clone()
            obs = env.reset(_dev(mask.astype(np.uint8))).cpu().numpy()
            for e, row in mb.reset(mask).items():
                np.testing.assert_array_equal(bm.bits(obs[e]), bm.bits(row))
            np.testing.assert_array_equal(obs[~mask], keep.cpu().numpy()[~mask])   # other rows untouched
            assert torch.equal(env.state["gamma_return"], g_before) and (g_before != 0).any()
            bm.assert_state_equal(env.state_numpy(), mb.state(), f"masked reset {k}")
    assert partial >= 3 and spread >= 4


def test_step_into_an_unaligned_slice_of_a_rollout_tensor():
    """out = slice 1 of a [2, 70, 11] tensor: its rows start 8 bytes off a 16-byte boundary, so the
    full wave takes the dword path; slice 0 stays untouched."""
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    E, T, P = 70, 10, 2
    rng = np.random.default_rng(3)
    price, tech = _panel(rng, T, P, 7)
    env = VecBitcoinEnv(price, tech, E, auto_reset=True, **SMALL)
    mb = bm.ModelBatch(price, tech, E, **SMALL)
    env.reset()
    mb.reset()
    buf = torch.full((2, E, P + 9), -7.0, device="cuda")
    rew = torch.zeros(2, E, device="cuda")
    done = torch.zeros(2, E, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and buf[1].data_ptr() % 16 == 8
    own = env.obs.clone()
    for k in range(T + 2):
        a = rng.uniform(-1, 1, E).astype(np.float32)
        got = env.step(_dev(a[:, None]), out=(buf[1], rew[1], done[1]))
        assert got[0].data_ptr() == buf[1].data_ptr()
        bm.assert_state_equal(bm.assert_step_equal(env, got, mb.step(a, True), f"step {k}"), mb.state())
    assert (buf[0] == -7.0).all() and (rew[0] == 0).all() and torch.equal(env.obs, own)


def test_captured_step_replays_over_an_episode_end():
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    E, T, P = 70, 9, 1
    rng = np.random.default_rng(5)
    price, tech = _panel(rng, T, P, 7)
    env = VecBitcoinEnv(price, tech, E, auto_reset=True, **SMALL)
    env.enable_terminal_obs()
    mb = bm.ModelBatch(price, tech, E, **SMALL)
    env.reset()
    mb.reset()
    a_in = torch.zeros(E, 1, device="cuda")
    outs = {}

    def body():
        outs["got"] = env.step(a_in)

    def follow(a, what):
        torch.cuda.synchronize()
        want = mb.step(a, True)
        bm.assert_state_equal(bm.assert_step_equal(env, outs["got"], want, what), mb.state(), what)
        return bool(want[2].all())

    body()
    ends = follow(np.zeros(E, np.float32), "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for k in range(2 * T):
        a = rng.uniform(-1, 1, E).astype(np.float32)
        a_in.copy_(_dev(a[:, None]))
        graph.replay()
        ends += follow(a, f"replay {k}")
    assert ends >= 2


def test_wrong_action_dtypes_raise():
    _need_gpu()
    from finrl_amd.vec_btc import VecBitcoinEnv
    price, tech = _panel(np.random.default_rng(0), 6, 1, 7)
    env = VecBitcoinEnv(price, tech, 4)
    env.reset()
    before = {k: v.clone() for k, v in env.state.items()}
    for bad in (torch.zeros(4, 1, dtype=torch.float64, device="cuda"), np.zeros((4, 1)),
                torch.zeros(4, 1, dtype=torch.float16, device="cuda"), [0.0] * 4):
        with pytest.raises(TypeError):
            env.step(bad)
    with pytest.raises(ValueError):
        env.step(torch.zeros(5, 1, device="cuda"))
    for k, v in before.items():
        assert torch.equal(env.state[k], v), k
    env.step(torch.zeros(4, device="cuda"))                       # [E] is taken as [E, 1]
