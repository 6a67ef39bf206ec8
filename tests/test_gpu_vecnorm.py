"""VecNormalize / RunningMeanStd on the MI355X against the NumPy model (tests/vecnorm_model.py): the
column moments at every lane layout and several tiles, the apply formula with tolerance 0, the step
order against unwrapped twin envs, frozen and switched-off modes, graph replay, the buffers, and the
state dict.

Tolerances of the moments (float64 sums of at most 70,001 shifted terms in any order: the error is at
most n * 2^-53 relative to sum (x-K)^2, which is at most about 50 * n * var for data within 7 sigma --
about 4e-10; 1e-8 leaves a margin of 25): var at rtol 1e-8, mean at atol 1e-8 * sigma (1e-8 * |mean|
for a constant column), count exact.  A plain sum of x^2 misses this on the 1e6 column by orders of
magnitude."""
import numpy as np
import pytest

import vecnorm_model as vm
from replay_cases import need_gpu
from vecnorm_cases import gaussian_columns

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -7777.0
ROWS = (1, 70, 259, 70001)
DIMS = ((1, 1), (3, 3), (291, 291), (291, 304), (1001, 1001))      # (dim, row pitch)


def on_device(x, pitch, fill=float("nan")):
    """x [n, dim] as a device view with rows `pitch` floats apart (the pad holds `fill`) -> (view, backing)."""
    n, dim = x.shape
    back = torch.full((n, pitch), fill, dtype=torch.float32, device="cuda")
    back[:, :dim].copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return back[:, :dim], back


def host(t):
    return t.detach().cpu().numpy()


def assert_stats(rms, model, sigma, tag):
    """Device stats against the model at the tolerances of the module docstring; scale from var."""
    mean, var = host(rms.mean), host(rms.var)
    atol = 1e-8 * np.where(sigma > 0, sigma, np.abs(model.mean))
    err = np.abs(mean - model.mean)
    assert (err <= atol).all(), f"mean {tag}: column {np.argmax(err - atol)} off by {err.max()}"
    np.testing.assert_allclose(var, model.var, rtol=1e-8, atol=0, err_msg=f"var {tag}")
    assert host(rms.count)[0] == model.count, f"count {tag}"
    np.testing.assert_allclose(host(rms.scale), 1 / np.sqrt(var + rms.epsilon), rtol=1e-15, atol=0,
                               err_msg=f"scale {tag}")        # sqrt and division, each within an ulp
    assert int(rms._ticket.item()) == 0, f"ticket {tag}"


@pytest.mark.parametrize("dim,pitch", DIMS)
@pytest.mark.parametrize("n", ROWS)
def test_moments_equal_model(n, dim, pitch):
    """One update, then two more with other row counts (a prefix and a suffix of the same rows), each
    against the model; the first update repeated from the same state gives identical bits."""
    need_gpu()
    from finrl_amd import RunningMeanStd
    x, sigma = gaussian_columns(n, dim)
    xd, _ = on_device(x, pitch)
    rms, model = RunningMeanStd(dim), vm.RunningMeanStd(dim)
    start = rms._block.clone()
    rms.update(xd)
    first = rms._block[:3 * dim + 1].clone()
    model.update(x)
    assert_stats(rms, model, sigma, "after one update")
    if dim > 1:
        assert host(rms.mean)[-1] == model.mean[-1]          # the constant column: the same roundings on both sides

    rms._block.copy_(start)
    rms.update(xd)
    assert torch.equal(rms._block[:3 * dim + 1].view(torch.int64), first.view(torch.int64))

    for lo, hi in ((0, n // 2 + 1), (n // 3, n)):
        rms.update(xd[lo:hi])
        model.update(x[lo:hi])
    assert_stats(rms, model, sigma, "after three updates")


def test_a_plain_sum_of_squares_would_miss_the_tolerance():
    """The reason for the shifted sums, on the 1e6 column: E[x^2] - E[x]^2 in float64 is off by far more
    than rtol 1e-8 of a variance of 1."""
    x = gaussian_columns(70001, 3)[0][:, 0].astype(np.float64)
    plain = (x * x).sum() / len(x) - (x.sum() / len(x)) ** 2
    assert abs(plain - x.var()) > 1e-6 * x.var()


APPLY_CASES = [  # n, dim, pitch in, pitch out
    (1, 3, 3, 3), (259, 3, 3, 5), (259, 291, 291, 291), (259, 291, 304, 304), (70, 291, 304, 291),
    (70, 291, 291, 304), (1, 291, 304, 304), (259, 1, 1, 1), (70, 1001, 1001, 1004)]


def special_rows(x):
    """x with a NaN, both infinities, both zeros and values far past both clip bounds spread over it."""
    x = x.copy()
    flat = x.reshape(-1)
    idx = np.linspace(0, flat.size - 1, num=min(flat.size, 9)).astype(int)
    vals = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, -1e30, 0.0, -0.0]
    for i, v in zip(idx, vals):
        flat[i] = v
    return x


@pytest.mark.parametrize("n,dim,pin,pout", APPLY_CASES)
def test_apply_equals_formula(n, dim, pin, pout):
    need_gpu()
    from finrl_amd import RunningMeanStd
    base, _ = gaussian_columns(259 if n <= 259 else n, dim)
    rms = RunningMeanStd(dim, clip=2.5)
    rms.update(on_device(base, dim)[0])
    mean, scale = host(rms.mean), host(rms.scale)
    x = special_rows(np.array(base[:n]))
    if dim >= 3 and n >= 2:                  # finite values four clips out on either side of the mean
        x[1, 1] = np.float32(mean[1] + 2.5 / scale[1] * 4)
        x[1, 2] = np.float32(mean[2] - 2.5 / scale[2] * 4)
    xd, _ = on_device(x, pin)
    for center in (True, False):
        out, back = on_device(np.zeros((n, dim), np.float32), pout, fill=SENTINEL)
        back.fill_(SENTINEL)
        got = rms.apply(xd, out, center=center)
        assert got is out
        want = vm.apply(x, mean, scale, 2.5, center=center)
        np.testing.assert_array_equal(host(out), want, err_msg=f"center={center}")
        assert (back[:, dim:] == SENTINEL).all()
        assert np.isnan(want).sum() >= 1 and (want == 2.5).any() and (want == -2.5).any()
    assert torch.equal(rms.mean, torch.from_numpy(mean).cuda())          # apply never touches the stats

    inplace, back = on_device(x, pin, fill=SENTINEL)                      # out == x, equal pitches
    rms.apply(inplace, inplace)
    np.testing.assert_array_equal(host(inplace), vm.apply(x, mean, scale, 2.5))
    assert (back[:, dim:] == SENTINEL).all()
    fresh = rms.apply(xd)                                                 # allocates a packed output
    np.testing.assert_array_equal(host(fresh), vm.apply(x, mean, scale, 2.5))


def test_apply_from_an_unaligned_base_takes_the_dword_path():
    need_gpu()
    from finrl_amd import RunningMeanStd
    x, _ = gaussian_columns(259, 291)
    rms = RunningMeanStd(291)
    back = torch.full((259 * 292 + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    xd = back[1:].view(259, 292)[:, :291]                                 # 4 bytes past the allocation
    xd.copy_(torch.from_numpy(x))
    rms.update(xd)
    model = vm.RunningMeanStd(291)
    model.update(x)
    np.testing.assert_allclose(host(rms.var), model.var, rtol=1e-8)
    rms.apply(xd, xd)
    np.testing.assert_array_equal(host(xd), vm.apply(x, host(rms.mean), host(rms.scale), 10.0))
    assert back[0].item() == SENTINEL and (back[1:].view(259, 292)[:, 291] == SENTINEL).all()


# ------------------------------------------------------------------------------------ envs
def crypto_env(E):
    from finrl_amd.vec_crypto import VecCryptoEnv
    rng = np.random.default_rng(E)
    T, N, W = 6, 2, 3
    price = 10.0 ** rng.uniform(1, 4, N) * np.exp(np.cumsum(rng.normal(0, 0.004, (T, N)), axis=0))
    return VecCryptoEnv({"price_array": price, "tech_array": rng.normal(0, 3000, (T, W))}, E, lookback=1)


def stock_env(E):
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    rng = np.random.default_rng(E)
    T, N, K = 6, 5, 3
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    panel = StockPanel(close, rng.normal(0, 1, (T, K, N)), np.abs(rng.normal(0, 30, T)))
    return VecStockTradingEnv(panel, E, hmax=100, initial_amount=100_000, turbulence_threshold=40.0)


ENVS = {"crypto": crypto_env, "stock": stock_env}


def actions_for(env, steps, seed=0):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return [torch.rand(env.num_envs, env.action_dim, generator=gen, device="cuda") * 2 - 1
            for _ in range(steps)]


def seen_sigma(rows):
    """Per column: the standard deviation of every raw row seen so far (0: constant so far)."""
    return np.concatenate(rows).astype(np.float64).std(axis=0)


@pytest.mark.parametrize("E", (70, 259))
@pytest.mark.parametrize("kind", sorted(ENVS))
def test_step_against_twin_env(kind, E):
    """Eight steps through an episode end: the wrapper over one env, the model fed an unwrapped twin's
    raw outputs.  Stats at the moments' tolerances, outputs against the apply formula on the device
    stats with tolerance 0, returns exact, done and the raw tensors passed through."""
    need_gpu()
    from finrl_amd import VecNormalize
    env, twin = ENVS[kind](E), ENVS[kind](E)
    norm = VecNormalize(env, gamma=0.97, clip_obs=5.0, clip_reward=3.0)
    D = env.obs.shape[1]
    assert (norm.num_envs, norm.action_dim, norm.device) == (E, env.action_dim, env.device)
    assert norm.auto_reset and norm.supports_record is False and norm.state is env.state
    model = vm.VecNormalize(E, D, gamma=0.97, clip_obs=5.0, clip_reward=3.0)

    def check(obs, raw, tag):
        assert_stats(norm.obs_rms, model.obs_rms, seen_sigma(obs_rows), f"obs {tag}")
        np.testing.assert_array_equal(
            host(obs), vm.apply(raw, host(norm.obs_rms.mean), host(norm.obs_rms.scale), 5.0), err_msg=tag)
        np.testing.assert_array_equal(host(norm.get_original_obs()), raw, err_msg=tag)
        np.testing.assert_array_equal(host(norm.returns), model.returns, err_msg=f"returns {tag}")

    raw = host(twin.reset())
    obs_rows, ret_rows = [raw], []
    obs = norm.reset()
    model.reset(raw)
    assert obs.data_ptr() == norm.obs.data_ptr()
    check(obs, raw, "reset")
    dones = ran_on = 0
    for t, a in enumerate(actions_for(env, 8)):
        raw, raw_r, raw_d = (host(x).copy() for x in twin.step(a)[:3])
        obs, rew, done, info = norm.step(a)
        assert info is None and done is env.done and rew is norm.reward
        pre_zero = model.returns * 0.97 + raw_r.astype(np.float64)
        model.step(raw, raw_r, raw_d)
        obs_rows.append(raw)
        ret_rows.append(pre_zero[:, None])
        check(obs, raw, f"step {t}")
        assert_stats(norm.ret_rms, model.ret_rms, seen_sigma(ret_rows), f"ret step {t}")
        np.testing.assert_array_equal(
            host(rew), vm.apply(raw_r, 0.0, host(norm.ret_rms.scale)[0], 3.0, center=False))
        np.testing.assert_array_equal(host(done), raw_d)
        np.testing.assert_array_equal(host(norm.get_original_reward()), raw_r)
        assert (host(norm.returns)[raw_d.astype(bool)] == 0).all()
        dones += int(raw_d.sum())
        ran_on += int((model.returns != 0).sum())
    assert dones >= E and ran_on                               # an episode ended, and returns ran on

    # reset(mask): returns zeroed under the mask, normalised without an update
    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")
    mask[::3] = 1
    before = norm.obs_rms._block[:3 * D + 1].clone()
    obs = norm.reset(mask)
    raw = host(twin.reset(mask))
    assert torch.equal(norm.obs_rms._block[:3 * D + 1].view(torch.int64), before.view(torch.int64))
    np.testing.assert_array_equal(host(obs), vm.apply(raw, host(norm.obs_rms.mean), host(norm.obs_rms.scale), 5.0))
    want = model.returns.copy()
    want[::3] = 0
    np.testing.assert_array_equal(host(norm.returns), want)


def stats_bits(norm):
    return torch.cat([norm.obs_rms._block[:3 * norm.obs_dim + 1], norm.ret_rms._block[:4]]).view(torch.int64).clone()


def test_frozen_and_switched_off_modes():
    need_gpu()
    from finrl_amd import VecNormalize
    E = 70
    env, twin = crypto_env(E), crypto_env(E)
    norm = VecNormalize(env)
    norm.reset()
    twin.reset()
    acts = actions_for(env, 9)
    for a in acts[:2]:
        norm.step(a)
        twin.step(a)
    norm.training = False                               # the eval form: frozen stats, one launch
    bits, returns = stats_bits(norm), norm.returns.clone()
    mean, scale = host(norm.obs_rms.mean), host(norm.obs_rms.scale)
    for a in acts[2:5]:
        raw, raw_r, _ = (host(x).copy() for x in twin.step(a)[:3])
        obs, rew, done, _ = norm.step(a)
        assert torch.equal(stats_bits(norm), bits) and torch.equal(norm.returns, returns)
        np.testing.assert_array_equal(host(obs), vm.apply(raw, mean, scale, 10.0))
        np.testing.assert_array_equal(host(rew), vm.apply(raw_r, 0.0, host(norm.ret_rms.scale)[0], 10.0,
                                                          center=False))
    fresh = stats_bits(VecNormalize(crypto_env(E)))
    for kw in (dict(norm_obs=False), dict(norm_reward=False), dict(norm_obs=False, norm_reward=False)):
        env, twin = crypto_env(E), crypto_env(E)
        norm = VecNormalize(env, **kw)
        model = vm.VecNormalize(E, env.obs.shape[1], **kw)
        raw = host(twin.reset())
        np.testing.assert_array_equal(host(norm.reset()), model.reset(raw))
        for a in acts[5:9]:
            raw, raw_r, raw_d = (host(x).copy() for x in twin.step(a)[:3])
            obs, rew, done, _ = norm.step(a)
            model.step(raw, raw_r, raw_d)
            if "norm_obs" in kw:
                np.testing.assert_array_equal(host(obs), raw)
                assert torch.equal(stats_bits(norm)[:-4], fresh[:-4])
            else:
                np.testing.assert_array_equal(host(obs), vm.apply(raw, host(norm.obs_rms.mean),
                                                                  host(norm.obs_rms.scale), 10.0))
            if "norm_reward" in kw:
                np.testing.assert_array_equal(host(rew), raw_r)
                assert torch.equal(stats_bits(norm)[-4:], fresh[-4:]) and (norm.returns == 0).all()
            else:
                np.testing.assert_array_equal(host(norm.returns), model.returns)
                np.testing.assert_allclose(host(norm.ret_rms.var), model.ret_rms.var, rtol=1e-8)


def test_captured_step_replays_equal_an_eager_twin():
    """norm.step captured once and replayed four times equals an eager wrapper bit for bit, stats and
    returns included: the ticket word is back at zero after every launch."""
    need_gpu()
    from finrl_amd import VecNormalize
    E = 259
    a_norm, b_norm = VecNormalize(stock_env(E)), VecNormalize(stock_env(E))
    acts = actions_for(a_norm, 5)
    a_norm.reset(); b_norm.reset()
    a_norm.step(acts[0]); b_norm.step(acts[0])          # first call outside the capture
    static = acts[0].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = b_norm.step(static)
    for t in range(1, 5):
        static.copy_(acts[t])
        g.replay()
        want = a_norm.step(acts[t])
        torch.cuda.synchronize()
        for name, x, y in zip(("obs", "reward", "done"), got, want):
            assert torch.equal(x, y), f"{name} at replay {t}"
        assert torch.equal(stats_bits(a_norm), stats_bits(b_norm)), f"stats at replay {t}"
        assert torch.equal(a_norm.returns, b_norm.returns)
        assert int(b_norm.obs_rms._ticket.item()) == 0
    count = 1e-4
    for _ in range(6):                                   # the reset, the eager step, four replays
        count += E
    assert float(b_norm.obs_rms.count.item()) == count


def policy(obs):
    a = torch.tanh(obs[:, :2] * 0.37 + obs[:, 2:4] * 0.11)
    return a, obs[:, 0] * 0.5, -a.abs().sum(1)


def test_rollout_and_replay_buffers_take_the_wrapper():
    need_gpu()
    from finrl_amd import ReplayBuffer, RolloutBuffer, VecNormalize
    E, n_steps = 70, 6
    a_norm, b_norm = VecNormalize(crypto_env(E)), VecNormalize(crypto_env(E))
    D, A = a_norm.obs_dim, a_norm.action_dim
    buf = RolloutBuffer(n_steps, E, D, A, obs_pitch=D + 3)               # a pitched rollout buffer
    buf._obs_buf.fill_(SENTINEL)
    last = buf.collect(a_norm, policy, a_norm.reset())
    obs = b_norm.reset().clone()
    assert torch.equal(buf.obs[0], obs)
    for t in range(n_steps):
        a, _, _ = policy(obs)
        o, r, d, _ = b_norm.step(a)
        assert torch.equal(buf.obs[t + 1], o) and torch.equal(buf.rewards[t], r), t
        assert torch.equal(buf.dones[t], d), t
        obs = o.clone()
    assert torch.equal(last, obs) and (buf._obs_buf[:, :, D:] == SENTINEL).all()
    assert buf.dones.sum().item() >= E                                   # an episode ended inside

    ring = ReplayBuffer(8, E, D, A)                                      # the default, aligned pitch
    c_norm, d_norm = VecNormalize(crypto_env(E)), VecNormalize(crypto_env(E))
    ring.start(c_norm, c_norm.reset())
    obs = d_norm.reset().clone()
    assert torch.equal(ring.obs[0], obs)
    for t, a in enumerate(actions_for(c_norm, 5, seed=3)):
        ring.step(c_norm, a)
        o, r, d, _ = d_norm.step(a)
        assert torch.equal(ring.obs[t + 1], o) and torch.equal(ring.rewards[t], r), t
        assert torch.equal(ring.dones[t], d) and torch.equal(ring.actions[t], a), t
    assert (ring.obs[1:6].abs() <= 10.0).all()                           # normalised rows: inside the clip


def test_state_dict_round_trip_and_reset():
    need_gpu()
    from finrl_amd import VecNormalize
    E = 70
    a_norm, b_env = VecNormalize(stock_env(E), gamma=0.9), stock_env(E)
    acts = actions_for(a_norm, 5)
    a_norm.reset(); b_env.reset()
    for a in acts[:3]:
        a_norm.step(a)
        b_env.step(a)
    state = a_norm.state_dict()
    assert all(v.device.type == "cpu" for v in state.values()) and state["obs_mean"].dtype == torch.float64
    assert sorted(state) == ["obs_count", "obs_mean", "obs_var", "ret_count", "ret_mean", "ret_var", "returns"]
    b_norm = VecNormalize(b_env, gamma=0.9)
    b_norm.load_state_dict(state)
    assert torch.equal(stats_bits(a_norm), stats_bits(b_norm))           # scale recomputed to the same bits
    for training in (True, False):
        a_norm.training = b_norm.training = training
        a = acts[3 + (not training)]
        for x, y in zip(a_norm.step(a)[:3], b_norm.step(a)[:3]):
            assert torch.equal(x, y)
        assert torch.equal(stats_bits(a_norm), stats_bits(b_norm)) and torch.equal(a_norm.returns, b_norm.returns)
    assert (a_norm.returns != 0).any()
    a_norm.reset()
    assert (a_norm.returns == 0).all()
    x = a_norm.get_original_obs()
    np.testing.assert_allclose(host(a_norm.unnormalize_obs(a_norm.normalize_obs(x))), host(x), rtol=1e-5, atol=1e-3)
    r = torch.linspace(-5, 5, 33, device="cuda")
    np.testing.assert_array_equal(
        host(a_norm.normalize_reward(r)), vm.apply(host(r), 0.0, host(a_norm.ret_rms.scale)[0], 10.0, center=False))
