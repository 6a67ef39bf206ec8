"""VecNormalize / RunningMeanStd on the MI355X at the shapes test_gpu_vecnorm.py leaves out: more than
1024 columns (the last block's merge walks them in blocks of 1024), exactly 128 row tiles, row tiles
taller than a block's row-lanes at one unit-lane, a return column of more than one tile, apply over
several row tiles and more than 64 column chunks, a real env 1140 columns wide -- and columns that
hold a NaN or an infinity, which must not reach their neighbours.

Every case asserts through vm.tiling / vm.apply_tiling (tests/vecnorm_model.py, checked on the CPU in
test_vecnorm_model.py) that it takes the path it is here for: a change of the tiling rule then fails a
test instead of quietly un-testing a branch.

Tolerances are test_gpu_vecnorm.py's: var at rtol 1e-8, mean at atol 1e-8 * sigma (1e-8 * |mean| for
a constant column), count exact, apply at tolerance 0.  Its bound on the kernel's error, n * 2^-53
relative to sum (x-K)^2 <= about 50 * n * var, grows with n: at n = 262,145 it is 1.5e-9, a margin of
about 7, and at the one taller case added here, n = 524,289, 2.9e-9, a margin of 3.4.  The model keeps
less than a tenth of the tolerance to itself (test_vecnorm_model.py).

Measured, worst kernel-vs-model error as a fraction of the tolerance (the module prints them; -s
shows them): moments 0.023, steps through ScriptedEnv 0.0040, the portfolio env 1e-7 (all its envs
show the same panel row, so every batch is constant)."""
import math

import numpy as np
import pytest

import test_gpu_vecnorm as base
import vecnorm_model as vm
from replay_cases import need_gpu
from vecnorm_cases import ScriptedEnv, gaussian_columns

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

host, on_device, SENTINEL = base.host, base.on_device, base.SENTINEL
WORST = {}                                       # group -> worst error seen, as a fraction of the tolerance


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for group, ratio in sorted(WORST.items()):
        print(f"\nkernel vs model, {group}: worst error {ratio:.3g} of the tolerance")


def check_stats(rms, model, sigma, tag, group):
    """base.assert_stats, after noting how much of the tolerance the kernel used."""
    unit = np.where(sigma > 0, sigma, np.abs(model.mean))
    ratio = max((np.abs(host(rms.mean) - model.mean) / (1e-8 * unit)).max(),
                (np.abs(host(rms.var) - model.var) / (1e-8 * model.var)).max())
    WORST[group] = max(WORST.get(group, 0.0), float(ratio))
    base.assert_stats(rms, model, sigma, tag)


# ------------------------------------------------------------------------------------ moments
MOMENTS = [  # n, dim, pitch, what vm.tiling must say, and what else makes the case
    (259, 1140, 1140, dict(vec=True, chunks=18, tiles=5, column_blocks=2), lambda t: 1140 - vm.MB == 116),
    (259, 1025, 1028, dict(vec=True, chunks=17, column_blocks=2),          # last unit partial; block 2: 1 column
     lambda t: 1025 % 4 == 1 and 1025 - vm.MB == 1),
    (70, 2049, 2049, dict(vec=False, chunks=33, column_blocks=3), lambda t: True),
    (2100, 1140, 1140, dict(vec=True, tiles=33, runs=1, column_blocks=2), lambda t: t.per > vm.FIN_DEPTH),
    (259, 4224, 4224, dict(vec=True, chunks=66, column_blocks=5), lambda t: True),
    (8192, 64, 64, dict(vec=True, tiles=vm.MAX_TILES, runs=16, per=8), lambda t: 8192 == t.tiles * t.tile_rows),
    (131072, 1, 1, dict(vec=False, lg=0, tiles=vm.MAX_TILES, tile_rows=1024), lambda t: True),
    (131073, 1, 1, dict(vec=False, lg=0, tiles=65, tile_rows=2048),        # rows past rl; a 1-row last tile
     lambda t: t.tile_rows > t.rl and 131073 - 64 * t.tile_rows == 1),
    (262145, 4, 4, dict(vec=True, lg=0, tile_rows=3072),
     lambda t: t.tile_rows > t.rl and 0 < 262145 - (t.tiles - 1) * t.tile_rows < t.tile_rows),
    (524289, 1, 1, dict(vec=False, lg=0, tile_rows=5120),                  # a lane's SECOND trip of four rows,
     lambda t: 4 * t.rl < t.tile_rows < 8 * t.rl),                         # three of them padding
]


@pytest.mark.parametrize("n,dim,pitch,path,more", MOMENTS, ids=[f"{c[0]}x{c[1]}p{c[2]}" for c in MOMENTS])
def test_moments_on_the_wide_and_tall_paths(n, dim, pitch, path, more):
    """As test_moments_equal_model: one update, a bit-identical repeat from the same state, then a
    prefix and a suffix of the same rows, each against the model."""
    need_gpu()
    from finrl_amd import RunningMeanStd
    t = vm.tiling(n, dim, pitch)
    assert {k: getattr(t, k) for k in path} == path and more(t), t
    x, sigma = gaussian_columns(n, dim)
    xd, _ = on_device(x, pitch)
    assert xd.data_ptr() % 16 == 0
    rms, model = RunningMeanStd(dim), vm.RunningMeanStd(dim)
    start = rms._block.clone()
    rms.update(xd)
    first = rms._block[:3 * dim + 1].clone()
    model.update(x)
    check_stats(rms, model, sigma, "after one update", "moments")
    if dim > 1:
        assert host(rms.mean)[-1] == model.mean[-1]          # the constant column: the same roundings on both sides

    rms._block.copy_(start)
    rms.update(xd)
    assert torch.equal(rms._block[:3 * dim + 1].view(torch.int64), first.view(torch.int64))

    for lo, hi in ((0, n // 2 + 1), (n // 3, n)):
        rms.update(xd[lo:hi])
        model.update(x[lo:hi])
    check_stats(rms, model, sigma, "after three updates", "moments")


# ------------------------------------------------------------------------------------ apply
APPLY = [  # n, dim, pitch in, pitch out, what vm.apply_tiling must say
    (4097, 1, 1, 1, dict(vec=False, lg=0, tile_rows=4096, tiles=2)),
    (1030, 3, 3, 5, dict(vec=False, lg=2, tile_rows=1024, tiles=2)),
    (300, 1140, 1140, 1144, dict(vec=True, chunks=18, tiles=2)),
    (70, 2049, 2049, 2052, dict(vec=False, chunks=33, tiles=2)),
    (70, 4224, 4224, 4224, dict(vec=True, chunks=66)),                     # more than 64 column chunks
]


@pytest.mark.parametrize("n,dim,pin,pout,path", APPLY, ids=[f"{c[0]}x{c[1]}" for c in APPLY])
def test_apply_over_several_row_tiles_and_many_chunks(n, dim, pin, pout, path):
    """test_apply_equals_formula's checks (tolerance 0 against vm.apply with and without the mean, pads
    untouched, the in-place form, a fresh output) at shapes of more than one row tile or 64 chunks."""
    t = vm.apply_tiling(n, dim, pin, pout)
    assert {k: getattr(t, k) for k in path} == path, t
    base.test_apply_equals_formula(n, dim, pin, pout)


# ------------------------------------------------------------------------------------ steps
STEPS, GAMMA, CLIP_OBS, CLIP_REW = 6, 0.97, 5.0, 3.0


def script(E, D):
    """Seven frames (the reset's, then six steps) -> obs [7, E, D], reward [7, E], done [7, E].
    Rewards of both signs over 1e-3 .. 1e5; done: nobody, every other env, the whole first tile of the
    return column, nobody, everybody, nobody."""
    x, _ = gaussian_columns((STEPS + 1) * E, D)
    rng = np.random.default_rng(E + D)
    reward = (rng.choice([-1.0, 1.0], (STEPS + 1, E)) * 10.0 ** rng.uniform(-3, 5, (STEPS + 1, E))).astype(np.float32)
    done = np.zeros((STEPS + 1, E), np.uint8)
    done[2, ::2] = 1
    done[3, :vm.tiling(E, 1, 1).tile_rows] = 1
    done[5] = 1
    reward[0] = 0
    return x.reshape(STEPS + 1, E, D).copy(), reward, done


def actions(env):
    return torch.zeros(env.num_envs, env.action_dim, device="cuda")


def drive(norm, model, raw_of, acts, group, out=None):
    """`len(acts)` steps of the wrapper against the model fed raw_of(t, action) = the raw (obs, reward,
    done) of step t as NumPy: what test_step_against_twin_env checks after every step."""
    D = norm.obs_dim
    obs_rows, ret_rows = [host(norm.get_original_obs()).copy()], []
    ran_on = 0
    for t, a in enumerate(acts):
        raw, raw_r, raw_d = raw_of(t, a)
        obs, rew, done, info = norm.step(a, out)
        assert info is None
        if out is None:
            assert done is norm.env.done and rew is norm.reward and obs.data_ptr() == norm.obs.data_ptr()
        else:
            assert obs is out[0] and rew is out[1] and done is out[2]
        pre_zero = model.returns * GAMMA + raw_r.astype(np.float64)
        model.step(raw, raw_r, raw_d)
        obs_rows.append(raw)
        ret_rows.append(pre_zero[:, None])
        tag = f"step {t}"
        check_stats(norm.obs_rms, model.obs_rms, base.seen_sigma(obs_rows), f"obs {tag}", group)
        check_stats(norm.ret_rms, model.ret_rms, base.seen_sigma(ret_rows), f"ret {tag}", group)
        np.testing.assert_array_equal(
            host(obs), vm.apply(raw, host(norm.obs_rms.mean), host(norm.obs_rms.scale), CLIP_OBS), err_msg=tag)
        np.testing.assert_array_equal(
            host(rew), vm.apply(raw_r, 0.0, host(norm.ret_rms.scale)[0], CLIP_REW, center=False), err_msg=tag)
        np.testing.assert_array_equal(host(done), raw_d, err_msg=tag)
        np.testing.assert_array_equal(host(norm.get_original_obs()), raw, err_msg=tag)
        np.testing.assert_array_equal(host(norm.get_original_reward()), raw_r, err_msg=tag)
        np.testing.assert_array_equal(host(norm.returns), model.returns, err_msg=f"returns {tag}")
        assert (host(norm.returns)[raw_d.astype(bool)] == 0).all(), tag
        ran_on += int((model.returns != 0).sum())
    assert ran_on


def scripted_pair(E, D, pitch, **kw):
    from finrl_amd import VecNormalize
    obs, reward, done = script(E, D)
    env = ScriptedEnv(obs, reward, done, pitch)
    assert env.obs.stride(0) == pitch or E == 1
    assert env.obs.data_ptr() % 16 == 0 and torch.isnan(env._obs_buf[:, D:]).all()
    norm = VecNormalize(env, gamma=GAMMA, clip_obs=CLIP_OBS, clip_reward=CLIP_REW, **kw)
    assert (norm.num_envs, norm.action_dim, norm.device) == (E, env.action_dim, env.device)
    assert norm.auto_reset and norm.state is env.state
    model = vm.VecNormalize(E, D, gamma=GAMMA, clip_obs=CLIP_OBS, clip_reward=CLIP_REW)
    first = norm.reset()
    model.reset(obs[0])
    np.testing.assert_array_equal(
        host(first), vm.apply(obs[0], host(norm.obs_rms.mean), host(norm.obs_rms.scale), CLIP_OBS))
    return norm, model, (obs, reward, done)


STEP_CASES = {  # (E, D, obs pitch): what the obs tiling and the return column's tiling must say
    (1025, 6, 8): lambda o, r: o.vec and o.tiles == 3 and r.tiles == 2 and 1025 - r.tile_rows == 1,
    (2500, 6, 6): lambda o, r: not o.vec and o.tiles == 20 and o.runs == 10 and r.tiles == 3 and r.runs == 3,
    (300, 1140, 1140): lambda o, r: o.column_blocks == 2 and o.tiles == 5 and r.tiles == 1,
    (131073, 1, 1): lambda o, r: o.tile_rows == r.tile_rows == 2048 and r.tiles == 65 and r.runs == 13,
}


@pytest.mark.parametrize("E,D,pitch", list(STEP_CASES), ids=[f"{c[0]}x{c[1]}p{c[2]}" for c in STEP_CASES])
def test_step_through_a_scripted_env(E, D, pitch):
    """Six training steps: return columns of two, three and 65 tiles, ragged last ones, both merges of
    one launch over several tiles, and the obs merge over two column blocks beside a return merge."""
    need_gpu()
    assert STEP_CASES[(E, D, pitch)](vm.tiling(E, D, pitch), vm.tiling(E, 1, 1))
    norm, model, (obs, reward, done) = scripted_pair(E, D, pitch)
    drive(norm, model, lambda t, a: (obs[t + 1], reward[t + 1], done[t + 1]), [actions(norm)] * STEPS, "steps")
    assert int(norm.state["frame"].item()) == STEPS
    for k in range(1, STEPS + 1):                                # the script the test meant to play
        assert done[k].sum() == (0, (E + 1) // 2, min(E, vm.tiling(E, 1, 1).tile_rows), 0, E, 0)[k - 1]

    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")      # reset(mask): no update, returns zeroed
    mask[::3] = 1
    norm.step(actions(norm))                                     # (frame 0 again; returns run on from zero)
    want = host(norm.returns).copy()
    assert want.any()
    want[::3] = 0
    before = base.stats_bits(norm)
    norm.reset(mask)
    assert torch.equal(base.stats_bits(norm), before)
    np.testing.assert_array_equal(host(norm.returns), want)


def test_step_into_out_at_a_pitch_that_forces_dwords():
    """The obs of the env move in 16-byte units for the moments; out[0] at 7 floats a row allows the
    apply launch dwords only.  The pads of out[0] stay, done is copied inside the launch."""
    need_gpu()
    E, D, pitch = 1025, 6, 8
    assert vm.tiling(E, D, pitch).vec and not vm.apply_tiling(E, D, pitch, 7).vec
    norm, model, (obs, reward, done) = scripted_pair(E, D, pitch)
    back = torch.full((E, 7), SENTINEL, dtype=torch.float32, device="cuda")
    out = (back[:, :D], torch.empty(E, dtype=torch.float32, device="cuda"),
           torch.full((E,), 9, dtype=torch.uint8, device="cuda"))
    kept = norm.obs.clone()
    drive(norm, model, lambda t, a: (obs[t + 1], reward[t + 1], done[t + 1]), [actions(norm)] * STEPS, "steps", out)
    assert (back[:, D:] == SENTINEL).all() and torch.equal(norm.obs, kept)


def test_frozen_steps_leave_the_stats_bit_for_bit():
    need_gpu()
    E, D, pitch = 2500, 6, 8
    assert vm.tiling(E, D, pitch).vec and vm.tiling(E, 1, 1).tiles == 3
    norm, model, (obs, reward, done) = scripted_pair(E, D, pitch)
    drive(norm, model, lambda t, a: (obs[t + 1], reward[t + 1], done[t + 1]), [actions(norm)] * 2, "steps")
    norm.training = False
    bits, returns = base.stats_bits(norm), norm.returns.clone()
    mean, scale, rscale = host(norm.obs_rms.mean), host(norm.obs_rms.scale), host(norm.ret_rms.scale)[0]
    assert returns.any()
    for t in range(2, STEPS):
        o, r, d, _ = norm.step(actions(norm))
        assert torch.equal(base.stats_bits(norm), bits) and torch.equal(norm.returns, returns)
        np.testing.assert_array_equal(host(o), vm.apply(obs[t + 1], mean, scale, CLIP_OBS))
        np.testing.assert_array_equal(host(r), vm.apply(reward[t + 1], 0.0, rscale, CLIP_REW, center=False))
        np.testing.assert_array_equal(host(d), done[t + 1])
        assert int(norm.obs_rms._ticket.item()) == 0


def test_captured_step_of_a_three_tile_return_column_replays():
    """As test_captured_step_replays_equal_an_eager_twin, at 2500 envs: the return column has three
    tiles and the obs twenty, so both merges of the captured launch run over several tiles."""
    need_gpu()
    E, D, pitch = 2500, 6, 6
    assert vm.tiling(E, 1, 1).tiles == 3 and vm.tiling(E, D, pitch).tiles == 20
    (a_norm, _, _), (b_norm, _, _) = scripted_pair(E, D, pitch), scripted_pair(E, D, pitch)
    act = actions(a_norm)
    a_norm.step(act); b_norm.step(act)                     # first call outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = b_norm.step(act)
    for t in range(1, 5):
        g.replay()
        want = a_norm.step(act)
        torch.cuda.synchronize()
        for name, x, y in zip(("obs", "reward", "done"), got, want):
            assert torch.equal(x, y), f"{name} at replay {t}"
        assert torch.equal(base.stats_bits(a_norm), base.stats_bits(b_norm)), f"stats at replay {t}"
        assert torch.equal(a_norm.returns, b_norm.returns)
        assert int(b_norm.obs_rms._ticket.item()) == 0
    assert int(b_norm.state["frame"].item()) == 5 == int(a_norm.state["frame"].item())
    count = 1e-4
    for _ in range(6):                                     # the reset, the eager step, four replays
        count += E
    assert float(b_norm.obs_rms.count.item()) == count


# ------------------------------------------------------------------------------------ a real wide env
def portfolio_env(E):
    from finrl_amd.panel import PortfolioPanel
    from finrl_amd.vec_portfolio import VecStockPortfolioEnv
    rng = np.random.default_rng(E)
    T, N, K = 6, 30, 8
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    return VecStockPortfolioEnv(PortfolioPanel(close, rng.normal(0, 1e-4, (T, N, N)), rng.normal(0, 1, (T, K, N))), E)


def test_step_over_the_dow30_portfolio_env():
    """VecNormalize over the DOW30 portfolio env, D = (30 + 8) * 30 = 1140: eight steps through an
    episode end against the model fed an unwrapped twin."""
    need_gpu()
    from finrl_amd import VecNormalize
    E = 70
    env, twin = portfolio_env(E), portfolio_env(E)
    D = env.obs.shape[1]
    t = vm.tiling(E, D, env.obs.stride(0), env.obs.data_ptr() % 16 == 0)
    assert D == 1140 and t.column_blocks == 2 and t.tiles > 1, t
    norm = VecNormalize(env, gamma=GAMMA, clip_obs=CLIP_OBS, clip_reward=CLIP_REW)
    model = vm.VecNormalize(E, D, gamma=GAMMA, clip_obs=CLIP_OBS, clip_reward=CLIP_REW)
    raw = host(twin.reset())
    first = norm.reset()
    model.reset(raw)
    np.testing.assert_array_equal(host(norm.get_original_obs()), raw)
    np.testing.assert_array_equal(
        host(first), vm.apply(raw, host(norm.obs_rms.mean), host(norm.obs_rms.scale), CLIP_OBS))
    dones = []

    def raw_of(t, a):
        out = tuple(host(x).copy() for x in twin.step(a)[:3])
        dones.append(int(out[2].sum()))
        return out

    drive(norm, model, raw_of, base.actions_for(env, 8), "the portfolio env")
    assert sum(dones) >= E                                       # an episode ended inside


# ------------------------------------------------------------------------------------ non-finite columns
PLACES = {"row 0": 0, "a later tile's first row": 128, "mid-tile": 100, "in the ragged last tile": 257}
VALUES = (float("nan"), float("inf"), float("-inf"))


def poisoned_mean(value, row, t):
    """What the kernel leaves as the mean of a column whose cell `row` holds `value` (include/finenv.h):
    the value itself only where every later operation adds something finite to it."""
    if math.isnan(value) or row % t.tile_rows == 0:      # x - K = inf - inf in the tile's own sums
        return float("nan")
    if row // t.tile_rows == t.tiles - 1:                # the last tile merged: nothing is subtracted from it
        return value
    return float("nan")                                  # a later tile's delta is finite - inf; inf + -inf


def bits(t, cols):
    return t.index_select(0, cols).view(torch.int64)


@pytest.mark.parametrize("place", list(PLACES), ids=[p.replace(" ", "_") for p in PLACES])
@pytest.mark.parametrize("dim,pitch", ((291, 304), (1140, 1140)))
def test_a_non_finite_cell_poisons_its_column_only(dim, pitch, place):
    """A NaN, +inf or -inf in one cell of a column: every other column -- the three other components
    of its 16-byte unit, the columns of its chunk (which share the block's LDS), the columns of the
    other block of 1024 -- keeps the very bits it has with a finite draw in that cell."""
    need_gpu()
    from finrl_amd import RunningMeanStd
    n, row = 259, PLACES[place]
    t = vm.tiling(n, dim, pitch)
    assert t.vec and (t.tile_rows, t.tiles) == (64, 5) and t.column_blocks == (2 if dim > 1024 else 1)
    assert {"row 0": row == 0, "a later tile's first row": row > 0 and row % 64 == 0,
            "mid-tile": row % 64 > 0 and row // 64 < 4, "in the ragged last tile": row > 256}[place]
    cols = [8, 11, dim - 1] + ([1023, 1024] if dim > 1024 else [])      # components 0 and 3 of a unit; the tail
    assert (dim - 1) % 4 == (2 if dim == 291 else 3) and dim % 4 == (3 if dim == 291 else 0)  # (of the partial unit)
    values = [VALUES[(j + list(PLACES).index(place)) % 3] for j in range(len(cols))]
    clean, _ = gaussian_columns(n, dim)
    dirty = clean.copy()
    dirty[row, cols] = values
    others = torch.tensor(sorted(set(range(dim)) - set(cols)), device="cuda")
    cd, dd = on_device(clean, pitch)[0], on_device(dirty, pitch)[0]
    good, bad = RunningMeanStd(dim), RunningMeanStd(dim)

    def compare(tag, want_mean):
        for name in ("mean", "var", "scale"):                                                   # (a)
            assert torch.equal(bits(getattr(bad, name), others), bits(getattr(good, name), others)), f"{name} {tag}"
        assert torch.equal(bad.count, good.count) and int(bad._ticket.item()) == 0              # (b)
        mean, var, scale = host(bad.mean)[cols], host(bad.var)[cols], host(bad.scale)[cols]
        print(f"{tag}: cell {values} at row {row} -> mean {mean}, var {var}")
        assert np.isnan(var).all() and np.isnan(scale).all(), tag                               # (c)
        np.testing.assert_array_equal(mean, want_mean, err_msg=tag)

    good.update(cd)
    bad.update(dd)
    compare("after the poisoned update", [poisoned_mean(v, row, t) for v in values])
    assert all(np.isnan(m) for v, m in zip(values, host(bad.mean)[cols]) if np.isnan(v))
    for lo, hi in ((0, n // 2 + 1), (n // 3, n)):                                               # (d)
        good.update(cd[lo:hi])
        bad.update(cd[lo:hi])
    compare("after two clean updates", [float("nan")] * len(cols))    # inf + (finite - inf) * w

    got = host(bad.apply(cd))                                                                   # (e)
    want = vm.apply(clean, host(good.mean), host(good.scale), 10.0)
    want[:, cols] = np.nan
    np.testing.assert_array_equal(got, want)
    assert np.isnan(got).sum() == n * len(cols)
