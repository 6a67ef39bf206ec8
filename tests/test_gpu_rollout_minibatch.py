"""RolloutBuffer.minibatch / get / next_epoch on the MI355X against the NumPy model
(tests/rollout_model.py) with tolerance 0: every lane-group width x unit size of the one kernel, short
last minibatches, the epoch word, caller outputs, a captured epoch and a collected rollout."""
import numpy as np
import pytest

import replay_model as rm
import rollout_model as rom
from replay_cases import POISON, need_gpu
from test_gpu_replay_dispatch import SHAPES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 7


def coded_buffer(n_steps, E, D, P, A, seed=SEED):
    """A RolloutBuffer whose cells hold a code of (row, column) or (row, field), exact in f32 -- a
    wrong row, column or field shows -- with NaN in the pad columns of obs, plus the host copies (obs
    without the pad).  Slice n_steps of obs, which is never drawn, carries the code of rows >= M."""
    from finrl_amd import RolloutBuffer
    buf = RolloutBuffer(n_steps, E, D, A, seed=seed, obs_pitch=P)
    assert buf.obs_pitch == P and tuple(buf.obs.shape) == (n_steps + 1, E, D) and buf.obs.stride(1) == P
    row = np.arange((n_steps + 1) * E, dtype=np.float64).reshape(n_steps + 1, E)
    obs = (row[:, :, None] * 1024 + np.arange(D)).astype(np.float32)
    act = (-(row[:n_steps, :, None] * 128 + np.arange(A) + 1)).astype(np.float32)
    scal = [(row[:n_steps] * 4 + j + 0.25).astype(np.float32) for j in range(4)]
    buf._obs_buf.fill_(float("nan"))
    buf.obs.copy_(torch.from_numpy(obs))
    for name, x in zip(("actions", "values", "log_probs", "advantages", "returns"), [act] + scal):
        getattr(buf, name).copy_(torch.from_numpy(x))
    return buf, (obs, act, *scal)


def assert_samples(smp, rows, want_rows, host, tag):
    """The six fields and the rows block against the model: dtype, shape and every value."""
    np.testing.assert_array_equal(rows.cpu().numpy(), want_rows, err_msg=f"rows {tag}")
    assert rows.dtype == torch.int32
    want = rom.minibatch_lookup(*host, want_rows)
    assert type(smp).__name__ == "RolloutBufferSamples" and len(smp) == 6
    for name, g, w in zip(smp._fields, smp, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {tag}: {g.dtype}{g.shape}"
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {tag}")


def poisoned_out(n, D, pitch, A, offset=0):
    """Caller outputs poisoned all over -> (the six tensors, the backing of observations): rows `pitch`
    floats apart, starting `offset` floats into an allocation."""
    kw = dict(dtype=torch.float32, device="cuda")
    back = torch.full((n * pitch + offset,), POISON, **kw)
    o = back[offset:].view(n, pitch)[:, :D]
    return (o, torch.full((n, A), POISON, **kw), *(torch.full((n,), POISON, **kw) for _ in range(4))), back


@pytest.mark.parametrize("D,P,A,unit,G", SHAPES)
def test_every_instantiation_equals_model(D, P, A, unit, G):
    """n_steps = 5, E = 27 (M = 135), batch size 131: several blocks with a partial last one at every
    G, then a last minibatch of 4 rows.  The shape lands on the (G, unit) the table names, and all six
    fields and last_rows equal the model; pad columns of a caller's output stay untouched."""
    need_gpu()
    n_steps, E, B = 5, 27, 131
    M = n_steps * E
    buf, host = coded_buffer(n_steps, E, D, P, A)

    smp = buf.minibatch(0, B)
    assert rm.gather_group(D, P, P, (buf._obs_buf.data_ptr(), smp.observations.data_ptr())) == (G, unit)
    assert smp.observations.shape == (B, D) and smp.old_values.shape == (B,)
    assert_samples(smp, buf.last_rows, rom.minibatch_rows(0, B, M, 0, SEED), host, "minibatch 0")

    last = buf.minibatch(1, B)                      # 4 rows: views of the leading rows
    assert last.observations.shape == (4, D) and last.observations.data_ptr() == smp.observations.data_ptr()
    assert last.returns.shape == (4,) and buf.last_rows.shape == (4,)
    want_last = rom.minibatch_rows(1, B, M, 0, SEED)
    assert_samples(last, buf.last_rows, want_last, host, "minibatch 1")
    assert sorted(rom.minibatch_rows(0, B, M, 0, SEED).tolist() + want_last.tolist()) == list(range(M))

    out, back = poisoned_out(B, D, P, A)
    assert rm.gather_group(D, P, P, (buf._obs_buf.data_ptr(), out[0].data_ptr())) == (G, unit)
    got = buf.minibatch(0, B, out=out)
    assert got.observations is out[0] and got.returns is out[5]
    assert_samples(got, buf.last_rows, rom.minibatch_rows(0, B, M, 0, SEED), host, "out=")
    assert (back.view(B, P)[:, D:] == POISON).all()


def test_get_yields_one_permutation_with_a_short_last_batch():
    need_gpu()
    n_steps, E, D, A, B = 3, 5, 6, 2, 4
    M = n_steps * E
    buf, host = coded_buffer(n_steps, E, D, D, A)
    orders = []
    for epoch in (0, 1):
        rows, sizes = [], []
        for k, smp in enumerate(buf.get(B)):
            assert buf.epochs == epoch              # bumped only when the generator ends
            assert_samples(smp, buf.last_rows, rom.minibatch_rows(k, B, M, epoch, SEED), host, f"{epoch}/{k}")
            rows += buf.last_rows.cpu().tolist()
            sizes.append(smp.observations.shape[0])
        assert sizes == [4, 4, 4, 3] and sorted(rows) == list(range(M))
        assert buf.epochs == epoch + 1 and int(buf.epoch.item()) == epoch + 1
        orders.append(rows)
    assert orders[0] != orders[1]


def test_epochs_differ_and_a_fresh_buffer_repeats_them():
    need_gpu()
    n_steps, E, D, A = 5, 27, 8, 3
    M = n_steps * E
    orders = []
    for _ in range(2):
        buf, host = coded_buffer(n_steps, E, D, D, A, seed=(3 << 32) | 11)
        mine = []
        for epoch in (0, 1, 2):
            (smp,) = list(buf.get())                 # None: one batch of all M rows
            assert smp.observations.shape == (M, D)
            want = rom.minibatch_rows(0, M, M, epoch, (3 << 32) | 11)
            assert_samples(smp, buf.last_rows, want, host, f"epoch {epoch}")
            mine.append(buf.last_rows.cpu().tolist())
        assert mine[0] != mine[1] and mine[1] != mine[2] and mine[0] != mine[2]
        orders.append(mine)
    assert orders[0] == orders[1]
    other, _ = coded_buffer(n_steps, E, D, D, A, seed=12)
    other.minibatch(0, M)
    assert other.last_rows.cpu().tolist() != orders[0][0]


def test_one_row_and_one_env():
    need_gpu()
    buf, host = coded_buffer(1, 1, 5, 8, 2)          # M = 1
    for epoch in (0, 1):
        (smp,) = list(buf.get())
        assert_samples(smp, buf.last_rows, np.zeros(1, np.int32), host, "M = 1")
    (smp,) = list(buf.get(1))
    assert_samples(smp, buf.last_rows, np.zeros(1, np.int32), host, "M = 1, batch 1")
    assert buf.epochs == 3

    buf, host = coded_buffer(7, 1, 5, 5, 2)          # E = 1: the row is the step
    rows = []
    for k, smp in enumerate(buf.get(3)):
        assert_samples(smp, buf.last_rows, rom.minibatch_rows(k, 3, 7, 0, SEED), host, f"E = 1, {k}")
        rows += buf.last_rows.cpu().tolist()
    assert sorted(rows) == list(range(7))


def test_unaligned_out_takes_the_dword_path():
    """D = 40 packed rows move as 16-byte units into an aligned output (G = 8) and as dwords into one
    that starts 4 bytes past an allocation (G = 32): the same batch, nothing written around it."""
    need_gpu()
    n_steps, E, D, A, B = 5, 27, 40, 3, 131
    M = n_steps * E
    buf, host = coded_buffer(n_steps, E, D, D, A)
    want = rom.minibatch_rows(0, B, M, 0, SEED)
    for offset, group in ((0, (8, 16)), (1, (32, 4))):
        out, back = poisoned_out(B, D, D, A, offset=offset)
        assert rm.gather_group(D, D, D, (buf._obs_buf.data_ptr(), out[0].data_ptr())) == group
        assert_samples(buf.minibatch(0, B, out=out), buf.last_rows, want, host, f"offset {offset}")
        assert (back[:offset] == POISON).all()
    wide, back = poisoned_out(B, D, D + 3, A)         # a pitch that is no multiple of 4 floats
    assert rm.gather_group(D, D, D + 3, (buf._obs_buf.data_ptr(), wide[0].data_ptr())) == (32, 4)
    assert_samples(buf.minibatch(0, B, out=wide), buf.last_rows, want, host, "pitch 43")
    assert (back.view(B, D + 3)[:, D:] == POISON).all()


def test_argument_errors_name_the_shapes():
    need_gpu()
    buf, _ = coded_buffer(3, 5, 6, 6, 2)
    for bad in (lambda: buf.minibatch(0, 0), lambda: buf.minibatch(0, 16), lambda: buf.minibatch(4, 4),
                lambda: buf.minibatch(-1, 4), lambda: list(buf.get(0)), lambda: list(buf.get(16))):
        with pytest.raises(ValueError, match=r"n_steps=3, num_envs=5 \(15 rows\)"):
            bad()
    out, _ = poisoned_out(4, 6, 6, 2)
    with pytest.raises(ValueError):
        buf.minibatch(0, 4, out=out[:5])
    with pytest.raises(ValueError, match="old_values"):
        buf.minibatch(0, 4, out=out[:2] + (out[2][:3],) + out[3:])
    with pytest.raises(ValueError):
        buf.minibatch(3, 4, out=out)                 # the last minibatch holds 3 rows
    assert buf.epochs == 0 and int(buf.epoch.item()) == 0


def test_captured_epoch_draws_a_fresh_permutation_at_every_replay():
    """Three minibatches (50, 50, 35 rows of M = 135) plus next_epoch, captured once: the eager epoch
    and two replays equal the model at epochs 0, 1 and 2."""
    need_gpu()
    n_steps, E, D, P, A, B = 5, 27, 20, 24, 3, 50
    M = n_steps * E
    buf, host = coded_buffer(n_steps, E, D, P, A)
    outs = [poisoned_out(min(B, M - k * B), D, P, A)[0] for k in range(3)]

    def epoch_of_minibatches():
        got = []
        for k in range(3):
            smp = buf.minibatch(k, B, out=outs[k])
            got.append((smp, buf.last_rows))
        buf.next_epoch()
        return got

    def check(got, epoch):
        rows = []
        for k, (smp, last_rows) in enumerate(got):
            assert_samples(smp, last_rows, rom.minibatch_rows(k, B, M, epoch, SEED), host, f"{epoch}/{k}")
            rows += last_rows.cpu().tolist()
        assert sorted(rows) == list(range(M))

    check(epoch_of_minibatches(), 0)                 # first calls outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = epoch_of_minibatches()
    for epoch in (1, 2):
        assert int(buf.epoch.item()) == epoch
        g.replay()
        torch.cuda.synchronize()
        check(got, epoch)
    assert int(buf.epoch.item()) == 3                # the bump is part of the capture


def test_collected_rollout_end_to_end():
    """VecCryptoEnv at the smallest shape of its parity test: collect, GAE, then one epoch of get();
    every yielded field equals torch indexing of the buffer by last_rows."""
    need_gpu()
    from finrl_amd import RolloutBuffer
    from finrl_amd.vec_crypto import VecCryptoEnv
    E, T, N, W, n_steps, B = 64, 12, 1, 0, 6, 100
    rng = np.random.default_rng(E + N)
    price = 10.0 ** rng.uniform(-1, 4.5, N) * np.exp(np.cumsum(rng.normal(0, 0.004, (T, N)), axis=0))
    env = VecCryptoEnv({"price_array": price, "tech_array": rng.normal(0, 3000, (T, W))}, E, lookback=1)
    D, M = env.obs_dim, n_steps * E
    buf = RolloutBuffer(n_steps, E, D, N, seed=SEED)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)

    def policy(obs):
        a = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
        return a, obs[:, 0] * 0.5 + a.sum(1) * 0.01, -a.abs().sum(1)

    last_obs = buf.collect(env, policy, env.reset())
    buf.compute_returns_and_advantage(last_obs[:, 0] * 0.5, 0.99, 0.95)
    flat = [buf.obs[:n_steps].reshape(M, D), buf.actions.reshape(M, N), buf.values.reshape(M),
            buf.log_probs.reshape(M), buf.advantages.reshape(M), buf.returns.reshape(M)]
    assert buf.advantages.abs().sum().item() > 0
    rows, sizes = [], []
    for k, smp in enumerate(buf.get(B)):
        r = buf.last_rows.long()
        np.testing.assert_array_equal(buf.last_rows.cpu().numpy(), rom.minibatch_rows(k, B, M, 0, SEED))
        for name, got, src in zip(smp._fields, smp, flat):
            assert torch.equal(got, src[r]), f"{name} of minibatch {k}"
        rows += r.cpu().tolist()
        sizes.append(len(r))
    assert sizes == [100, 100, 100, 84] and sorted(rows) == list(range(M)) and buf.epochs == 1
