"""Shared by the replay buffer's GPU tests (tests/test_gpu_replay*.py): the coded ring, the head setter,
poisoned caller outputs, the host copy of a ring, the small crypto env and the batch comparison."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

POISON = -7777.0
RING_SEED = 4          # chosen so that every way an n-step return can end occurs (asserted on the model)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def coded_ring(S, E, D, P, A, seed=0, ring_seed=None):
    """A ReplayBuffer whose obs / action cells hold a code of (slot, env, column) (exact in f32; NaN in
    the pad columns of obs), plus host copies (obs without the pad).  Rewards and dones, ring_seed None:
    a code of (slot, env) and a checkerboard; an int: rewards of both signs with magnitudes 1e-3 .. 1e6
    and Bernoulli(0.25) dones from that seed."""
    from finrl_amd import ReplayBuffer
    buf = ReplayBuffer(S, E, D, A, obs_pitch=P, seed=seed)
    assert buf.obs_pitch == P and tuple(buf.obs.shape) == (S, E, D) and buf.obs.stride(1) == P
    se = np.arange(S * E, dtype=np.float64).reshape(S, E)
    obs = (se[:, :, None] * 512 + np.arange(D)).astype(np.float32)
    act = (-(se[:, :, None] * 64 + np.arange(A) + 1)).astype(np.float32)
    if ring_seed is None:
        rew = (se + 0.5).astype(np.float32)
        done = ((np.arange(S)[:, None] + np.arange(E)[None, :]) % 2).astype(np.uint8)
    else:
        rng = np.random.default_rng(ring_seed)
        rew = (rng.choice([-1.0, 1.0], (S, E)) * 10.0 ** rng.uniform(-3, 6, (S, E))).astype(np.float32)
        done = (rng.random((S, E)) < 0.25).astype(np.uint8)
    buf._obs_buf.fill_(float("nan"))
    buf.obs.copy_(torch.from_numpy(obs))
    buf.actions.copy_(torch.from_numpy(act))
    buf.rewards.copy_(torch.from_numpy(rew))
    buf.dones.copy_(torch.from_numpy(done))
    return buf, (obs, act, rew, done)


def set_head(buf, pos, n_valid):
    buf.pos, buf._n_valid = pos, n_valid
    buf.head.copy_(torch.tensor([pos, n_valid], dtype=torch.int32))


def outs(B, D, A, kind, n_fields):
    """Caller outputs poisoned all over -> (the n_fields tensors in the order of ReplayBufferSamples
    (5) or NStepReplayBufferSamples (6), the two backing observation buffers).  "packed": rows D floats
    apart starting one float past an allocation (4-byte aligned only); "slice": columns 4 .. 4+D of
    rows of their own pitch."""
    kw = dict(dtype=torch.float32, device="cuda")
    if kind == "packed":
        back = [torch.full((B * D + 1,), POISON, **kw) for _ in range(2)]
        o, n = (b[1:].view(B, D) for b in back)
    else:
        pitch = (D + 3) // 4 * 4 + 8
        back = [torch.full((B, pitch), POISON, **kw) for _ in range(2)]
        o, n = (b[:, 4:4 + D] for b in back)
    return (o, torch.full((B, A), POISON, **kw), n,
            *(torch.full((B, 1), POISON, **kw) for _ in range(n_fields - 3))), back


def host_ring(buf):
    return tuple(x.cpu().numpy() for x in (buf.obs, buf.actions, buf.rewards, buf.dones))


def per_ring(S, E, D, P, A, seed=0, ring_seed=None):
    """coded_ring's contents in a PrioritizedReplayBuffer, plus the host copies."""
    from finrl_amd import PrioritizedReplayBuffer
    src, host = coded_ring(S, E, D, P, A, ring_seed=ring_seed)
    buf = PrioritizedReplayBuffer(S, E, D, A, obs_pitch=P, seed=seed)
    for name in ("_obs_buf", "actions", "rewards", "dones"):
        getattr(buf, name).copy_(getattr(src, name))
    return buf, host


def random_tickets(S, E, seed):
    """uint32 [S, E]: a third zeros, some at 1 and at 2^32 - 1, the rest anywhere."""
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 2 ** 32, (S, E), dtype=np.uint64)
    kind = rng.integers(0, 6, (S, E))
    t[kind < 2] = 0
    t[kind == 2] = 2 ** 32 - 1
    t[kind == 3] = 1
    t.reshape(-1)[rng.integers(0, S * E)] = 12345          # never all zero
    return t.astype(np.uint32)


def set_tickets(buf, t):
    buf.tickets.copy_(torch.from_numpy(np.ascontiguousarray(t).view(np.int32)))
    buf.rebuild()


def crypto_env(E, auto_reset=True):
    """VecCryptoEnv on a 7-row panel of 3 coins: episodes end inside a ring of a few slots."""
    from finrl_amd.vec_crypto import VecCryptoEnv
    rng = np.random.default_rng(1)
    T, N, W = 7, 3, 4
    price = 10.0 ** rng.uniform(0, 3, N) * np.exp(np.cumsum(rng.normal(0, 5e-3, (T, N)), axis=0))
    cfg = {"price_array": price, "tech_array": rng.normal(0, 3000, (T, W))}
    return VecCryptoEnv(cfg, E, lookback=1, auto_reset=auto_reset)


def assert_batch(smp, want, tag, steps=None):
    """The fields of a samples namedtuple of any kind (the five, then discounts and / or probabilities
    where it has them) and, where given, the steps block after them, against ``want`` in that order:
    dtype, shape and every value."""
    got = tuple(smp) + (() if steps is None else (steps,))
    assert len(want) == len(got), f"{tag}: {len(want)} expected fields for {len(got)}"
    for name, g, w in zip(smp._fields + ("steps",), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {tag}: {g.dtype}{g.shape}"
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {tag}")
