"""CPU-side checks of the replay buffer's n-step sampler: the new ABI struct and symbols, the
argument validation of finenv_replay_sample_nstep / _gather_nstep (refused before any launch), and
hand-worked known answers of the NumPy model (tests/replay_nstep_model.py)."""
import ctypes as C

import numpy as np
import pytest

import replay_nstep_model as nm
from replay_abi_cases import assert_refusals, lib  # noqa: F401


def test_struct_sizes(lib):
    from finrl_amd import _native as nat
    assert lib.finenv_struct_size(26) == C.sizeof(nat.ReplayNStepPtrs) == 32
    assert lib.finenv_struct_size(25) == -1 and lib.finenv_struct_size(22) == -1
    assert lib.finenv_struct_size(27) == -1
    assert lib.finenv_struct_size(23) == C.sizeof(nat.ReplayViewPtrs) == 56
    assert lib.finenv_struct_size(24) == C.sizeof(nat.ReplayBatchPtrs) == 48
    assert lib.finenv_abi_version() == 3


def test_symbols_are_exported(lib):
    for name in ("finenv_replay_sample_nstep", "finenv_replay_gather_nstep"):
        assert hasattr(lib, name), name


def test_python_surface():
    import finrl_amd
    from finrl_amd.replay import ReplayBuffer
    assert finrl_amd.NStepReplayBufferSamples._fields == (
        "observations", "actions", "next_observations", "dones", "rewards", "discounts")
    assert finrl_amd.ReplayBufferSamples._fields == finrl_amd.NStepReplayBufferSamples._fields[:5]
    assert callable(ReplayBuffer.sample_nstep) and callable(ReplayBuffer.gather_nstep)


def test_nstep_entry_points_reject_bad_arguments(lib):
    for name in ("sample_nstep", "gather_nstep"):
        assert_refusals(lib, name)


# ------------------------------------------------------------------------------------------------
# hand-worked known answers of the model
# ------------------------------------------------------------------------------------------------
def _ring(S=6, E=2):
    """rewards 1, 2, 4 in slots 0, 1, 2 of env 0 (8, 16, 32 after them); obs[s][e] = [10 s + e]."""
    rew = np.zeros((S, E), np.float32)
    rew[:, 0] = [1, 2, 4, 8, 16, 32][:S]
    rew[:, 1] = -rew[:, 0]
    obs = (10.0 * np.arange(S)[:, None, None] + np.arange(E)[None, :, None]).astype(np.float32)
    act = -obs
    return obs, act, rew, np.zeros((S, E), np.uint8)


def test_model_three_steps_no_done():
    """1 + 0.5 * 2 + 0.25 * 4 = 3.0, discount 0.5^3, next observation three slots on."""
    obs, act, rew, done = _ring()
    o, a, nx, d, r, g, m = nm.nstep_lookup(obs, act, rew, done, np.array([[0], [0]]), pos=5, n=3, gamma=0.5)
    assert r.dtype == np.float32 and g.dtype == np.float32 and d.dtype == np.float32
    assert (r[0, 0], g[0, 0], d[0, 0], m[0]) == (3.0, 0.125, 0.0, 3)
    assert o[0, 0] == 0.0 and a[0, 0] == -0.0 and nx[0, 0] == 30.0


def test_model_done_on_the_second_step():
    """A done on the second step: 1 + 0.5 * 2 = 2.0, discount 0.25, done 1, next observation two on."""
    obs, act, rew, done = _ring()
    done[1, 0] = 1
    o, a, nx, d, r, g, m = nm.nstep_lookup(obs, act, rew, done, np.array([[0, 0], [0, 1]]), pos=5, n=3,
                                           gamma=0.5)
    assert (r[0, 0], g[0, 0], d[0, 0], m[0], nx[0, 0]) == (2.0, 0.25, 1.0, 2, 20.0)
    assert (r[1, 0], g[1, 0], d[1, 0], m[1], nx[1, 0]) == (-3.0, 0.125, 0.0, 3, 31.0)   # env 1: no done


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_model_newest_slot_gives_one_step(n):
    """A start that is the newest stored slot (pos - 1) has one stored step ahead: m = 1 whatever n,
    the reward is the stored one and the next observation is obs[pos]; one slot older gives min(n, 2).
    Also across the wrap (pos = 0: the newest slot is S - 1)."""
    obs, act, rew, done = _ring()
    S = obs.shape[0]
    for pos in (3, 0):
        newest, older = (pos - 1) % S, (pos - 2) % S
        o, a, nx, d, r, g, m = nm.nstep_lookup(obs, act, rew, done, np.array([[newest, older], [0, 0]]),
                                               pos=pos, n=n, gamma=0.5)
        assert m.tolist() == [1, min(n, 2)]
        assert r[0, 0] == rew[newest, 0] and g[0, 0] == np.float32(0.5) and nx[0, 0] == obs[pos, 0, 0]
        assert nx[1, 0] == obs[(older + m[1]) % S, 0, 0]


def test_model_n1_is_the_one_step_lookup():
    import replay_model as rm
    rng = np.random.default_rng(0)
    S, E = 5, 7
    obs = rng.normal(size=(S, E, 3)).astype(np.float32)
    act = rng.normal(size=(S, E, 2)).astype(np.float32)
    rew = rng.normal(size=(S, E)).astype(np.float32)
    done = (rng.random((S, E)) < 0.3).astype(np.uint8)
    pairs = np.stack([np.repeat(np.arange(S), E), np.tile(np.arange(E), S)])
    got = nm.nstep_lookup(obs, act, rew, done, pairs, pos=2, n=1, gamma=0.9)
    for g, w in zip(got[:5], rm.lookup(obs, act, rew, done, pairs)):
        np.testing.assert_array_equal(g, w)
    assert (got[5] == np.float32(0.9)).all() and (got[6] == 1).all()


def test_model_sum_is_float64_of_float32_powers():
    """gamma = 0.99: g_2 is fl32(fl32(0.99) * fl32(0.99)), not 0.99 ** 2 in double; the sum is in
    double and rounded once."""
    obs, act, rew, done = _ring()
    rew[:3, 0] = [1e6, -1e-3, 3.0]
    got = nm.nstep_lookup(obs, act, rew, done, np.array([[0], [0]]), pos=5, n=3, gamma=0.99)
    g1 = np.float32(0.99)
    g2 = np.float32(g1 * g1)
    want = np.float64(np.float32(1e6)) + np.float64(g1) * np.float64(np.float32(-1e-3)) \
        + np.float64(g2) * np.float64(np.float32(3.0))
    assert got[4][0, 0] == np.float32(want)
    assert got[5][0, 0] == np.float32(g2 * g1)
