"""CPU-side checks of the rollout minibatch's C ABI: the two new structs and their finenv_struct_size
indices, and the argument validation of finenv_rollout_minibatch, which refuses every bad call before
any HIP call (the addresses here are never dereferenced)."""
import ctypes as C

import pytest

from replay_abi_cases import FAKE, INV, lib  # noqa: F401

N_STEPS, E_VIEW = 5, 27           # M = 135


def _view(**kw):
    from finrl_amd import _native as nat
    good = dict(obs=FAKE, actions=FAKE, values=FAKE, log_probs=FAKE, advantages=FAKE, returns=FAKE,
                n_steps=N_STEPS, n_envs=E_VIEW, obs_dim=5, obs_pitch=8, action_dim=2, reserved0=0)
    return nat.RolloutViewPtrs(**dict(good, **kw))


def _batch(**kw):
    from finrl_amd import _native as nat
    good = dict(observations=FAKE, actions=FAKE, old_values=FAKE, old_log_prob=FAKE, advantages=FAKE,
                returns=FAKE, batch_size=7, obs_pitch=5)
    return nat.RolloutBatchPtrs(**dict(good, **kw))


def call(lib, view=True, batch=True, epoch=FAKE, first=0, rows=None):
    v = C.byref(_view() if view is True else view) if view is not None else None
    b = C.byref(_batch() if batch is True else batch) if batch is not None else None
    return lib.finenv_rollout_minibatch(v, epoch, 1, first, b, rows, None)


def test_struct_sizes_and_symbol(lib):
    from finrl_amd import _native as nat
    assert lib.finenv_struct_size(30) == C.sizeof(nat.RolloutViewPtrs) == 72
    assert lib.finenv_struct_size(31) == C.sizeof(nat.RolloutBatchPtrs) == 56
    assert lib.finenv_struct_size(29) == -1 and lib.finenv_struct_size(32) == -1
    assert lib.finenv_struct_size(28) == C.sizeof(nat.ReplayPerPtrs)
    assert lib.finenv_abi_version() == 3
    assert hasattr(lib, "finenv_rollout_minibatch")


def test_python_surface():
    import finrl_amd
    from finrl_amd.rollout import RolloutBuffer
    assert finrl_amd.RolloutBufferSamples._fields == (
        "observations", "actions", "old_values", "old_log_prob", "advantages", "returns")
    for name in ("minibatch", "next_epoch", "get", "collect", "step", "put",
                 "compute_returns_and_advantage"):
        assert callable(getattr(RolloutBuffer, name))


def test_null_arguments_are_refused(lib):
    assert call(lib, view=None) == INV
    assert call(lib, batch=None) == INV
    assert call(lib, epoch=None) == INV
    for name in ("obs", "actions", "values", "log_probs", "advantages", "returns"):
        assert call(lib, view=_view(**{name: None})) == INV, name
    for name in ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns"):
        assert call(lib, batch=_batch(**{name: None})) == INV, name


def test_bad_shapes_are_refused(lib):
    for kw in (dict(n_steps=0), dict(n_steps=-1), dict(n_envs=0), dict(n_envs=-4), dict(obs_dim=0),
               dict(action_dim=0), dict(obs_pitch=4), dict(obs_pitch=0)):
        assert call(lib, view=_view(**kw)) == INV, kw
    for kw in (dict(batch_size=0), dict(batch_size=-3), dict(obs_pitch=4)):
        assert call(lib, batch=_batch(**kw)) == INV, kw
    # n_steps * n_envs >= 2^31; 2^31 - 1 rows are fine as far as the row count goes (refused here only
    # for the position past them)
    assert call(lib, view=_view(n_steps=2 ** 16, n_envs=2 ** 15)) == INV
    assert call(lib, view=_view(n_steps=2 ** 20, n_envs=2 ** 20)) == INV
    assert call(lib, view=_view(n_steps=1, n_envs=2 ** 31 - 1), first=2 ** 31 - 7) == INV


def test_bad_positions_are_refused(lib):
    M = N_STEPS * E_VIEW
    for first, B in ((-1, 7), (M, 1), (M - 6, 7), (0, M + 1), (2 ** 31, 1), (2 ** 63 - 1, 7),
                     (-2 ** 63, 7)):
        assert call(lib, batch=_batch(batch_size=B), first=first) == INV, (first, B)


def test_minibatch_needs_a_gpu(lib):
    torch = pytest.importorskip("torch")
    from finrl_amd import RolloutBuffer
    from finrl_amd._native import FinenvError
    buf = RolloutBuffer(3, 5, 4, 2, device="cpu")
    assert buf.epochs == 0 and buf.epoch.dtype == torch.int64 and tuple(buf.epoch.shape) == (1,)
    with pytest.raises(FinenvError):
        buf.minibatch(0, 4)
