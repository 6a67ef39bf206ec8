"""CPU-side checks of prioritised replay: the new ABI struct and symbols, the tree size rule, the
argument validation of the finenv_replay_per_* entry points (refused before any launch), and
hand-worked known answers of the NumPy model (tests/replay_per_model.py)."""
import ctypes as C

import numpy as np
import pytest

import replay_per_model as pm
from replay_abi_cases import BAD_PERS, E_VIEW, FAKE, INV, S_VIEW, _per, assert_refusals, lib  # noqa: F401

NAMES = ("tree_words", "rebuild", "put", "update", "find", "sample", "sample_nstep")


def test_struct_sizes_and_symbols(lib):
    from finrl_amd import _native as nat
    assert lib.finenv_struct_size(28) == C.sizeof(nat.ReplayPerPtrs) == 32
    assert lib.finenv_struct_size(27) == -1 and lib.finenv_struct_size(29) == -1
    assert lib.finenv_struct_size(26) == C.sizeof(nat.ReplayNStepPtrs)
    assert lib.finenv_abi_version() == 3
    for name in NAMES:
        assert hasattr(lib, "finenv_replay_per_" + name), name


def test_python_surface():
    import finrl_amd
    from finrl_amd.replay import PrioritizedReplayBuffer, ReplayBuffer
    assert issubclass(finrl_amd.PrioritizedReplayBuffer, ReplayBuffer)
    assert finrl_amd.PrioritizedReplayBufferSamples._fields == \
        finrl_amd.ReplayBufferSamples._fields + ("probabilities",)
    assert finrl_amd.PrioritizedNStepReplayBufferSamples._fields == \
        finrl_amd.NStepReplayBufferSamples._fields + ("probabilities",)
    for name in ("update_priorities", "importance_weights", "find", "rebuild", "sample", "sample_nstep"):
        assert callable(getattr(PrioritizedReplayBuffer, name))
    assert PrioritizedReplayBuffer.gather is ReplayBuffer.gather
    assert PrioritizedReplayBuffer.gather_nstep is ReplayBuffer.gather_nstep


@pytest.mark.parametrize("n,want", [(1, 1), (64, 1), (65, 3), (4096, 65), (4097, 1 + 2 + 65),
                                    (4617, 76), (2 ** 31 - 1, 1 + 2 + 128 + 8192 + 524288 + 33554432),
                                    (0, -1), (2 ** 31, -1), (-5, -1)])
def test_tree_words(lib, n, want):
    assert lib.finenv_replay_per_tree_words(n) == want
    assert pm.tree_words(n) == want


def test_tree_entry_points_reject_bad_arguments(lib):
    good = _per()
    S, E = S_VIEW, E_VIEW
    calls = {
        "rebuild": lambda p, S=S, E=E: lib.finenv_replay_per_rebuild(p, S, E, None),
        "put": lambda p, S=S, E=E, pos=1, nxt=2: lib.finenv_replay_per_put(p, S, E, pos, nxt, None),
        "update": lambda p, S=S, E=E, idx=FAKE, w=FAKE, B=7:
            lib.finenv_replay_per_update(p, S, E, idx, w, B, None),
        "find": lambda p, S=S, E=E, u=FAKE, B=7, out=FAKE:
            lib.finenv_replay_per_find(p, S, E, u, B, out, None),
    }
    for name, f in calls.items():
        assert f(None) == INV, name
        for kw in BAD_PERS:
            assert f(C.byref(_per(**kw))) == INV, (name, kw)
        for s, e in ((1, 3), (0, 3), (-2, 3), (4, 0), (4, -1), (2 ** 16, 2 ** 15)):   # S < 2, E < 1, N = 2^31
            assert f(C.byref(good), S=s, E=e) == INV, (name, s, e)
    put, update, find = calls["put"], calls["update"], calls["find"]
    for pos, nxt in ((-1, 2), (S, 2), (1, -1), (1, S), (S + 7, S + 8)):
        assert put(C.byref(good), pos=pos, nxt=nxt) == INV, (pos, nxt)
    for B in (0, -3):
        assert update(C.byref(good), B=B) == INV and find(C.byref(good), B=B) == INV
    assert update(C.byref(good), idx=None) == INV and update(C.byref(good), w=None) == INV
    assert find(C.byref(good), u=None) == INV and find(C.byref(good), out=None) == INV


def test_sample_entry_points_reject_bad_arguments(lib):
    for name in ("per_sample", "per_sample_nstep"):
        assert_refusals(lib, name)


def test_prioritized_buffer_needs_a_gpu(lib):
    pytest.importorskip("torch")
    from finrl_amd import PrioritizedReplayBuffer
    from finrl_amd._native import FinenvError
    with pytest.raises(FinenvError):
        PrioritizedReplayBuffer(4, 3, 5, 2, device="cpu")


# ------------------------------------------------------------------------------------------------
# hand-worked known answers of the model
# ------------------------------------------------------------------------------------------------
def test_model_three_leaves():
    """Tickets 1, 0, 3: u = 0 is leaf 0; u = 1, 2, 3 fall in leaf 2; the zero leaf is never selected;
    u past the total is taken as total - 1."""
    t = np.array([1, 0, 3], dtype=np.uint32)
    assert pm.total(t) == 4
    assert pm.find_leaves(t, [0, 1, 3]).tolist() == [0, 2, 2]
    assert pm.find_leaves(t, [2, 4, 2 ** 64 - 1]).tolist() == [2, 2, 2]
    assert pm.build_tree(t).tolist() == [4]
    assert pm.find_leaves(np.zeros(3, np.uint32), [0, 5]).tolist() == [0, 0]
    assert pm.pairs_of([0, 5, 14], 5).tolist() == [[0, 1, 2], [0, 0, 4]]


def test_model_ticket_clamps():
    w = np.array([np.nan, 0.0, -1.0, 1e-9, np.inf, 1.0, 65535.99999, 70000.0], dtype=np.float32)
    assert pm.ticket(w, 16).tolist() == [1, 1, 1, 1, 2 ** 32 - 1, 65536, 2 ** 32 - 1, 2 ** 32 - 1]
    assert pm.ticket(np.float32(2.0 ** 31), 0).tolist() == 2 ** 31
    assert pm.ticket(np.float32(2.0 ** 32), 0).tolist() == 2 ** 32 - 1
    assert pm.ticket(np.float32(1.0), 31).tolist() == 2 ** 31
    assert pm.ticket(np.float32(-0.0), 31).tolist() == 1


def test_model_rint_ties_go_to_even():
    """F = 1: w * 2 = 0.5, 1.5, 2.5, 3.5 -> 0 (then clamped to 1), 2, 2, 4."""
    w = np.array([0.25, 0.75, 1.25, 1.75, 2.25], dtype=np.float32)
    assert pm.ticket(w, 1).tolist() == [1, 2, 2, 4, 4]
    assert pm.ticket(np.float32(2.5), 0).tolist() == 2 and pm.ticket(np.float32(3.5), 0).tolist() == 4


def test_model_tree_layout():
    """N = 4617 all ones: root 4617, then the two level-2 nodes 4096 and 521, then 73 level-1 nodes
    (72 of 64 and one of 9)."""
    tree = pm.build_tree(np.ones(4617, np.uint32))
    assert tree.size == 76 and tree.dtype == np.uint64
    assert tree[:3].tolist() == [4617, 4096, 521]
    assert tree[3:75].tolist() == [64] * 72 and tree[75] == 9
    big = pm.build_tree(np.full(65, 2 ** 32 - 1, np.uint32))
    assert big.tolist() == [65 * (2 ** 32 - 1), 64 * (2 ** 32 - 1), 2 ** 32 - 1]


def test_model_fill_and_update_rules():
    t = np.zeros((3, 2), np.uint32)
    t = pm.put(t, 0, 0, 1)                       # max_ticket 0 is taken as 1
    assert t.tolist() == [[1, 1], [0, 0], [0, 0]]
    t = pm.put(t, 7, 1, 2)
    t = pm.put(t, 7, 2, 0)                       # the ring is full: slot 0 is excluded again
    assert t.tolist() == [[0, 0], [7, 7], [7, 7]]
    assert pm.put(t, 9, 1, 1).tolist() == [[0, 0], [9, 9], [7, 7]]          # pos_next == pos: nothing zeroed
    pairs = np.array([[0, 1, 5, 2], [0, 1, -4, 1]])
    w = np.array([3.0, 2.0, np.nan, 0.5], np.float32)
    got, top = pm.update(t, 7, pairs, w, 2)
    assert got.tolist() == [[0, 0], [7, 8], [1, 2]] and top == 12          # the dropped entry counts in max


def test_model_draw_is_proportional_and_skips_zero_leaves():
    t = np.array([[0, 0, 0], [5, 1, 0], [0, 2, 8]], dtype=np.uint32)
    pairs, prob = pm.draw_pairs(7, 3, 4096, t, 3)
    assert prob.dtype == np.float32
    leaves = pairs[0].astype(np.int64) * 3 + pairs[1]
    flat = t.reshape(-1)
    assert (flat[leaves] != 0).all()
    np.testing.assert_array_equal(prob, (flat[leaves] / 16.0).astype(np.float32))
    share = np.bincount(leaves, minlength=9) / 4096.0
    np.testing.assert_allclose(share, flat / 16.0, atol=0.03)   # 4 sigma of the largest share is 0.031
    assert not np.array_equal(pairs, pm.draw_pairs(7, 4, 4096, t, 3)[0])
