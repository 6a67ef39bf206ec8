"""CPU-side checks of the NumPy model of the rollout buffer's permutation (tests/rollout_model.py):
it is a bijection of [0, M) at every size, changes with the epoch, and at the sizes where the contract
claims it (M >= 16) spreads every position over every row like a uniform permutation would."""
import numpy as np
import pytest

import rollout_model as rom

SEED = 7
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 17, 33, 65, 80, 131, 393, 4097, 65536, 2 ** 20 + 1]


@pytest.mark.parametrize("M", SIZES)
def test_perm_is_a_bijection(M):
    for epoch in (0, 1, 5):
        walks = []
        rows = rom.perm(np.arange(M), M, epoch, SEED, walks=walks)
        assert rows.dtype == np.int64 and rows.shape == (M,)
        assert rows.min() == 0 and rows.max() == M - 1
        assert (np.bincount(rows, minlength=M) == 1).all()
        if M & (M - 1) == 0 and M >= 4:                      # a power of two fills its bits: no walk
            assert walks[0].max() == 1


@pytest.mark.parametrize("M", [m for m in SIZES if m >= 16])
def test_epochs_differ(M):
    i = np.arange(M)
    assert not np.array_equal(rom.perm(i, M, 0, SEED), rom.perm(i, M, 1, SEED))


def test_perm_is_elementwise_in_position_and_epoch():
    """The vectorised form over arrays of positions and epochs equals the scalar form per element,
    the high word of the epoch and of the seed included."""
    M, seed = 393, (5 << 32) | 9
    i = np.array([0, 1, 200, 392])
    n = np.array([0, 3, 2 ** 32, 2 ** 40 + 1], dtype=np.uint64)
    got = rom.perm(i[:, None], M, n[None, :], seed)
    for a, pos in enumerate(i):
        for b, epoch in enumerate(n):
            assert got[a, b] == rom.perm(int(pos), M, int(epoch), seed)
    assert len({tuple(got[:, b]) for b in range(4)}) == 4


def test_one_row():
    assert rom.perm(np.zeros(3, dtype=np.int64), 1, 9, SEED).tolist() == [0, 0, 0]
    assert rom.minibatch_rows(0, 1, 1, 0, SEED).tolist() == [0]


def test_minibatch_rows_cover_an_epoch():
    M, B = 135, 50
    parts = [rom.minibatch_rows(k, B, M, 2, SEED) for k in range(3)]
    assert [p.size for p in parts] == [50, 50, 35] and parts[0].dtype == np.int32
    assert sorted(np.concatenate(parts).tolist()) == list(range(M))


@pytest.mark.parametrize("M", [48, 80])
def test_positions_spread_uniformly_over_rows(M):
    """K = 16,384 epochs: the count of every (position, row) pair is Binomial(K, 1 / M) under a
    uniform permutation, sigma = sqrt(K / M * (1 - 1 / M)).  Every count within 6 sigma of K / M
    (the M * M counts of a uniform permutation would stay within about 4.3)."""
    K = 16384
    rows = rom.perm(np.arange(M)[:, None], M, np.arange(K)[None, :], SEED)        # [M, K]
    counts = np.zeros((M, M), dtype=np.int64)
    np.add.at(counts, (np.repeat(np.arange(M), K), rows.reshape(-1)), 1)
    assert (counts.sum(0) == K).all() and (counts.sum(1) == K).all()
    sigma = np.sqrt(K / M * (1 - 1 / M))
    worst = np.abs(counts - K / M).max() / sigma
    print(f"M = {M}: worst (position, row) count {worst:.2f} sigma from K / M")
    assert worst <= 6.0
