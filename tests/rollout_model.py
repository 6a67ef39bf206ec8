"""NumPy restatement of the rollout buffer's shuffled minibatches (include/finenv.h, "Shuffled
minibatches"): the stateless permutation -- four Feistel rounds of Philox4x32-10 over the bits of
M - 1, cycle-walked into [0, M) -- and the lookup row -> the six fields of a batch.  A helper of the
rollout minibatch tests, not a test."""
import numpy as np

from replay_model import MASK, philox4x32_10


def perm(i, M, epoch, seed, walks=None):
    """Rows (int64, the shape of ``i`` broadcast with ``epoch``) of positions ``i`` in [0, M) of epoch
    ``epoch`` (ints or arrays) under ``seed``.  ``walks``: a list that receives the array of passes
    each position took (1 = no walk)."""
    i, epoch = np.broadcast_arrays(np.asarray(i, dtype=np.uint64), np.asarray(epoch, dtype=np.uint64))
    assert M >= 1 and (i < M).all()
    if M == 1:
        if walks is not None:
            walks.append(np.zeros(i.shape, dtype=np.int64))
        return np.zeros(i.shape, dtype=np.int64)
    bits = max(2, int(M - 1).bit_length())
    a = bits // 2
    b = bits - a
    ma, mb = np.uint64((1 << a) - 1), np.uint64((1 << b) - 1)
    key = (seed & MASK, (seed >> 32) & MASK)

    def rounds(x, n):
        L, R = x >> np.uint64(a), x & ma
        n_lo, n_hi = n & np.uint64(MASK), n >> np.uint64(32)
        for r in range(4):
            if r % 2 == 0:
                L = L ^ (philox4x32_10((R, r, n_lo, n_hi), key)[0] & mb)
            else:
                R = R ^ (philox4x32_10((L, r, n_lo, n_hi), key)[0] & ma)
        return (L << np.uint64(a)) | R

    x, n = i.reshape(-1).copy(), epoch.reshape(-1)
    passes = np.zeros(x.shape, dtype=np.int64)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        x[todo] = rounds(x[todo], n[todo])
        passes[todo] += 1
        todo = x >= np.uint64(M)
    if walks is not None:
        walks.append(passes.reshape(i.shape))
    return x.astype(np.int64).reshape(i.shape)


def minibatch_rows(k, batch_size, M, epoch, seed):
    """int32 [n]: the rows of minibatch k of an epoch, n = min(batch_size, M - k * batch_size)."""
    first = k * batch_size
    return perm(np.arange(first, min(first + batch_size, M)), M, epoch, seed).astype(np.int32)


def minibatch_lookup(obs, actions, values, log_probs, advantages, returns, rows):
    """The batch of flat ``rows`` (t * E + e) from host copies of the rollout tensors: obs
    [n_steps + 1, E, D] (the view without pad columns), actions [n_steps, E, A], the four scalar
    fields [n_steps, E] -> observations [B, D], actions [B, A], old_values, old_log_prob, advantages,
    returns [B] (SB3's RolloutBufferSamples order)."""
    r = np.asarray(rows, dtype=np.int64)
    return tuple(x.reshape((-1,) + x.shape[2:])[r]
                 for x in (obs, actions, values, log_probs, advantages, returns))
