"""NumPy restatement of the replay buffer's sampler (include/finenv.h, "Replay buffer"): the
Philox4x32-10 draw of (slot, env) pairs and the lookup (slot, env) -> the five rows of a batch.  A
helper of the replay tests, not a test."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two -> the four output words as
    uint64 arrays holding 32-bit values (Salmon et al., SC'11; Random123 philox4x32, 10 rounds)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)           # 32 x 32 -> 64 bits, exact
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def valid_slots(pos, n_valid, S):
    """The slots holding a complete transition, newest first: (pos - 1 - j) mod S, j < n_valid."""
    return [(pos - 1 - j) % S for j in range(n_valid)]


def head_after(n_steps, S):
    """(pos, n_valid) after n_steps stored steps of a fresh ring."""
    return n_steps % S, min(n_steps, S - 1)


def draw_pairs(seed, draw, B, pos, n_valid, S, E):
    """int32 [2, B]: the pairs finenv_replay_sample draws for (seed, draw number, head)."""
    i = np.arange(B, dtype=np.uint64)
    x = philox4x32_10((i, 0, draw & MASK, (draw >> 32) & MASK), (seed & MASK, (seed >> 32) & MASK))
    j = ((x[0] * np.uint64(max(n_valid, 1))) >> np.uint64(32)).astype(np.int64)
    slot = (pos - 1 - j) % S
    env = ((x[1] * np.uint64(E)) >> np.uint64(32)).astype(np.int64)
    return np.stack([slot, env]).astype(np.int32)


def lookup(obs, actions, rewards, dones, pairs):
    """The batch of `pairs` (int [2, B]) from host copies of the ring: obs [S, E, D] (the view without
    pad columns), actions [S, E, A], rewards [S, E], dones [S, E] -> observations, actions,
    next_observations, dones [B, 1] f32, rewards [B, 1] (SB3's ReplayBufferSamples order)."""
    S = obs.shape[0]
    s, e = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    return (obs[s, e], actions[s, e], obs[(s + 1) % S, e],
            dones[s, e].astype(np.float32)[:, None], rewards[s, e][:, None])


def gather_group(D, view_pitch, out_pitch, bases):
    """(lanes per sample, bytes per unit) the sampler takes for rows of D floats: 16-byte units when
    D >= 4, both pitches are multiples of 4 floats and the three observation bases are 16-byte
    aligned, else dwords; the lanes are the smallest power of two in [4, 64] with 2 G >= units."""
    vec = D >= 4 and view_pitch % 4 == 0 and out_pitch % 4 == 0 and all(b % 16 == 0 for b in bases)
    units = (D + 3) // 4 if vec else D
    G = 4
    while G < 64 and 2 * G < units:
        G *= 2
    return G, 16 if vec else 4
