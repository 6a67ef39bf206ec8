"""NumPy restatement of the replay buffer's n-step sampler (include/finenv.h, "n-step returns"): the
horizon, the length, the discounted return (float32 powers of gamma, float64 sum in increasing step
order) and the look-up of the late next observation.  The draw is the one-step sampler's
(replay_model.draw_pairs).  A helper of the n-step replay tests, not a test."""
import numpy as np

from replay_model import draw_pairs  # noqa: F401  (the n-step draw IS the one-step draw)


def clamp_n_valid(n_valid, S):
    """n_valid as the draw takes it: into [1, S - 1]."""
    return min(max(int(n_valid), 1), S - 1)


def horizon(pos, slots, n, S):
    """h = min(n, ((pos - 1 - s) mod S) + 1), mod non-negative, per start slot."""
    s = np.asarray(slots, dtype=np.int64)
    return np.minimum(n, (int(pos) - 1 - s) % S + 1)


def nstep_lookup(obs, actions, rewards, dones, pairs, pos, n, gamma):
    """The n-step batch of `pairs` (int [2, B]) from host copies of the ring (as replay_model.lookup)
    and the head word `pos` -> observations, actions, next_observations, dones [B, 1] f32,
    rewards [B, 1] f32, discounts [B, 1] f32, steps [B] int32."""
    S = obs.shape[0]
    s, e = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    B = s.shape[0]
    h = horizon(pos, s, n, S)
    gam = np.float32(gamma)
    g = np.ones(B, dtype=np.float32)                # g_i, one float32 multiply per step
    acc = np.zeros(B, dtype=np.float64)
    m = np.zeros(B, dtype=np.int32)
    last_done = np.zeros(B, dtype=np.uint8)
    disc = np.ones(B, dtype=np.float32)
    alive = np.ones(B, dtype=bool)                  # no done yet and i < h
    for i in range(n):
        on = alive & (i < h)
        si = (s + i) % S
        term = g.astype(np.float64) * rewards[si, e].astype(np.float64)     # exact
        acc = np.where(on, term if i == 0 else acc + term, acc)
        g = g * gam
        assert g.dtype == np.float32
        m = np.where(on, i + 1, m).astype(np.int32)
        last_done = np.where(on, dones[si, e], last_done).astype(np.uint8)
        disc = np.where(on, g, disc)
        alive = on & (dones[si, e] == 0)
    return (obs[s, e], actions[s, e], obs[(s + m) % S, e], last_done.astype(np.float32)[:, None],
            acc.astype(np.float32)[:, None], disc[:, None], m)


def end_kinds(rewards, dones, pairs, pos, n):
    """Per pair, how its return ended: (m, by_done, by_head) -- by_done: the step m-1 has a done;
    by_head: no done and m = h < n."""
    S = dones.shape[0]
    s, e = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    h = horizon(pos, s, n, S)
    m = nstep_lookup(np.zeros((S, dones.shape[1], 1), np.float32), np.zeros((S, dones.shape[1], 1), np.float32),
                     rewards, dones, pairs, pos, n, 1.0)[6]
    by_done = dones[(s + m - 1) % S, e] != 0
    return m, by_done, (~by_done) & (m == h) & (h < n)
