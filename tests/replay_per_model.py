"""NumPy restatement of prioritised replay (include/finenv.h, "Prioritised replay"): the ticket rule,
the fan-out-64 tree in its stated layout, the selection by searchsorted, the draw, the probabilities
and the fill and update rules.  Everything is integer, so every comparison against it is exact.  A
helper of the prioritised replay tests, not a test."""
import numpy as np

from replay_model import MASK, philox4x32_10

FAN = 64
TOP = 2 ** 32 - 1


def ticket(w, frac_bits):
    """uint32 tickets of shaped priorities w (float32): 1 unless w > 0, else rint(w * 2^F) in double
    (exact; ties to even) clamped into [1, 2^32 - 1]."""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint(w.astype(np.float64) * float(2 ** int(frac_bits)))
        x = np.minimum(np.maximum(x, 1.0), float(TOP))
    return np.where(w > 0, x, 1.0).astype(np.uint64).astype(np.uint32)


def level_sizes(n_leaves):
    """[n_1, n_2, ..., 1]: nodes per level, bottom-up."""
    sizes, n = [], int(n_leaves)
    while True:
        n = (n + FAN - 1) // FAN
        sizes.append(n)
        if n == 1:
            return sizes


def tree_words(n_leaves):
    return sum(level_sizes(n_leaves)) if 1 <= n_leaves <= 2 ** 31 - 1 else -1


def build_tree(tickets):
    """uint64 [words]: every node the sum of its (up to 64) children, levels stored top-down."""
    cur = np.asarray(tickets, dtype=np.uint32).reshape(-1).astype(np.uint64)
    levels = []
    while True:
        pad = (-cur.size) % FAN
        cur = np.concatenate([cur, np.zeros(pad, np.uint64)]).reshape(-1, FAN).sum(axis=1, dtype=np.uint64)
        levels.append(cur)
        if cur.size == 1:
            return np.concatenate(levels[::-1])


def total(tickets):
    return int(np.asarray(tickets, dtype=np.uint32).astype(np.uint64).sum(dtype=np.uint64))


def find_leaves(tickets, u):
    """The leaves selected by the values u (Python ints or uint64): u is taken as min(u, total - 1);
    total == 0 gives leaf 0."""
    c = np.cumsum(np.asarray(tickets, dtype=np.uint32).reshape(-1).astype(np.uint64), dtype=np.uint64)
    tot = int(c[-1])
    if tot == 0:
        return np.zeros(len(u), dtype=np.int64)
    uu = np.array([min(int(x), tot - 1) for x in u], dtype=np.uint64)
    return np.searchsorted(c, uu, side="right").astype(np.int64)


def pairs_of(leaves, E):
    leaves = np.asarray(leaves, dtype=np.int64)
    return np.stack([leaves // E, leaves % E]).astype(np.int32)


def draw_u(seed, draw, B, tot):
    """u of sample i: umul64hi((x0 << 32) | x1, total) of the uniform draw's Philox words."""
    i = np.arange(B, dtype=np.uint64)
    x = philox4x32_10((i, 0, draw & MASK, (draw >> 32) & MASK), (seed & MASK, (seed >> 32) & MASK))
    return [(((int(a) << 32) | int(b)) * int(tot)) >> 64 for a, b in zip(x[0], x[1])]


def draw_pairs(seed, draw, B, tickets, E):
    """(int32 [2, B] pairs, float32 [B] probabilities) of finenv_replay_per_sample."""
    flat = np.asarray(tickets, dtype=np.uint32).reshape(-1)
    tot = total(flat)
    leaves = find_leaves(flat, draw_u(seed, draw, B, tot))
    prob = (flat[leaves].astype(np.float64) / np.float64(tot)).astype(np.float32)
    return pairs_of(leaves, E), prob


def put(tickets, max_ticket, pos, pos_next):
    """The fill rule on tickets [S, E] (a copy is returned): slot pos takes max_ticket (0 taken as 1),
    slot pos_next takes 0 unless it is pos."""
    t = np.array(tickets, dtype=np.uint32)
    t[pos] = max(int(max_ticket), 1)
    if pos_next != pos:
        t[pos_next] = 0
    return t


def update(tickets, max_ticket, pairs, w, frac_bits):
    """The write-back for DISTINCT pairs or duplicates of equal value -> (tickets, max_ticket): a leaf
    at 0 stays 0, any other takes its entry's ticket; max_ticket covers every entry."""
    t = np.array(tickets, dtype=np.uint32)
    S, E = t.shape
    q = ticket(w, frac_bits)
    s = np.clip(np.asarray(pairs[0], dtype=np.int64), 0, S - 1)
    e = np.clip(np.asarray(pairs[1], dtype=np.int64), 0, E - 1)
    live = t[s, e] != 0
    t[s[live], e[live]] = q[live]
    return t, max(int(max_ticket), int(q.max()))
