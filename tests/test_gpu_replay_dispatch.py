"""The sampler's dispatch table on the MI355X: every lane-group width x unit size, under each of the
three draw sources and both return forms (60 instantiations of one kernel), each against the NumPy
models with tolerance 0."""
import numpy as np
import pytest

import replay_model as rm
import replay_nstep_model as nm
import replay_per_model as pm
from replay_cases import (RING_SEED, assert_batch, coded_ring, need_gpu, per_ring, random_tickets, set_head,
                          set_tickets)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# D, P, A -> bytes per unit, lanes per sample
SHAPES = [(3, 3, 6, 4, 4),              # action floats past G go through the loop behind the stores
          (13, 13, 3, 4, 8),
          (20, 21, 1, 4, 16),
          (51, 51, 10, 4, 32),
          (130, 131, 70, 4, 64),        # two units and six action floats through that loop
          (5, 16, 1, 16, 4),            # tail of 1
          (40, 40, 3, 16, 8),
          (100, 112, 3, 16, 16),
          (160, 160, 3, 16, 32),
          (301, 304, 30, 16, 64),       # tail of 1
          (518, 520, 3, 16, 64)]        # one unit through the loop, tail of 2


@pytest.mark.parametrize("D,P,A,unit,G", SHAPES)
def test_every_sampler_instantiation_equals_model(D, P, A, unit, G):
    """S = 5, E = 3, B = 131: several blocks with a partial last one at every G.  The shape lands on
    the (G, unit) the table names (the rule of the launch, restated in replay_model.gather_group),
    and sample / gather / sample_nstep / gather_nstep and the prioritised sample / sample_nstep equal
    the models: batch, last_indices, last_steps, discounts and probabilities."""
    need_gpu()
    S, E, B, n, gamma, seed = 5, 3, 131, 3, 0.9, 7
    pos, n_valid = rm.head_after(S + 1, S)
    buf, host = coded_ring(S, E, D, P, A, seed=seed, ring_seed=RING_SEED)
    per, _ = per_ring(S, E, D, P, A, seed=seed, ring_seed=RING_SEED)
    t = random_tickets(S, E, D)
    t[pos] = 0
    set_tickets(per, t)
    rng = np.random.default_rng(D)
    pairs = np.stack([rng.integers(0, S, B), rng.integers(0, E, B)]).astype(np.int32)
    idx = torch.from_numpy(pairs).cuda()

    def check(b, smp, want, tag, steps=None):
        bases = (b._obs_buf.data_ptr(), smp.observations.data_ptr(), smp.next_observations.data_ptr())
        assert rm.gather_group(D, b.obs_pitch, b.obs_pitch, bases) == (G, unit), tag
        assert_batch(smp, want, tag, steps=steps)

    set_head(buf, pos, n_valid)
    set_head(per, pos, n_valid)
    check(buf, buf.gather(idx), rm.lookup(*host, pairs), "gather")
    check(buf, buf.gather_nstep(idx, n, gamma), nm.nstep_lookup(*host, pairs, pos, n, gamma), "gather_nstep",
          steps=buf.last_steps)

    drawn = rm.draw_pairs(seed, 0, B, pos, n_valid, S, E)
    check(buf, buf.sample(B), rm.lookup(*host, drawn), "sample")
    np.testing.assert_array_equal(buf.last_indices.cpu().numpy(), drawn)
    drawn = rm.draw_pairs(seed, 1, B, pos, n_valid, S, E)
    check(buf, buf.sample_nstep(B, n, gamma), nm.nstep_lookup(*host, drawn, pos, n, gamma), "sample_nstep",
          steps=buf.last_steps)
    np.testing.assert_array_equal(buf.last_indices.cpu().numpy(), drawn)

    drawn, prob = pm.draw_pairs(seed, 0, B, t, E)
    assert pos not in set(drawn[0].tolist())
    check(per, per.sample(B), rm.lookup(*host, drawn) + (prob[:, None],), "prioritised sample")
    np.testing.assert_array_equal(per.last_indices.cpu().numpy(), drawn)
    drawn, prob = pm.draw_pairs(seed, 1, B, t, E)
    want = nm.nstep_lookup(*host, drawn, pos, n, gamma)
    check(per, per.sample_nstep(B, n, gamma), want[:6] + (prob[:, None], want[6]), "prioritised sample_nstep",
          steps=per.last_steps)
    np.testing.assert_array_equal(per.last_indices.cpu().numpy(), drawn)
