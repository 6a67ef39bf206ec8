"""What the three replay ABI test files share (no torch): the library fixture, well-formed structs
over an address that is never dereferenced, one table each of bad views, batches, n-step structs and
PER structs, and the six sampling entry points behind one calling form, so that every table is
applied to every entry point it concerns."""
import ctypes as C

import pytest

FAKE = 0x1000       # a non-null address that is never dereferenced: every call here is refused first
INV = -1            # FINENV_ERR_INVALID
S_VIEW, E_VIEW = 4, 3


@pytest.fixture(scope="module")
def lib():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def _struct(name, good, kw):
    from finrl_amd import _native as nat
    return getattr(nat, name)(**dict(good, **kw))


def _view(**kw):
    return _struct("ReplayViewPtrs", dict(obs=FAKE, actions=FAKE, rewards=FAKE, dones=FAKE, n_slots=S_VIEW,
                                          n_envs=E_VIEW, obs_dim=5, obs_pitch=8, action_dim=2,
                                          reserved0=0), kw)


def _batch(**kw):
    return _struct("ReplayBatchPtrs", dict(observations=FAKE, next_observations=FAKE, actions=FAKE,
                                           rewards=FAKE, dones=FAKE, batch_size=7, obs_pitch=5), kw)


def _nstep(**kw):
    return _struct("ReplayNStepPtrs", dict(head=FAKE, discounts=FAKE, steps=FAKE, n_steps=2, gamma=0.99),
                   kw)


def _per(**kw):
    return _struct("ReplayPerPtrs", dict(tickets=FAKE, tree=FAKE, max_ticket=FAKE, frac_bits=16,
                                         reserved0=0), kw)


BAD_VIEWS = [dict(obs=None), dict(actions=None), dict(rewards=None), dict(dones=None),
             dict(n_slots=1), dict(n_slots=0), dict(n_envs=0), dict(obs_dim=0), dict(action_dim=0),
             dict(obs_pitch=4)]
BAD_PER_VIEWS = [dict(n_slots=2 ** 16, n_envs=2 ** 15)]         # 2^31 leaves: fine without a tree
BAD_BATCHES = [dict(observations=None), dict(next_observations=None), dict(actions=None),
               dict(rewards=None), dict(dones=None), dict(batch_size=0), dict(batch_size=-3),
               dict(obs_pitch=4)]
BAD_NSTEPS = [dict(n_steps=0), dict(n_steps=-1), dict(n_steps=S_VIEW), dict(n_steps=S_VIEW + 5),
              dict(gamma=float("nan")), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("inf")),
              dict(gamma=float("-inf")), dict(head=None), dict(discounts=None)]
BAD_PERS = [dict(tickets=None), dict(tree=None), dict(max_ticket=None), dict(frac_bits=-1),
            dict(frac_bits=32)]

# entry point (after "finenv_replay_") -> the arguments it takes beside view and batch
SAMPLERS = {"sample": ("head", "draw"), "gather": ("indices",),
            "sample_nstep": ("head", "draw", "nstep"), "gather_nstep": ("indices", "nstep"),
            "per_sample": ("per", "draw"), "per_sample_nstep": ("per", "draw", "nstep")}


def call(lib, name, **kw):
    """finenv_replay_<name> with good arguments but for ``kw``: view / batch / nstep / per as a struct
    (passed by reference) or None, head / draw / indices as an address or None."""
    a = dict(view=_view(), batch=_batch(), nstep=_nstep(), per=_per(), head=FAKE, draw=FAKE, indices=FAKE)
    assert set(kw) <= {"view", "batch"} | set(SAMPLERS[name]), (name, kw)
    a.update(kw)
    v, b, n, p = (None if a[k] is None else C.byref(a[k]) for k in ("view", "batch", "nstep", "per"))
    ns = (n,) if "nstep" in SAMPLERS[name] else ()
    fn = getattr(lib, "finenv_replay_" + name)
    if "per" in SAMPLERS[name]:
        return fn(v, p, a["draw"], 1, b, *ns, None, None, None)
    if "head" in SAMPLERS[name]:
        return fn(v, a["head"], a["draw"], 1, b, *ns, None, None)
    return fn(v, a["indices"], b, *ns, None)


def assert_refusals(lib, name):
    """Every null argument and every entry of every table that concerns finenv_replay_<name>."""
    takes = SAMPLERS[name]
    for arg in ("view", "batch") + takes:
        assert call(lib, name, **{arg: None}) == INV, (name, arg)
    for kw in BAD_VIEWS + (BAD_PER_VIEWS if "per" in takes else []):
        assert call(lib, name, view=_view(**kw)) == INV, (name, kw)
    for kw in BAD_BATCHES:
        assert call(lib, name, batch=_batch(**kw)) == INV, (name, kw)
    if "per" in takes:
        for kw in BAD_PERS:
            assert call(lib, name, per=_per(**kw)) == INV, (name, kw)
    if "nstep" in takes:
        for kw in BAD_NSTEPS:
            assert call(lib, name, nstep=_nstep(**kw)) == INV, (name, kw)
        # the largest n a view admits is S - 1; a 2-slot ring admits only n = 1
        assert call(lib, name, view=_view(n_slots=2), nstep=_nstep(n_steps=2)) == INV, name
