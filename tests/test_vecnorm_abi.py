"""CPU-side checks of the running-statistics C ABI: the finenv_vecnorm struct and its
finenv_struct_size index, and the argument validation of finenv_vecnorm_update / _apply / _step /
_refresh, which refuse every bad call before any launch (the addresses here are never dereferenced)."""
import ctypes as C

import abi_header as H
from replay_abi_cases import FAKE, INV, lib  # noqa: F401

DIM, E = 5, 70
POINTERS = ("mean", "var", "scale", "count", "partials", "ticket")


def _stats(**kw):
    from finrl_amd import _native as nat
    good = dict(mean=FAKE, var=FAKE, scale=FAKE, count=FAKE, partials=FAKE, ticket=FAKE, dim=DIM,
                partials_cap=2 * nat.VECNORM_MAX_TILES * DIM, epsilon=1e-8, clip=10.0)
    good.update(kw)
    return nat.VecNormPtrs(**good)


def _ret(**kw):
    from finrl_amd import _native as nat
    return _stats(**dict(dict(dim=1, partials_cap=2 * nat.VECNORM_MAX_TILES), **kw))


def _ref(s):
    return None if s is None else C.byref(s)


def update(lib, stats=True, x=FAKE, n=E, pitch=8):
    return lib.finenv_vecnorm_update(_ref(_stats() if stats is True else stats), x, n, pitch, None)


def apply(lib, stats=True, x=FAKE, n=E, pitch_in=8, out=FAKE, pitch_out=DIM, center=1):
    return lib.finenv_vecnorm_apply(_ref(_stats() if stats is True else stats), x, n, pitch_in, out,
                                    pitch_out, center, None)


def step(lib, obs_stats=True, ret_stats=True, obs=FAKE, obs_pitch=8, reward=FAKE, done=FAKE, returns=FAKE,
         obs_out=FAKE, obs_out_pitch=DIM, reward_out=FAKE, done_out=None, n=E, training=1, norm_obs=1,
         norm_reward=1):
    return lib.finenv_vecnorm_step(
        _ref(_stats() if obs_stats is True else obs_stats), _ref(_ret() if ret_stats is True else ret_stats),
        obs, obs_pitch, reward, done, returns, 0.99, obs_out, obs_out_pitch, reward_out, done_out, n,
        training, norm_obs, norm_reward, None)


def test_struct_size_and_symbols(lib):
    from finrl_amd import _native as nat
    assert lib.finenv_struct_size(33) == C.sizeof(nat.VecNormPtrs) == 72
    assert lib.finenv_struct_size(32) == -1 and lib.finenv_struct_size(34) == -1
    assert lib.finenv_struct_size(31) == C.sizeof(nat.RolloutBatchPtrs)
    assert lib.finenv_abi_version() == 3
    for name in ("update", "apply", "step", "refresh"):
        assert hasattr(lib, "finenv_vecnorm_" + name)
    assert H.constants()["FINENV_VECNORM_MAX_TILES"] == nat.VECNORM_MAX_TILES


def test_python_surface():
    import finrl_amd
    from finrl_amd.vecnorm import RunningMeanStd, VecNormalize
    assert finrl_amd.VecNormalize is VecNormalize and finrl_amd.RunningMeanStd is RunningMeanStd
    for name in ("step", "reset", "get_original_obs", "get_original_reward", "normalize_obs",
                 "normalize_reward", "unnormalize_obs", "state_dict", "load_state_dict"):
        assert callable(getattr(VecNormalize, name))
    assert VecNormalize.supports_record is False


def test_null_arguments_are_refused(lib):
    assert update(lib, stats=None) == INV and update(lib, x=None) == INV
    assert apply(lib, stats=None) == INV and apply(lib, x=None) == INV and apply(lib, out=None) == INV
    assert lib.finenv_vecnorm_refresh(None, None) == INV
    for name in POINTERS:
        bad = _stats(**{name: None})
        assert update(lib, stats=bad) == INV, name
        assert apply(lib, stats=bad) == INV, name
        assert step(lib, obs_stats=bad) == INV, name
        assert step(lib, ret_stats=_ret(**{name: None})) == INV, name
        assert lib.finenv_vecnorm_refresh(C.byref(bad), None) == INV, name
    assert step(lib, obs_stats=None) == INV and step(lib, ret_stats=None) == INV
    for name in ("obs", "reward", "done", "returns", "obs_out", "reward_out"):
        assert step(lib, **{name: None}) == INV, name


def test_bad_shapes_are_refused(lib):
    for dim in (0, -1):
        assert update(lib, stats=_stats(dim=dim)) == INV
        assert apply(lib, stats=_stats(dim=dim)) == INV
        assert step(lib, obs_stats=_stats(dim=dim)) == INV
        assert lib.finenv_vecnorm_refresh(C.byref(_stats(dim=dim)), None) == INV
    for n in (0, -1, -2 ** 40):
        assert update(lib, n=n) == INV and apply(lib, n=n) == INV
    for n in (0, -1):
        assert step(lib, n=n) == INV
    for pitch in (DIM - 1, 0, -8):
        assert update(lib, pitch=pitch) == INV
        assert apply(lib, pitch_in=pitch) == INV and apply(lib, pitch_out=pitch) == INV
        assert step(lib, obs_pitch=pitch) == INV and step(lib, obs_out_pitch=pitch) == INV
    assert step(lib, ret_stats=_ret(dim=2, partials_cap=1024)) == INV        # the return stats are one column


def test_small_partials_are_refused(lib):
    """70 rows of 5 columns at pitch 8 from a 16-byte aligned base move as 16-byte units: 2 unit-lanes,
    512 row-lanes, one tile of 512 rows -> 2 * 1 * 5 doubles; 70,001 rows make 69 tiles of 1,024 -> 690."""
    assert update(lib, stats=_stats(partials_cap=9)) == INV
    assert update(lib, stats=_stats(partials_cap=0)) == INV
    assert update(lib, stats=_stats(partials_cap=689), n=70001) == INV
    assert step(lib, obs_stats=_stats(partials_cap=9)) == INV
    assert step(lib, ret_stats=_ret(partials_cap=1)) == INV
