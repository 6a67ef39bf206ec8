"""bench.py --dump-outputs, the writer alone on host tensors: names, dtypes, the 64 MB budget and the
fixed env sample shared by every array (tests/test_gpu_bench_contract.py runs it end to end)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Work:
    def __init__(self, E, D, axis=0):
        self.E, self.axis = E, axis
        ar = torch.arange(E, dtype=torch.float64)
        self.obs = ar[:, None].float().repeat(1, D)
        self.reward = ar.float() * 0.5
        self.done = (torch.arange(E) % 3 == 0).to(torch.uint8)
        self.cash = ar * 1.25

    def outputs(self):
        outs = dict(obs=self.obs, reward=self.reward, done=self.done, cash=self.cash)
        if self.axis:
            outs = {k: v.unsqueeze(0).repeat(2, *([1] * v.dim())) for k, v in outs.items()}
        return outs, self.axis


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_output_written_whole(tmp_path):
    w = _Work(100, 7)
    info = bench.dump_outputs(w, str(tmp_path))
    got = _load(str(tmp_path))
    assert sorted(got) == ["cash", "done", "obs", "reward"] and info["envs"] == 100
    assert got["obs"].dtype == np.float32 and got["reward"].dtype == np.float32
    assert got["done"].dtype == np.float32 and got["cash"].dtype == np.float64
    np.testing.assert_array_equal(got["obs"], w.obs.numpy())
    np.testing.assert_array_equal(got["done"], w.done.numpy().astype(np.float32))
    np.testing.assert_array_equal(got["cash"], w.cash.numpy())


@pytest.mark.parametrize("axis", [0, 1])
def test_large_output_sampled_within_budget(tmp_path, axis):
    E, D = 65536, 301                               # the headline batch: 79 MB of obs alone
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(_Work(E, D, axis), str(a))
    bench.dump_outputs(_Work(E, D, axis), str(b))
    ga, gb = _load(str(a)), _load(str(b))
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_BUDGET_BYTES + 4096
    rows = ga["reward"] * 2 if axis == 0 else ga["reward"][1] * 2          # reward = 0.5 * env index
    assert 0.25 * E < rows.size < E and np.all(np.diff(rows) > 0)      # a sorted sample, no repeats
    obs = ga["obs"] if axis == 0 else ga["obs"][0]
    cash = ga["cash"] if axis == 0 else ga["cash"][0]
    np.testing.assert_array_equal(obs[:, 0], rows)                     # one sample for every array
    np.testing.assert_array_equal(cash, rows * 1.25)
    for k in ga:
        np.testing.assert_array_equal(ga[k], gb[k])                    # the same sample each run


def test_refused_without_env_outputs():
    with pytest.raises(SystemExit, match="dump-outputs"):
        bench.main(["--env", "launcher-selftest", "--dump-outputs", "x"])
