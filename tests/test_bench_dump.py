"""bench.py --dump-outputs on CPU (a stand-in core, no GPU): the last step's obs_buf / rew_buf / reset_buf land as float32
DIR/<name>.npy; above the size limit, the rows of a fixed seeded sample of the envs, with their indices in env_index.npy."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _core(n, num_obs=158):
    g = torch.Generator().manual_seed(0)
    return types.SimpleNamespace(N=n, obs_buf=torch.randn(n, num_obs, generator=g), rew_buf=torch.randn(n, generator=g),
                                 reset_buf=torch.rand(n, generator=g) > 0.5)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_output_as_float32(tmp_path):
    core = _core(4096)
    bench.dump_outputs(str(tmp_path), core)
    got = _load(str(tmp_path))
    assert sorted(got) == ["obs", "reset", "rew"]
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["obs"], core.obs_buf.numpy())
    np.testing.assert_array_equal(got["rew"], core.rew_buf.numpy())
    np.testing.assert_array_equal(got["reset"], core.reset_buf.numpy().astype(np.float32))


def test_dump_above_the_limit_is_a_fixed_sample(tmp_path):
    core, limit = _core(4096), 300_000
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        bench.dump_outputs(d, core, limit=limit)
    a, b = _load(dirs[0]), _load(dirs[1])
    assert sorted(a) == ["env_index", "obs", "reset", "rew"]
    assert sum(x.nbytes for x in a.values()) <= limit
    assert all(np.array_equal(a[k], b[k]) for k in a)                 # the same sample every run
    idx = a["env_index"].astype(np.int64)
    assert len(np.unique(idx)) == len(idx) > 0
    np.testing.assert_array_equal(a["obs"], core.obs_buf.numpy()[idx])
    np.testing.assert_array_equal(a["rew"], core.rew_buf.numpy()[idx])
