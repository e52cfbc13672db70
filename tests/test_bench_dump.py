"""CPU: ``bench.py --dump-outputs`` -- exact float64 encoding of the packed words, a fixed seeded sample of envs when
the records exceed the 64 MB budget, and the flag's restriction to the flagship workload."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake(nenv, steps=256, rows=3, words=2, seed=0):
    g = torch.Generator().manual_seed(seed)

    def words64(*shape):
        return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, generator=g)

    rec = SimpleNamespace(planes=words64(steps, rows, nenv),
                          meta=torch.randint(-2 ** 31, 2 ** 31 - 1, (steps, nenv), dtype=torch.int32, generator=g))
    env = SimpleNamespace(_planes=words64(2, words, nenv),
                          _meta=torch.randint(-2 ** 31, 2 ** 31 - 1, (nenv,), dtype=torch.int32, generator=g))
    roll = SimpleNamespace(env=env, stats=torch.tensor([7, 3, 2, 2, 91], dtype=torch.int64))
    return rec, roll


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def _u64(d, name):
    return (d[name + "_hi"].astype(np.uint64) << np.uint64(32)) | d[name + "_lo"].astype(np.uint64)


def test_dump_of_a_large_batch_is_a_fixed_sample_within_budget(tmp_path):
    import bench

    rec, roll = _fake(8192)  # 8192 envs x 256 plies: 117 MB of records as float64
    bench.dump_outputs(str(tmp_path / "a"), rec, roll)
    bench.dump_outputs(str(tmp_path / "b"), rec, roll)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    for name in a:
        assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
    ids = a["records_env_ids"].astype(np.int64)
    assert 0 < len(ids) < 8192 and np.all(np.diff(ids) > 0)
    assert np.array_equal(_u64(a, "records_planes"), rec.planes.numpy().view(np.uint64)[:, :, ids])
    assert np.array_equal(a["records_meta"].astype(np.uint32), rec.meta.numpy().view(np.uint32)[:, ids])
    assert np.array_equal(_u64(a, "env_planes"), roll.env._planes.numpy().view(np.uint64))
    assert np.array_equal(a["env_meta"].astype(np.uint32), roll.env._meta.numpy().view(np.uint32))
    assert a["rollout_stats"].tolist() == [7, 3, 2, 2, 91]


def test_dump_of_a_small_batch_is_whole(tmp_path):
    import bench

    rec, roll = _fake(300, steps=16)
    bench.dump_outputs(str(tmp_path), rec, roll)
    d = _load(tmp_path)
    assert np.array_equal(d["records_env_ids"], np.arange(300))
    assert np.array_equal(_u64(d, "records_planes"), rec.planes.numpy().view(np.uint64))


def test_dump_outputs_is_for_the_rollout_mode():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "selfplay", "--dump-outputs", "x"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--dump-outputs" in out.stderr
