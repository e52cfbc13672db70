"""GPU: ``bench.py --dump-outputs`` writes what the last timed launch computed -- the same bits in two runs with the
same arguments, and the same bits as the rollout driven here launch for launch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--envs", "2048", "--chunk", "64", "--steps", "3", "--warmup", "2", "--settle", "1",
        "--seed", "5", "--no-cpu-baseline", "--no-api-path"]


def _bench_dump(path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = out.stdout.strip().splitlines()[-1]
    assert '"steps": 3' in line
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_bench_dump_is_the_last_timed_launch_and_reproducible(tmp_path):
    a, b = _bench_dump(tmp_path / "a"), _bench_dump(tmp_path / "b")
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name
    assert sum(v.nbytes for v in a.values()) <= 64 << 20

    import __graft_entry__ as entry

    entry._ensure_path()
    import mnk_hip
    from env.torch_vector_mnk_env import TorchVectorMnkEnv
    from selfplay.random_rollout import RandomRollout

    mnk_hip.load()
    env = TorchVectorMnkEnv(9, 9, 5, 2048, device="cuda:0")
    env.reset()
    roll = RandomRollout(env, seed=5)
    for _ in range(1 + 2 + 3):  # set-up, warm-up, timed launches
        rec = roll.run(64)
    torch.cuda.synchronize()
    ids = a["records_env_ids"].astype(np.int64)
    assert np.array_equal(ids, np.arange(2048))  # (small enough to be dumped whole)
    planes = rec.planes.cpu().numpy().view(np.uint64)
    hi = a["records_planes_hi"].astype(np.uint64)
    lo = a["records_planes_lo"].astype(np.uint64)
    assert np.array_equal((hi << np.uint64(32)) | lo, planes)
    assert np.array_equal(a["records_meta"].astype(np.uint32), rec.meta.cpu().numpy().view(np.uint32))
    assert np.array_equal(a["rollout_stats"].astype(np.int64), roll.stats.cpu().numpy())
    state = env._planes.cpu().numpy().view(np.uint64)
    assert np.array_equal((a["env_planes_hi"].astype(np.uint64) << np.uint64(32)) | a["env_planes_lo"].astype(np.uint64),
                          state)
    assert np.array_equal(a["env_meta"].astype(np.uint32), env._meta.cpu().numpy().view(np.uint32))
