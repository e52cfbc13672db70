"""GPU: a plain ``bench.py`` run does only what its headline figure needs (set-up, warm-up, the timed steps, the line);
``--full`` adds every other measurement of the line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--envs", "4096", "--chunk", "64", "--steps", "4", "--warmup", "2", "--settle", "2"]
EXTRAS = ("api_path_env_steps_per_s", "api_path_graphed_env_steps_per_s", "api_path_one_launch", "replay_env_steps_per_s",
          "with_action_log", "selfplay")


def _line(argv, env=None):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[:2000]
    return json.loads(lines[0])


def _headline(d):
    assert d["steps"] == 4 and d["warmup"] == 2 and d["setup_launches"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    assert d["value"] == pytest.approx(4096 * 64 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    r = d["roofline"]
    assert r["launches"] == 4 and r["frac"] == pytest.approx(r["achieved"] / r["peak"])


def test_plain_one_gpu_run_measures_the_headline_alone():
    d = _line(SMALL)
    _headline(d)
    assert d["repetitions"] is None and d["cpu_baseline"] is None
    assert not any(key in d for key in EXTRAS)
    assert "measured_write_ceiling_GBps" not in d["roofline"]
    assert d["gpu"]["compute_units"] > 0 and d["gpu"]["rocminfo"] is None


def test_full_one_gpu_run_keeps_every_other_measurement():
    d = _line(SMALL + ["--full", "--cpu-seconds", "1"])
    _headline(d)
    assert len(d["repetitions"]["values"]) == 5 and d["repetitions"]["values"][0] == d["value"]
    assert all(key in d for key in EXTRAS) and "train_cadence_384_envs" in d["selfplay"] and "config3" in d["selfplay"]
    assert d["roofline"]["measured_write_ceiling_GBps"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"
    assert isinstance(d["gpu"]["rocminfo"], (dict, str))


@pytest.mark.parametrize("allgather", ["auto", "direct"])
def test_plain_rehearsed_multi_gpu_run_keeps_what_decides_value(allgather):
    """The multi-GPU code path (one RCCL rank) without --full: no repetitions and no compute-only run; the exchange forms
    alone are timed under --allgather auto, which picks `value` from them, and not when the form is pinned."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(var, None)
    d = _line(["--rehearse-exchange", "--steps", "4", "--warmup", "2", "--settle", "2", "--envs", "4096",
               "--allgather", allgather], env=env)
    ex = d["exchange"]
    assert d["value"] > 0 and ex["allgather_ms"] > 0 and "C ABI, RCCL" in ex["transport"]
    assert d["repetitions"] is None and d["value_without_exchange"] is None
    assert ex["compute_ms_per_chunk"] is None and ex["exposed_ms_per_chunk"] is None and ex["overlap_fraction"] is None
    if allgather == "auto":
        assert ex["alone"]["ncclAllGather_ms"] > 0 and ex["alone"]["direct_sendrecv_ms"] > 0 and "auto" in ex
    else:
        assert "alone" not in ex and "direct" in ex["transport"]
