"""Rollout kernel with and without the statistics fold: the headline launch with `stats` given and null, back to back
(developer tool, GPU box).  usage: python tools/exp_stats_cost.py [MxNxK] [envs]      (MNK_HIP_LIB selects the build)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd")]
import torch
import mnk_hip
from env.torch_vector_mnk_env import TorchVectorMnkEnv
from selfplay.random_rollout import RandomRollout

board = tuple(int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "9x9x5").split("x"))
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
env = TorchVectorMnkEnv(*board, N, device="cuda:0"); roll = RandomRollout(env, seed=0); buf = roll.alloc(256)
def launch(stats):
    mnk_hip.call("mnk_rollout_random", mnk_hip.ptr(env._planes), mnk_hip.ptr(env._meta), N, *board, 256, 0, roll.step, 0,
                 mnk_hip.ptr(buf.planes), mnk_hip.ptr(buf.meta), mnk_hip.ptr(stats), None, 0, env._stream())
    roll.step += 256
for _ in range(300): launch(roll._stats)
for rep in range(5):
    for name, stats in (("stats", roll._stats), ("null", None)):
        for _ in range(30): launch(stats)
        torch.cuda.synchronize(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(64): launch(stats)
        e1.record(); torch.cuda.synchronize()
        print(board, N, f"rep {rep}", name, round(e0.elapsed_time(e1) * 1e3 / 64, 2), "us per 256 plies", flush=True)
