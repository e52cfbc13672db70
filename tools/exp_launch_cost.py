"""Fixed cost per launch of the rollout kernel: the headline case at T = 64, 256 and 1024 plies per launch, least-squares
fit of a + b*T over every repetition (developer tool, GPU box).
usage: python tools/exp_launch_cost.py [MxNxK] [envs]      (MNK_HIP_LIB selects the build)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd")]
import numpy as np
import torch
from env.torch_vector_mnk_env import TorchVectorMnkEnv
from selfplay.random_rollout import RandomRollout

board = tuple(int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "9x9x5").split("x"))
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
TS, REPS = (64, 256, 1024), 5
env = TorchVectorMnkEnv(*board, N, device="cuda:0"); roll = RandomRollout(env, seed=0)
bufs = {T: roll.alloc(T) for T in TS}
for T in TS:
    for _ in range(300 * 64 // T + 8): roll.run(T, out=bufs[T])
xs, ys = [], []
for rep in range(REPS):
    for T in TS:
        launches = max(16, 64 * 256 // T)
        for _ in range(8): roll.run(T, out=bufs[T])
        torch.cuda.synchronize(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches): roll.run(T, out=bufs[T])
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / launches
        xs.append(T); ys.append(us)
        print(board, N, f"rep {rep} T = {T}: {us:.2f} us per launch", flush=True)
b, a = np.polyfit(np.array(xs, float), np.array(ys), 1)
print(board, N, f"fit over {len(xs)} points: a = {a:.2f} us per launch, b = {b * 1e3:.2f} ns per ply ({b * 256:.2f} us per 256 plies)")
