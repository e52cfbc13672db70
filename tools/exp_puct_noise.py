"""Developer tool: what the PUCT player's built-in root noise (mnk_puct_root_noise) costs per act().

For 9x9x5 x 1 024 rows and 19x19x5 x 256 rows (positions half full at most, one leaf per row; alpha 0.3 and 0.03), device
time with device events, each figure the median over ``--reps`` batches of ``--launches`` back-to-back calls, in us per
call:
  kernel_us      mnk_puct_root_noise on the conv net's float32 priors of those roots
  wrapper_us     the extra work of the example's evaluator wrapper (examples/alphazero_selfplay.py, RootNoise) on the same
                 call: torch.distributions.Dirichlet over [rows, C], the mask, the normalisation and the mix -- the wrapper
                 around an evaluator that returns ready tensors
  evaluator_us   one call of the conv net of tools/exp_puct.py on the roots (what the noise is to be compared with: an
                 act is iterations / leaves + 1 of them)

usage: python tools/exp_puct_noise.py [--reps 9] [--launches 20] [--out profiles/exp_puct_noise.json]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
# (name, m, n, k, rows, alpha)
SETUPS = (("9x9x5 x 1024", 9, 9, 5, 1024, 0.3), ("19x19x5 x 256", 19, 19, 5, 256, 0.03))
EPS = 0.25


def device_us(fn, reps, launches):
    """median over ``reps`` of the device time of ``launches`` back-to-back calls of ``fn``, per call"""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / launches)
    return statistics.median(times), min(times), max(times)


def measure(setup, reps, launches):
    import numpy as np
    import torch

    import mnk_hip
    from exp_puct import evaluator
    from tactical_rule import random_positions

    name, m, n, k, rows, alpha = setup
    C, dev = m * n, torch.device("cuda:0")
    obs_np = random_positions(m, n, k, rows, np.random.default_rng(C), max_fill=0.5)
    obs = torch.from_numpy(obs_np).to(dev)
    mask = (obs.sum(dim=1) == 0).flatten(1).contiguous()
    conv = evaluator("conv", C)
    priors, values = conv(obs, mask)
    priors = priors.float().contiguous()
    out = torch.zeros((rows, C), dtype=torch.float32, device=dev)
    stream = mnk_hip.stream_ptr(dev)
    step = [0]

    def kernel():
        mnk_hip.call("mnk_puct_root_noise", mnk_hip.ptr(priors), mnk_hip.LOGITS_F32, mnk_hip.ptr(mask), rows, C, 1, alpha,
                     EPS, 1, None, step[0], None, 0, mnk_hip.ptr(out), stream)
        step[0] += 1

    spec = importlib.util.spec_from_file_location("alphazero_selfplay", os.path.join(ROOT, "examples", "alphazero_selfplay.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    wrapper = ex.RootNoise(lambda o, msk: (priors, values), 1, alpha=alpha, eps=EPS)  # (period 1: every call is the roots')
    row = {"setup": name, "rows": rows, "cells": C, "alpha": alpha, "eps": EPS,
           "free_cells_mean": round(mask.sum().item() / rows, 1)}
    for key, fn in (("kernel_us", kernel), ("wrapper_us", lambda: wrapper(obs, mask)), ("evaluator_us", lambda: conv(obs, mask))):
        med, lo, hi = device_us(fn, reps, launches)
        row[key], row[key + "_min"], row[key + "_max"] = round(med, 2), round(lo, 2), round(hi, 2)
    row["kernel_share_of_evaluator_call"] = round(row["kernel_us"] / row["evaluator_us"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct_noise.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    rows = []
    for setup in SETUPS:
        row = measure(setup, args.reps, args.launches)
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "launches": args.launches, "rows": rows}, f,
                  indent=1)


if __name__ == "__main__":
    main()
