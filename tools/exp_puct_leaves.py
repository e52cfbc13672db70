"""Developer tool: what several leaves per row and evaluator call (PUCTSearchPolicy(leaves=L)) buy per act().

For every set-up -- the two of tools/exp_puct.py (the conv net on 9x9x5 x 1 024 rows and on 19x19x5 x 256 rows), the
trivial evaluator on 9x9x5 x 1 024, and the conv net on 9x9x5 x 64 rows, where the evaluator is most likely bound by
latency -- ``act`` at I = 256 with L = 1, 2, 4, 8, 16 in ONE process: every policy is built and warmed up first (every
batch shape the evaluator will see), then ``--reps`` passes over the five L in turn, each act timed with device events of
its own; the median per L is reported.  L = 1 runs the entry points without ``leaves`` (what the player ran before).
  us_per_act, us_per_evaluator_call = us_per_act / (I / L + 1), void_share = the share of the I simulations a row did not
  get because a slot was void (from the root visits; rows without a legal cell left out).

``--profile``: one eager act per set-up and L, in that order, for ``rocprofv3 --kernel-trace --output-format csv`` (a run
of its own).  ``--trace DIR`` then reads the per-dispatch trace, cuts it at every k_puct_begin* dispatch and writes the
summed duration of the k_puct_* kernels of each act (``env_us_per_act``) into the JSON next to the timings.

usage: python tools/exp_puct_leaves.py [--reps 5] [--out profiles/exp_puct_leaves.json] [--profile | --trace DIR]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
# (name, m, n, k, rows, evaluator)
SETUPS = (("conv 9x9x5 x 1024", 9, 9, 5, 1024, "conv"), ("conv 19x19x5 x 256", 19, 19, 5, 256, "conv"),
          ("trivial 9x9x5 x 1024", 9, 9, 5, 1024, "trivial"), ("conv 9x9x5 x 64", 9, 9, 5, 64, "conv"))
LEAVES, I = (1, 2, 4, 8, 16), 256


def build(setup):
    """(obs, {L: policy}, visits) of one set-up; the five policies share one evaluator"""
    import numpy as np
    import torch

    from exp_puct import evaluator
    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions

    _, m, n, k, rows, kind = setup
    obs_np = random_positions(m, n, k, rows, np.random.default_rng(m * n + I), max_fill=0.5)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
    ev = evaluator(kind, m * n)
    pols = {L: PUCTSearchPolicy(k, evaluator=ev, iterations=I, seed=1, leaves=L) for L in LEAVES}
    return obs, pols, torch.zeros((rows, m * n), dtype=torch.int32, device="cuda:0")


def timing(setup, reps):
    import torch

    obs, pols, visits = build(setup)
    live = (obs["observation"].sum(dim=1) == 0).flatten(1).any(dim=1)
    void = {}
    for L, pol in pols.items():  # warm-up: every batch shape, the buffers
        for _ in range(2):
            pol.act(obs, visits=visits)
        void[L] = 1.0 - visits[live].sum().item() / (I * int(live.sum()))
    torch.cuda.synchronize()
    times = {L: [] for L in LEAVES}
    for _ in range(reps):
        for L, pol in pols.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pol.act(obs)
            e1.record()
            e1.synchronize()
            times[L].append(e0.elapsed_time(e1) * 1e3)
    out = []
    for L in LEAVES:
        us = statistics.median(times[L])
        out.append({"setup": setup[0], "iterations": I, "leaves": L, "us_per_act": round(us, 1),
                    "us_per_act_min": round(min(times[L]), 1), "us_per_act_max": round(max(times[L]), 1),
                    "us_per_evaluator_call": round(us / (I // L + 1), 2), "void_share": round(void[L], 4)})
    return out


def env_side(trace_dir):
    """{(setup, L): summed us of the k_puct_* dispatches of that act} from the --profile pass's kernel trace"""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(files[-1])) if "k_puct_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    acts = []
    for r in rows:
        if "k_puct_begin" in r["Kernel_Name"]:
            acts.append(0)
        acts[-1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    keys = [(s[0], L) for s in SETUPS for L in LEAVES]
    assert len(acts) == len(keys), (len(acts), len(keys))
    return {key: ns / 1e3 for key, ns in zip(keys, acts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct_leaves.json"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--trace")
    args = ap.parse_args()
    if args.trace:
        env = env_side(args.trace)
        with open(args.out) as f:
            data = json.load(f)
        for row in data["rows"]:
            row["env_us_per_act"] = round(env[(row["setup"], row["leaves"])], 1)
            print(json.dumps(row))
        with open(args.out, "w") as f:
            json.dump(data, f, indent=1)
        return
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    if args.profile:  # one eager act per set-up and L; the profiler does the timing
        for setup in SETUPS:
            obs, pols, _ = build(setup)
            for L in LEAVES:
                pols[L].act(obs)
        torch.cuda.synchronize()
        print("profile pass done")
        return
    rows = []
    for setup in SETUPS:
        for row in timing(setup, args.reps):
            print(json.dumps(row), flush=True)
            rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
