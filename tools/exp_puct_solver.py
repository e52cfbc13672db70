"""Developer tool: what the proofs of wins, draws and losses (PUCTSearchPolicy(solver=True)) cost and find per act().

On two set-ups of tools/exp_puct_leaves.py -- 9x9x5 x 1 024 rows of random mid-game positions, the conv net and the
trivial evaluator -- ``act`` at I = 256 with L = 1 and 4, the solver off and on, in ONE process: every policy is built and
warmed up first, then ``--reps`` passes over the eight policies in turn, each act timed with device events of its own; the
median is reported.  Solver off is the player as it was (L = 1: the entry points without ``leaves``).
  us_per_act, proven_share = the share of the rows with a legal cell whose root is proven when the act ends (solver on),
  visits_share = the adjusted root visits handed out over the I simulations asked for.

``--profile``: one eager act per set-up, L and solver setting, in that order, for ``rocprofv3 --kernel-trace
--output-format csv`` (a run of its own, no counters).  ``--trace DIR`` then reads the per-dispatch trace, cuts it at every
k_puct_begin* dispatch and writes the summed duration of the k_puct_* kernels of each act (``env_us_per_act``) into the JSON
next to the timings.

usage: python tools/exp_puct_solver.py [--reps 5] [--out profiles/exp_puct_solver.json] [--profile | --trace DIR]"""
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
SETUPS = (("conv 9x9x5 x 1024", 9, 9, 5, 1024, "conv"), ("trivial 9x9x5 x 1024", 9, 9, 5, 1024, "trivial"))
LEAVES, I = (1, 4), 256
KEYS = [(L, solver) for L in LEAVES for solver in (False, True)]


def build(setup):
    """(obs, {(L, solver): policy}) of one set-up; the policies share one evaluator"""
    import numpy as np
    import torch

    from exp_puct import evaluator
    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions

    _, m, n, k, rows, kind = setup
    obs_np = random_positions(m, n, k, rows, np.random.default_rng(m * n + I), max_fill=0.5)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
    ev = evaluator(kind, m * n)
    return obs, {(L, s): PUCTSearchPolicy(k, evaluator=ev, iterations=I, seed=1, leaves=L, solver=s) for L, s in KEYS}


def timing(setup, reps):
    import torch

    import mnk_hip

    obs, pols = build(setup)
    rows, C = obs["observation"].shape[0], obs["observation"].shape[2] * obs["observation"].shape[3]
    visits = torch.zeros((rows, C), dtype=torch.int32, device="cuda:0")
    proof = torch.zeros(rows, dtype=torch.int8, device="cuda:0")
    live = (obs["observation"].sum(dim=1) == 0).flatten(1).any(dim=1)
    proven, handed = {}, {}
    for key, pol in pols.items():  # warm-up: every batch shape, the buffers
        for _ in range(2):
            pol.act(obs, visits=visits, **({"proof": proof} if key[1] else {}))
        proven[key] = (proof[live] != mnk_hip.PROOF_UNKNOWN).float().mean().item() if key[1] else 0.0
        handed[key] = visits[live].sum().item() / (I * int(live.sum()))
    torch.cuda.synchronize()
    times = {key: [] for key in KEYS}
    for _ in range(reps):
        for key, pol in pols.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pol.act(obs)
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e3)
    out = []
    for L, solver in KEYS:
        t = times[(L, solver)]
        out.append({"setup": setup[0], "iterations": I, "leaves": L, "solver": solver,
                    "us_per_act": round(statistics.median(t), 1), "us_per_act_min": round(min(t), 1),
                    "us_per_act_max": round(max(t), 1), "proven_share": round(proven[(L, solver)], 4),
                    "visits_share": round(handed[(L, solver)], 4)})
    return out


def env_side(trace_dir):
    """{(setup, L, solver): summed us of the k_puct_* dispatches of that act} from the --profile pass's kernel trace"""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(files[-1])) if "k_puct_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    acts = []
    for r in rows:
        if "k_puct_begin" in r["Kernel_Name"]:
            acts.append(0)
        acts[-1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    keys = [(s[0],) + key for s in SETUPS for key in KEYS]
    assert len(acts) == len(keys), (len(acts), len(keys))
    return {key: ns / 1e3 for key, ns in zip(keys, acts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct_solver.json"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--trace")
    args = ap.parse_args()
    if args.trace:
        env = env_side(args.trace)
        with open(args.out) as f:
            data = json.load(f)
        for row in data["rows"]:
            row["env_us_per_act"] = round(env[(row["setup"], row["leaves"], row["solver"])], 1)
            print(json.dumps(row))
        with open(args.out, "w") as f:
            json.dump(data, f, indent=1)
        return
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    if args.profile:  # one eager act per set-up, L and solver setting; the profiler does the timing
        for setup in SETUPS:
            obs, pols = build(setup)
            for key in KEYS:
                pols[key].act(obs)
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
