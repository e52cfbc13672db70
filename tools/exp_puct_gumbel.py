"""Developer tool: what an act() with a Gumbel root (PUCTSearchPolicy(gumbel=m)) costs beside the PUCT act it replaces.

On the conv set-up of tools/exp_puct_leaves.py -- 9x9x5 x 1 024 rows of random mid-game positions, the conv net -- ``act``
of Gumbel(I = 16, m = 8), Gumbel(I = 32, m = 8), PUCT(I = 16) and PUCT(I = 256) in ONE process: every policy is built and
warmed up first, then ``--reps`` passes over the policies in turn, each act timed with device events of its own; the
median is reported.  ``prep_us``: mnk_puct_gumbel_root alone on the conv net's priors and values of those roots, the median
of ``--reps`` launches timed the same way.

usage: python tools/exp_puct_gumbel.py [--reps 5] [--out profiles/exp_puct_gumbel.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
SETUP = ("conv 9x9x5 x 1024", 9, 9, 5, 1024, "conv")
#       name            I    gumbel
KEYS = (("gumbel 16", 16, 8), ("gumbel 32", 32, 8), ("puct 16", 16, None), ("puct 256", 256, None))


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct_gumbel.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    entry.build_hip()
    import numpy as np
    import torch

    import mnk_hip
    from exp_puct import evaluator
    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions

    torch.backends.cudnn.benchmark = False
    name, m, n, k, rows, kind = SETUP
    C = m * n
    obs_np = random_positions(m, n, k, rows, np.random.default_rng(C + 256), max_fill=0.5)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
    ev = evaluator(kind, C)
    pols = {key: PUCTSearchPolicy(k, evaluator=ev, iterations=I, seed=1, gumbel=g) for key, I, g in KEYS}
    for pol in pols.values():  # warm-up: the buffers, the table
        for _ in range(2):
            pol.act(obs)
    torch.cuda.synchronize()
    times = {key: [] for key in pols}
    for _ in range(args.reps):
        for key, pol in pols.items():
            times[key].append(timed(lambda: pol.act(obs)))
    out = []
    for key, I, g in KEYS:
        t = times[key]
        out.append({"setup": name, "player": key, "iterations": I, "considered": g, "evaluator_calls": I + 1,
                    "us_per_act": round(statistics.median(t), 1), "us_per_act_min": round(min(t), 1),
                    "us_per_act_max": round(max(t), 1)})
        print(json.dumps(out[-1]), flush=True)

    # the prep kernel alone, on the conv net's answer for these roots
    mask = (obs["observation"].sum(dim=1) == 0).flatten(1).contiguous()
    priors, values = ev(obs["observation"], mask)
    priors, values = priors.float().contiguous(), values.float().reshape(-1).contiguous()
    gscore = torch.empty((rows, C), device="cuda:0")
    vroot = torch.empty(rows, device="cuda:0")
    stream = mnk_hip.stream_ptr(torch.device("cuda:0"))

    def prep():
        mnk_hip.call("mnk_puct_gumbel_root", mnk_hip.ptr(priors), mnk_hip.LOGITS_F32, mnk_hip.ptr(mask), mnk_hip.ptr(values),
                     mnk_hip.LOGITS_F32, rows, C, 1.0, 1, None, 0, None, 0, mnk_hip.ptr(gscore), mnk_hip.ptr(vroot), stream)

    for _ in range(3):
        prep()
    torch.cuda.synchronize()
    t = [timed(prep) for _ in range(max(args.reps, 5))]
    prep_row = {"setup": name, "kernel": "mnk_puct_gumbel_root", "prep_us": round(statistics.median(t), 1),
                "prep_us_min": round(min(t), 1), "prep_us_max": round(max(t), 1)}
    print(json.dumps(prep_row), flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": out, "prep": prep_row}, f, indent=1)


if __name__ == "__main__":
    main()
