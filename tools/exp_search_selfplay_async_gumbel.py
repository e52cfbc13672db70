"""Developer tool: what the Gumbel root costs beside the per-ply budgets (AsyncSearchSelfPlay(gumbel=m) /
mnk_search_selfplay_advance_gumbel).

Workload: 9x9x5 at 1 024 rows, I = 64, fast 16, ``full_prob`` 0.25, considered 16; ``trivial`` (uniform priors, value 0) and
``conv`` (the example's net: 4 conv layers of 64 channels and two heads), the evaluators of tools/exp_puct.py.  The row
without the option goes through the entry point the player took before (mnk_search_selfplay_advance), whose code object is
the parent commit's (profiles/exp_search_selfplay_async_gumbel_kernels.md): that row is the baseline, taken in the same
process.

Per row: the time of a round (device events around ``rounds`` rounds, after a warm-up, the mean and the spread of ``reps``
repetitions), plies per evaluator call and row beside the rule's 1 / (p (I + 1) + (1 - p)(F + 1)), and, in a pass of its
own with events around every launch, the duration of the env-side kernel.  Nothing here says anything about playing
strength.

usage: python tools/exp_search_selfplay_async_gumbel.py [--out profiles/exp_search_selfplay_async_gumbel.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from exp_search_selfplay_async import SEED, LaunchEvents, mean, timed  # noqa: E402

I, FAST, FULL_PROB, CONSIDERED = 64, 16, 0.25, 16
SHAPE = (9, 9, 5, 1024)
OLD, NEW = "mnk_search_selfplay_advance", "mnk_search_selfplay_advance_gumbel"


def player(kind, gumbel):
    from exp_puct import evaluator

    from selfplay.search_selfplay import AsyncSearchSelfPlay

    m, n, k, envs = SHAPE
    return AsyncSearchSelfPlay(m, n, k, envs, evaluator=evaluator(kind, m * n), iterations=I, fast_iterations=FAST,
                               full_prob=FULL_PROB, temp_plies=8, seed=SEED, gumbel=gumbel)


def measure(kind, gumbel, args):
    m, n, k, envs = SHAPE
    sp = player(kind, gumbel)
    sp.advance(args.warmup)
    us, p0 = [], int(sp.row_plies.sum())
    for _ in range(args.reps):
        us.append(timed(lambda: sp.advance(args.rounds)) / args.rounds)
    plies = int(sp.row_plies.sum()) - p0
    name = NEW if gumbel else OLD
    row = {"board": f"{m}x{n}x{k}", "envs": envs, "evaluator": kind, "gumbel": gumbel, "iterations": I,
           "fast_iterations": FAST, "full_prob": FULL_PROB, "entry_point": name, "rounds_per_repetition": args.rounds,
           "round_us": {"mean": mean(us), "min": round(min(us), 2), "max": round(max(us), 2)},
           "plies_per_evaluator_call_and_row": round(plies / (args.reps * args.rounds) / envs, 5),
           "plies_per_call_by_the_rule": round(1 / (FULL_PROB * (I + 1) + (1 - FULL_PROB) * (FAST + 1)), 5)}
    with LaunchEvents((name,)) as ev:
        sp.advance(args.rounds)
    row["kernel_us_per_launch"] = mean(ev.us()[name])
    row["games"] = sp.pop_game_stats()["games"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=200, help="rounds per repetition")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--evaluators", default="trivial,conv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_search_selfplay_async_gumbel.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    if not os.environ.get("MNK_HIP_LIB"):
        entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    rows = []
    for kind in args.evaluators.split(","):
        for gumbel in (None, CONSIDERED):
            rows.append(measure(kind, gumbel, args))
            print(json.dumps(rows[-1]), flush=True)
            with open(args.out, "w") as f:  # (after every row: a run that is cut short keeps what it measured)
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
