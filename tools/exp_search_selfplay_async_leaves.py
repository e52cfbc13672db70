"""Developer tool: what several leaves per evaluator call (AsyncSearchSelfPlay(leaves=L) /
mnk_search_selfplay_advance_leaves) cost and buy beside the per-ply budgets.

Workloads: 9x9x5 at 1 024 and at 64 rows and 19x19x5 at 256 rows, I = 256, fast 32, ``full_prob`` 0.25, L in {1, 2, 4, 8,
16}; ``conv`` (the example's net: 4 conv layers of 64 channels and two heads) and ``trivial`` (uniform priors, value 0), the
evaluators of tools/exp_puct.py.  L = 1 goes through the entry point the player took before (mnk_search_selfplay_advance),
whose code object is the parent commit's (profiles/exp_search_selfplay_async_leaves_kernels.md): that row is the baseline,
taken in the same process.

Per row: the time of a round (device events around ``rounds`` rounds, after a warm-up, the mean and the spread of ``reps``
repetitions), plies per second and full-search records per second over those repetitions, the share of the slots of rows
in the middle of a search that were void -- by the cap (beyond the ply's budget: from ``row_sims``) and by the walk (the
rest: slots whose state in the workspace is 0) -- and, in a pass of its own with events around every launch, the summed
duration of the env-side kernel over ``rounds`` rounds.  Nothing here says anything about playing strength.

usage: python tools/exp_search_selfplay_async_leaves.py [--out profiles/exp_search_selfplay_async_leaves.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from exp_search_selfplay_async import SEED, LaunchEvents, full_records, mean, timed  # noqa: E402

I, FAST, FULL_PROB = 256, 32, 0.25
SHAPES = ((9, 9, 5, 1024), (9, 9, 5, 64), (19, 19, 5, 256))
LEAVES = (1, 2, 4, 8, 16)
OLD, NEW = "mnk_search_selfplay_advance", "mnk_search_selfplay_advance_leaves"


def player(shape, kind, L):
    from exp_puct import evaluator

    from selfplay.search_selfplay import AsyncSearchSelfPlay

    m, n, k, envs = shape
    return AsyncSearchSelfPlay(m, n, k, envs, evaluator=evaluator(kind, m * n), iterations=I, fast_iterations=FAST,
                               full_prob=FULL_PROB, temp_plies=8, seed=SEED, leaves=L)


def slot_states(sp):
    """uint32 [N, L]: every slot's state word in the workspace (the layout: csrc/mnk_puct_tree.h)"""
    import torch

    al = lambda x, a: (x + a - 1) // a * a  # noqa: E731
    C, L, J = sp.m * sp.n, sp.leaves, sp.iterations
    nwg = (sp.m * (sp.n + 1) + 31) // 32
    node = al(al(16 + 16 * nwg, 16) + 2 * (J + 2), 16)
    child = al(al(node + 12 * (J + 1), 16) + 4 * (J + 1) * C, 16)
    xhdr = al(child + 2 * (J + 1) * C, 16)
    words = sp.workspace.reshape(sp.num_envs, -1).view(torch.int32)
    cols = [2] + [xhdr // 4 + 2 * (j - 1) + 1 for j in range(1, L)]
    return words[:, cols]


def voids(sp, rounds):
    """over ``rounds`` rounds, of the slots of the rows that went on searching: (slots, void by the cap, void by the walk)"""
    import torch

    tot = torch.zeros(3, dtype=torch.int64, device=sp.row_plies.device)
    for _ in range(rounds):
        before = sp.row_sims.clone()
        sp.advance(1)
        on = sp.fresh == 0
        offered = (sp.row_sims - before)[on].sum()
        void = (slot_states(sp)[on] == 0).sum()
        slots = on.sum() * sp.leaves
        tot += torch.stack([slots, slots - offered, void - (slots - offered)])
    return [int(x) for x in tot.tolist()]


def measure(shape, kind, L, args):
    m, n, k, envs = shape
    sp = player(shape, kind, L)
    sp.advance(args.warmup)
    us, p0, f0 = [], int(sp.row_plies.sum()), full_records(sp)
    for _ in range(args.reps):
        us.append(timed(lambda: sp.advance(args.rounds)) / args.rounds)
    seconds = sum(us) * args.rounds / 1e6
    plies, full = int(sp.row_plies.sum()) - p0, full_records(sp) - f0
    row = {"board": f"{m}x{n}x{k}", "envs": envs, "evaluator": kind, "leaves": L, "iterations": I, "fast_iterations": FAST,
           "full_prob": FULL_PROB, "entry_point": NEW if L > 1 else OLD, "rounds_per_repetition": args.rounds,
           "round_us": {"mean": mean(us), "min": round(min(us), 2), "max": round(max(us), 2)},
           "plies_per_second": round(plies / seconds, 1), "full_records_per_second": round(full / seconds, 1),
           "plies_per_evaluator_call_and_row": round(plies / (args.reps * args.rounds) / envs, 5)}
    if L > 1:
        slots, cap, walk = voids(sp, args.void_rounds)
        row["void_slots"] = {"slots_of_searching_rows": slots, "share_by_cap": round(cap / max(slots, 1), 4),
                             "share_by_walk": round(walk / max(slots, 1), 4)}
    name = NEW if L > 1 else OLD
    with LaunchEvents((name,)) as ev:
        sp.advance(args.rounds)
    row["kernel_us_summed_over_rounds"] = round(sum(ev.us()[name]), 1)
    row["kernel_us_per_launch"] = mean(ev.us()[name])
    row["games"] = sp.pop_game_stats()["games"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=200, help="rounds per repetition")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--void-rounds", type=int, default=100)
    ap.add_argument("--evaluators", default="conv,trivial")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_search_selfplay_async_leaves.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    if not os.environ.get("MNK_HIP_LIB"):
        entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    rows = []
    for shape in SHAPES:
        for kind in args.evaluators.split(","):
            for L in LEAVES:
                rows.append(measure(shape, kind, L, args))
                print(json.dumps(rows[-1]), flush=True)
                with open(args.out, "w") as f:  # (after every row: a run that is cut short keeps what it measured)
                    json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
