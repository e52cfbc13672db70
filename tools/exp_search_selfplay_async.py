"""Developer tool: what search self-play with per-row budgets (AsyncSearchSelfPlay / mnk_search_selfplay_advance) costs and
what it buys, beside the lockstep player (SearchSelfPlay.play) in the same process.

Shapes: 9x9x5 x 1 024 rows and 19x19x5 x 256 rows, with the two evaluators of tools/exp_puct.py (``conv``: 4 conv layers of
64 channels and two heads; ``trivial``: uniform priors, value 0).

``lockstep``: with ``full_prob = 1`` and I = 64 the two players do the same work; us per ply of each over ``plies`` plies
after a warm-up (device events around the whole run), and the average of each env-side launch with device events around
every single launch in the busy stream: ``mnk_puct_step`` and ``mnk_search_selfplay_step`` of the lockstep player,
``mnk_search_selfplay_advance`` of the new one, its rounds that end a ply (every (I + 1)-th) apart from the others.

``budgets``: I = 256, fast 32, ``full_prob`` 0.25 against lockstep at I = 256 over the same number of evaluator calls:
plies, finished games and full-search records, per second and per evaluator call.  The full records of the new player
are counted on the host from the budget rule (a function of key, row and ply).  Nothing here says anything about playing
strength: whether training on such data is better per unit of compute is the user's experiment.

usage: python tools/exp_search_selfplay_async.py [--plies 4] [--calls 2056] [--out profiles/exp_search_selfplay_async.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
SHAPES = ((9, 9, 5, 1024), (19, 19, 5, 256))
SEED = 1


def players(shape, kind, I, fast=None, full_prob=1.0):
    from exp_puct import evaluator

    from selfplay.search_selfplay import AsyncSearchSelfPlay, SearchSelfPlay

    m, n, k, envs = shape
    ev = evaluator(kind, m * n)
    lock = SearchSelfPlay(m, n, k, envs, evaluator=ev, iterations=I, temp_plies=8, seed=SEED)
    new = AsyncSearchSelfPlay(m, n, k, envs, evaluator=ev, iterations=I, fast_iterations=fast, full_prob=full_prob,
                              temp_plies=8, seed=SEED)
    return lock, new


def timed(fn):
    import torch

    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


class LaunchEvents:
    """device events around every call of the named entry points while active: {name: [us, ...]} in call order"""

    def __init__(self, names):
        self.names, self.events = set(names), []

    def __enter__(self):
        import torch

        import mnk_hip

        self.lib, self.inner = mnk_hip, mnk_hip.call

        def call(name, *args):
            if name not in self.names:
                return self.inner(name, *args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = self.inner(name, *args)
            e1.record()
            self.events.append((name, e0, e1))
            return rc

        mnk_hip.call = call
        return self

    def __exit__(self, *exc):
        import torch

        self.lib.call = self.inner
        torch.cuda.synchronize()

    def us(self):
        out = {}
        for name, e0, e1 in self.events:
            out.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
        return out


def mean(xs):
    return round(sum(xs) / len(xs), 2) if xs else None


def lockstep_cost(shape, kind, I, plies):
    lock, new = players(shape, kind, I)
    lock.play(1)
    new.advance(I + 1)
    us_lock = timed(lambda: lock.play(plies)) / plies
    us_new = timed(lambda: new.advance(plies * (I + 1))) / plies
    with LaunchEvents(("mnk_puct_step", "mnk_search_selfplay_step", "mnk_puct_begin")) as a:
        lock.play(2)
    with LaunchEvents(("mnk_search_selfplay_advance",)) as b:
        new.advance(2 * (I + 1))
    la, adv = a.us(), b.us()["mnk_search_selfplay_advance"]
    ends = [x for j, x in enumerate(adv) if j % (I + 1) == I]
    rest = [x for j, x in enumerate(adv) if j % (I + 1) != I]
    m, n, k, envs = shape
    return {"board": f"{m}x{n}x{k}", "envs": envs, "iterations": I, "evaluator": kind,
            "lockstep_us_per_ply": round(us_lock, 1), "advance_us_per_ply": round(us_new, 1),
            "us_puct_begin": mean(la.get("mnk_puct_begin")), "us_puct_step": mean(la.get("mnk_puct_step")),
            "us_search_selfplay_step": mean(la.get("mnk_search_selfplay_step")),
            "us_advance_selecting": mean(rest), "us_advance_ending_a_ply": mean(ends),
            "env_side_launches_per_ply": {"lockstep": I + 3, "advance": I + 1}}


def full_records(new):
    """the plies of the run that were searched in full, from the budget rule"""
    import numpy as np

    from oracle import philox

    plies = new.row_plies.cpu().numpy()
    rows = np.arange(len(plies), dtype=np.uint64) + np.uint64(new.sampler.env_id0)
    total = 0
    for p in range(int(plies.max())):
        word = philox.rand_u32(new.sampler.seed, rows, p, 9).astype(np.uint64)
        total += int(((word < np.uint64(new.full_threshold)) & (plies > p)).sum())
    return total


def budgets(shape, kind, I, fast, full_prob, calls):
    lock, new = players(shape, kind, I, fast, full_prob)
    plies = max(1, calls // (I + 1))
    calls = plies * (I + 1)
    lock.play(1)
    new.advance(I + 1)
    lock.pop_game_stats()
    new.pop_game_stats()
    before = int(new.row_plies.sum())
    full_before = full_records(new)
    us_lock = timed(lambda: lock.play(plies))
    us_new = timed(lambda: new.advance(calls))
    g_lock, g_new = lock.pop_game_stats()["games"], new.pop_game_stats()["games"]
    m, n, k, envs = shape
    p_lock, p_new = plies * envs, int(new.row_plies.sum()) - before
    f_new = full_records(new) - full_before

    def rates(us, p, g, f):
        return {"seconds": round(us / 1e6, 3), "plies": p, "games": g, "full_records": f,
                "plies_per_call": round(p / calls / envs, 5), "plies_per_second": round(p / us * 1e6, 1),
                "games_per_second": round(g / us * 1e6, 2), "full_records_per_second": round(f / us * 1e6, 1)}

    return {"board": f"{m}x{n}x{k}", "envs": envs, "iterations": I, "fast_iterations": fast, "full_prob": full_prob,
            "evaluator": kind, "evaluator_calls": calls, "lockstep": rates(us_lock, p_lock, g_lock, p_lock),
            "advance": rates(us_new, p_new, g_new, f_new), "plies_per_call_ratio": round(p_new / p_lock, 3),
            "derived_plies_per_call_ratio": round((I + 1) / (full_prob * (I + 1) + (1 - full_prob) * (fast + 1)), 3),
            "row_plies_min_max": [int(new.row_plies.min()), int(new.row_plies.max())]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=4)
    ap.add_argument("--calls", type=int, default=2056, help="evaluator calls of each side of the budgets comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_search_selfplay_async.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    lock_rows, budget_rows = [], []
    for shape in SHAPES:
        for kind in ("conv", "trivial"):
            row = lockstep_cost(shape, kind, 64, args.plies)
            print(json.dumps(row), flush=True)
            lock_rows.append(row)
    for shape in SHAPES:
        for kind in ("conv", "trivial"):
            row = budgets(shape, kind, 256, 32, 0.25, args.calls)
            print(json.dumps(row), flush=True)
            budget_rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "lockstep": lock_rows, "budgets": budget_rows}, f, indent=1)


if __name__ == "__main__":
    main()
