"""Developer tool: what the options of per-row search self-play (AsyncSearchSelfPlay(root_noise=..., solver=...) /
mnk_search_selfplay_advance_opts) cost and buy, and that the plain player does not pay for them.

Shapes and evaluators are those of tools/exp_search_selfplay_async.py: 9x9x5 x 1 024 rows and 19x19x5 x 256 rows, I = 256,
fast 32, ``full_prob`` 0.25; ``conv`` (4 conv layers of 64 channels and two heads) and ``trivial`` (uniform priors, value 0).
Times are device events, after a warm-up, over at least 5 repetitions.

``plain``: us per ``mnk_search_selfplay_advance`` launch (device events around every launch in the busy stream, trivial
evaluator) of this build against another build of the library -- ``--parent-lib``, the parent commit's -- in fresh
processes that alternate, every process repeating the same rounds of the same games.  The bar is the parent's own
run-to-run spread (min .. max over its repetitions).  Without ``--parent-lib`` only this build is measured.

``options``: the new entry point with the options off against the old one (the same rounds of the same games); the average
launch with noise on at the mixed budgets; with every ply full and I = 64 the launches that noise every root (every
(I + 1)-th) apart from those that select and those that end a ply; the round with the ``conv`` evaluator without noise, with
the built-in noise and with the evaluator wrapper of examples/alphazero_selfplay.py (``FreshRootNoise``).

``solver``: plies per evaluator call and the share of plies that ended by proof (a ply that took fewer launches than its
budget + 1, from the ply counts after every launch and the budget rule), with the solver and without, over the same number
of evaluator calls; from the empty board and from late positions (every row after ``late`` plies of the oracle's uniformly
random play).  Nothing here says anything about playing strength.

usage: python tools/exp_search_selfplay_async_opts.py [--parent-lib PATH] [--out profiles/exp_search_selfplay_async_opts.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"),
                os.path.join(ROOT, "examples")]
from exp_search_selfplay_async import SEED, SHAPES, LaunchEvents, mean, timed  # noqa: E402

I, FAST, FULL_PROB = 256, 32, 0.25
LATE = {"9x9x5": 40, "19x19x5": 150}  # plies of random play before a late start
OLD, NEW = "mnk_search_selfplay_advance", "mnk_search_selfplay_advance_opts"
NOISE = {"9x9x5": (0.3, 0.25), "19x19x5": (0.03, 0.25)}


def name_of(shape):
    return "x".join(map(str, shape[:3]))


def player(shape, kind, iterations=I, fast=FAST, full_prob=FULL_PROB, wrapper=False, **options):
    from exp_puct import evaluator

    from selfplay.search_selfplay import AsyncSearchSelfPlay

    m, n, k, envs = shape
    ev = evaluator(kind, m * n)
    if wrapper:
        from alphazero_selfplay import FreshRootNoise

        ev = FreshRootNoise(ev, *NOISE[name_of(shape)])
    sp = AsyncSearchSelfPlay(m, n, k, envs, evaluator=ev, iterations=iterations, fast_iterations=fast, full_prob=full_prob,
                             temp_plies=8, seed=SEED, **options)
    if wrapper:
        ev.fresh = lambda: sp.fresh
    return sp


def launch_us(sp, name, warmup, rounds, reps):
    """[reps] averages of the us of every ``name`` launch over ``rounds`` rounds each, after ``warmup`` rounds"""
    sp.advance(warmup)
    out = []
    for _ in range(reps):
        with LaunchEvents((name,)) as ev:
            sp.advance(rounds)
        out.append(mean(ev.us()[name]))
    return out


class ViaTheNewEntryPoint:
    """while active, every call of the old entry point goes to the new one with the options off"""

    def __enter__(self):
        import mnk_hip

        self.lib, self.inner = mnk_hip, mnk_hip.call
        mnk_hip.call = lambda name, *a: (self.inner(NEW, *a[:-1], 0, 0.0, 0.0, 0, None, a[-1]) if name == OLD
                                         else self.inner(name, *a))
        return self

    def __exit__(self, *exc):
        self.lib.call = self.inner


def spread(xs):
    return {"mean": mean(xs), "min": round(min(xs), 2), "max": round(max(xs), 2), "repetitions": [round(x, 2) for x in xs]}


# ----------------------------------------------------------------------------- plain: this build against the parent's
def worker_plain(args):
    """(a fresh process per build: the library is loaded once) one JSON line {board: [us per launch, ...]}"""
    out = {name_of(shape): launch_us(player(shape, "trivial"), OLD, args.warmup, args.rounds, args.reps) for shape in SHAPES}
    print("RESULT " + json.dumps(out), flush=True)


def plain(args):
    builds = {"this": None}
    if args.parent_lib:
        builds["parent"] = os.path.abspath(args.parent_lib)
    runs = {b: {name_of(s): [] for s in SHAPES} for b in builds}
    for _ in range(args.processes):
        for build, path in reversed(list(builds.items())):  # parent, this, parent, this, ...
            env = dict(os.environ)
            if path:
                env["MNK_HIP_LIB"] = path
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(args.warmup),
                                   "--rounds", str(args.rounds), "--reps", str(args.reps)], env=env, check=True,
                                  capture_output=True, text=True, timeout=600)
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            for board, us in json.loads(line[7:]).items():
                runs[build][board] += us
    rows = []
    for shape in SHAPES:
        board = name_of(shape)
        row = {"board": board, "envs": shape[3], "iterations": I, "fast_iterations": FAST, "full_prob": FULL_PROB,
               "entry_point": OLD, "launches_per_repetition": args.rounds,
               "this_us_per_launch": spread(runs["this"][board])}
        if "parent" in runs:
            par = row["parent_us_per_launch"] = spread(runs["parent"][board])
            row["parent_spread_us"] = round(par["max"] - par["min"], 2)
            row["this_mean_inside_parent_spread"] = par["min"] <= row["this_us_per_launch"]["mean"] <= par["max"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


# ----------------------------------------------------------------------------- options: what they cost
def options(args):
    rows = []
    for shape in SHAPES:
        board, noise = name_of(shape), NOISE[name_of(shape)]
        row = {"board": board, "envs": shape[3], "noise": list(noise)}
        row["old_entry_us"] = spread(launch_us(player(shape, "trivial"), OLD, args.warmup, args.rounds, args.reps))
        with ViaTheNewEntryPoint():  # (the events go around the player's call, which is then the new entry point's)
            row["new_entry_options_off_us"] = spread(launch_us(player(shape, "trivial"), OLD, args.warmup, args.rounds,
                                                               args.reps))
        row["noise_on_us"] = spread(launch_us(player(shape, "trivial", root_noise=noise), NEW, args.warmup, args.rounds,
                                              args.reps))
        row["solver_on_us"] = spread(launch_us(player(shape, "trivial", solver=True), NEW, args.warmup, args.rounds,
                                               args.reps))
        # every ply full, rows in step: launch j backs up a root's evaluation iff j % (J + 1) == 0, ends a ply iff == J
        J = 64
        sp = player(shape, "trivial", iterations=J, fast=None, full_prob=1.0, root_noise=noise)
        sp.advance(J + 1)
        with LaunchEvents((NEW,)) as ev:
            sp.advance(args.reps * (J + 1))
        us = ev.us()[NEW]
        row["in_step_I64_us"] = {"noising_every_root": mean(us[0::J + 1]), "ending_a_ply": mean(us[J::J + 1]),
                                 "selecting": mean([x for j, x in enumerate(us) if j % (J + 1) not in (0, J)])}
        rounds = {}
        for label, kw in (("no_noise", {}), ("builtin_noise", {"root_noise": noise}), ("wrapper_noise", {"wrapper": True})):
            sp = player(shape, "conv", **kw)
            sp.advance(args.warmup)
            rounds[label] = spread([timed(lambda: sp.advance(args.rounds)) / args.rounds for _ in range(args.reps)])
        row["conv_round_us"] = rounds
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


# ----------------------------------------------------------------------------- solver: what it buys
def late_start(sp, shape, plies):
    """every row after ``plies`` plies of the oracle's uniformly random play (games that ended on the way began again)"""
    import torch

    from oracle.env_torch import OracleVectorEnv
    from oracle.packing import pack_boards

    m, n, k, envs = shape
    env = OracleVectorEnv(m, n, k, envs)
    from oracle.rollout import random_rollout

    random_rollout(env, SEED, 0, plies)
    planes = pack_boards(env.boards.numpy() != 0, m, n)
    meta = (env.move_counts.numpy() << 1) | env.current_player.numpy()
    s = sp.state_dict()
    s["env"]["planes"] = torch.from_numpy(planes.view("int64"))
    s["env"]["meta"] = torch.from_numpy(meta.astype("int64")).to(s["env"]["meta"].dtype)
    sp.load_state_dict(s)


def ended_by_proof(sp, history, first):
    """of the plies played during ``history`` (int64 [R, N]: every row's ply count after each launch; ``first``: before
    the first), those that took fewer launches than their budget + 1"""
    import numpy as np

    from oracle import philox

    hist = np.concatenate([first[None], history])
    rows = np.arange(hist.shape[1], dtype=np.uint64) + np.uint64(sp.sampler.env_id0)
    early = total = 0
    for i in range(hist.shape[1]):
        ends = np.flatnonzero(np.diff(hist[:, i]))  # the launches in which row i played
        if len(ends) < 2:
            continue
        took = np.diff(ends)  # launches of the plies hist[ends[1:], i] .. : from the launch after the last ply to its own
        plies = hist[ends[1:], i].astype(np.uint64)
        word = np.array([philox.rand_u32(sp.sampler.seed, rows[i:i + 1], int(p), 9)[0] for p in plies], np.uint64)
        budget = np.where(word < np.uint64(sp.full_threshold), sp.iterations, sp.fast_iterations)
        early += int((took < budget + 1).sum())
        total += len(took)
    return early, total


def solver(args):
    import torch

    rows = []
    for shape in SHAPES:
        for start in ("empty", "late"):
            row = {"board": name_of(shape), "envs": shape[3], "start": start, "evaluator": "trivial",
                   "evaluator_calls": args.calls}
            if start == "late":
                row["late_plies_of_random_play"] = LATE[name_of(shape)]
            for label, on in (("solver_off", False), ("solver_on", True)):
                sp = player(shape, "trivial", solver=on)
                if start == "late":
                    late_start(sp, shape, LATE[name_of(shape)])
                first = sp.row_plies.cpu().numpy()
                history = torch.zeros((args.calls, shape[3]), dtype=torch.int64, device=sp.row_plies.device)
                for r in range(args.calls):
                    sp.advance(1)
                    history[r].copy_(sp.row_plies)
                early, total = ended_by_proof(sp, history.cpu().numpy(), first)
                plies = int(sp.row_plies.sum()) - int(first.sum())
                row[label] = {"plies": plies, "plies_per_call": round(plies / args.calls / shape[3], 5),
                              "games": sp.pop_game_stats()["games"], "plies_ended_by_proof": early, "of_plies": total,
                              "share_ended_by_proof": round(early / max(total, 1), 4)}
            row["plies_per_call_ratio"] = round(row["solver_on"]["plies"] / max(row["solver_off"]["plies"], 1), 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmnk_hip.so, for the plain comparison")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per build in the plain comparison")
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=400, help="launches per repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1028, help="evaluator calls of each side of the solver comparison")
    ap.add_argument("--only", choices=("plain", "options", "solver"), default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_search_selfplay_async_opts.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    if not os.environ.get("MNK_HIP_LIB"):
        entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    if args.worker:
        return worker_plain(args)
    out = {}
    if os.path.exists(args.out):  # (--only: the other parts stay as they were measured)
        with open(args.out) as f:
            out.update(json.load(f))
    # (plain first: its fresh processes start before this one has touched the GPU)
    for part, fn in (("plain", plain), ("options", options), ("solver", solver)):
        if args.only in (None, part):
            out[part] = fn(args)
            if part != "plain":
                out["device"] = torch.cuda.get_device_name(0)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
