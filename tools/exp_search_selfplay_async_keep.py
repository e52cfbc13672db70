"""Developer tool: what keeping the played move's subtree costs per-row search self-play
(AsyncSearchSelfPlay(keep_tree=True) / mnk_search_selfplay_advance_keep) and what it carries, and that the existing
players do not pay for it.

Shapes and evaluators are those of tools/exp_search_selfplay_async.py: 9x9x5 x 1 024 rows and 19x19x5 x 256 rows, I = 256,
fast 32, ``full_prob`` 0.25, ``tree_nodes`` 513; ``conv`` and ``trivial``.  Times are device events around every launch in
the busy stream, after a warm-up, over at least 5 repetitions.

``plain``: us per ``mnk_search_selfplay_advance`` launch of this build against the parent commit's library
(``--parent-lib``) in fresh processes that alternate (tools/exp_search_selfplay_async_opts.py's ``plain``); the bar is the
parent's own run-to-run spread.

``launch``: us per launch of ``mnk_search_selfplay_advance_keep`` (options off) against
``mnk_search_selfplay_advance_opts`` with the options off, the trivial evaluator, the same seed.

``carry``: the launches of the keeping player split into those in which no row, some row and every row ended a ply (from
the ply counts after every launch): how many, us each; with every ply full and I = 64 the rows stay in step and every
(I + 1)-th launch ends every row's ply.  The round with the ``conv`` evaluator with and without ``keep_tree``, and the
carry's share of it: (share of launches with a ply end) x (their us - a selecting launch's us) / the round.

``peaked``: the carry at a size that matters -- an evaluator whose priors halve from cell to cell, under which a row
carries tens to hundreds of nodes: the launches split as in ``carry`` and by the most nodes a row carried in them, in fresh
processes; with ``--carry-lib B=PATH`` (a build with ``-DMNK_KEEP_CARRY_B=B``) the same games with another number of nodes
in flight in the carry's copy loop, alternating.

``carried``: per ply that ended, the nodes kept and the root visits carried into the next ply, separately for next plies
that are full and fast (the budget rule), and the share of plies that started fresh.  Nothing here says anything about
playing strength: whether fast plies on carried trees train better is the user's experiment.

usage: python tools/exp_search_selfplay_async_keep.py [--parent-lib PATH] [--out profiles/exp_search_selfplay_async_keep.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"),
                os.path.join(ROOT, "examples")]
import exp_search_selfplay_async_opts as opts  # noqa: E402
from exp_search_selfplay_async import SHAPES, LaunchEvents, mean, timed  # noqa: E402
from exp_search_selfplay_async_opts import launch_us, name_of, player, spread  # noqa: E402

I, FAST, FULL_PROB, TREE_NODES = 256, 32, 0.25, 513
OPTS, KEEP = "mnk_search_selfplay_advance_opts", "mnk_search_selfplay_advance_keep"


def keeper(shape, kind, **kw):
    kw.setdefault("tree_nodes", TREE_NODES)
    return player(shape, kind, keep_tree=True, **kw)


def launch(args):
    rows = []
    for shape in SHAPES:
        row = {"board": name_of(shape), "envs": shape[3], "iterations": I, "fast_iterations": FAST, "full_prob": FULL_PROB,
               "tree_nodes": TREE_NODES}
        with opts.ViaTheNewEntryPoint():  # (the plain player's call, sent to the opts entry point with the options off)
            row["opts_entry_options_off_us"] = spread(launch_us(player(shape, "trivial"), opts.OLD, args.warmup, args.rounds,
                                                                args.reps))
        row["keep_entry_us"] = spread(launch_us(keeper(shape, "trivial"), KEEP, args.warmup, args.rounds, args.reps))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def split_by_ply_ends(sp, name, rounds):
    """``rounds`` launches: (us of every launch, rows that ended a ply in it, [rounds, N, 2] carried after it, [rounds, N]
    ply counts after it)"""
    import torch

    N = sp.num_envs
    plies = torch.zeros((rounds + 1, N), dtype=torch.int64, device=sp.row_plies.device)
    carried = torch.zeros((rounds, N, 2), dtype=torch.int32, device=sp.row_plies.device)
    plies[0].copy_(sp.row_plies)
    with LaunchEvents((name,)) as ev:
        for r in range(rounds):
            sp.advance(1)
            plies[r + 1].copy_(sp.row_plies)
            carried[r].copy_(sp.carried)
    us = ev.us()[name]
    ended = (plies[1:] != plies[:-1]).sum(dim=1).cpu().tolist()
    return us, ended, carried.cpu().numpy(), plies.cpu().numpy()


def classes(us, ended, N):
    out = {}
    for label, pick in (("no_row", lambda e: e == 0), ("some_row", lambda e: 0 < e < N), ("every_row", lambda e: e == N)):
        xs = sorted(u for u, e in zip(us, ended) if pick(e))
        out[label] = {"launches": len(xs), "mean_us": mean(xs), "median_us": round(xs[len(xs) // 2], 2) if xs else None,
                      "max_us": round(xs[-1], 2) if xs else None}
    return out


def carry(args):
    rows = []
    for shape in SHAPES:
        N = shape[3]
        row = {"board": name_of(shape), "envs": N, "tree_nodes": TREE_NODES}
        sp = keeper(shape, "trivial")
        sp.advance(args.warmup)
        us, ended, _, _ = split_by_ply_ends(sp, KEEP, args.reps * args.rounds)
        mixed_launches = len(ended)
        row["mixed_budgets"] = classes(us, ended, N)
        J = 64  # every ply full, rows in step: every (J + 1)-th launch ends every row's ply and carries its subtree
        sp = keeper(shape, "trivial", iterations=J, fast=None, full_prob=1.0, tree_nodes=2 * J + 1)
        sp.advance(J + 1)
        us, ended, car, _ = split_by_ply_ends(sp, KEEP, args.reps * (J + 1))
        row["in_step_I64"] = classes(us, ended, N)
        row["in_step_I64"]["mean_nodes_kept"] = mean(car[[r for r, e in enumerate(ended) if e == N], :, 0].reshape(-1).tolist())
        rounds = {}
        for label, kw in (("keep_tree_off", None), ("keep_tree_on", {})):
            sp = player(shape, "conv") if kw is None else keeper(shape, "conv")
            sp.advance(args.warmup)
            rounds[label] = spread([timed(lambda: sp.advance(args.rounds)) / args.rounds for _ in range(args.reps)])
        row["conv_round_us"] = rounds
        mixed = row["mixed_budgets"]
        with_end = mixed["some_row"]["launches"] + mixed["every_row"]["launches"]
        if with_end and mixed["no_row"]["launches"]:
            extra = (mixed["some_row"]["mean_us"] or 0.0) - mixed["no_row"]["mean_us"]
            row["carry_share_of_conv_round"] = round(with_end / mixed_launches * extra / rounds["keep_tree_on"]["mean"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def carried(args):
    import numpy as np

    from oracle import philox

    rows = []
    for shape, kind in ((shape, kind) for shape in SHAPES for kind in ("trivial", "conv")):
        N = shape[3]
        sp = keeper(shape, kind)
        sp.advance(args.warmup)
        _, _, car, plies = split_by_ply_ends(sp, KEEP, args.calls)
        ids = np.arange(N, dtype=np.uint64) + np.uint64(sp.sampler.env_id0)
        kept = {"full": [], "fast": []}
        visits = {"full": [], "fast": []}
        for r in range(args.calls):
            for i in np.flatnonzero(plies[r + 1] != plies[r]):  # row i ended a ply: carried is its next ply's start
                word = philox.rand_u32(sp.sampler.seed, ids[i:i + 1], int(plies[r + 1, i]), 9)[0]
                label = "full" if int(word) < sp.full_threshold else "fast"
                kept[label].append(int(car[r, i, 0]))
                visits[label].append(int(car[r, i, 1]))
        row = {"board": name_of(shape), "envs": N, "evaluator": kind, "launches": args.calls, "tree_nodes": TREE_NODES,
               "keep_nodes": TREE_NODES - I}
        for label in ("full", "fast"):
            k, v = kept[label], visits[label]
            row[f"next_ply_{label}"] = {"plies": len(k), "mean_nodes_kept": mean(k), "max_nodes_kept": max(k, default=0),
                                        "mean_root_visits_carried": mean(v),
                                        "share_started_fresh": round(sum(1 for x in k if x == 0) / max(len(k), 1), 4),
                                        "share_truncated": round(sum(1 for x in k if x == TREE_NODES - I) / max(len(k), 1), 4)}
        row["games"] = sp.pop_game_stats()["games"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


# ----------------------------------------------------------------------------- peaked: the carry at a size that matters
def peaked_evaluator(cells):
    """priors that halve from cell to cell in the order a * 37 mod C, down to 2^-14 (the table of
    tests/search_selfplay_async_keep_cases.py), value 0: a search under them is narrow and deep, and a row carries tens to
    hundreds of nodes"""
    import torch

    table = (2.0 ** -torch.clamp((torch.arange(cells) * 37) % cells, max=14).float()).to("cuda")
    return lambda obs, mask: (mask.float() * table, torch.zeros(len(mask), device=mask.device))


def worker_peaked(args):
    """(a fresh process per library) one JSON line: per board, the launches split by ply ends and by the most nodes a row
    carried in them"""
    import numpy as np

    from exp_search_selfplay_async import SEED
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    out = {}
    for m, n, k, envs in SHAPES:
        sp = AsyncSearchSelfPlay(m, n, k, envs, evaluator=peaked_evaluator(m * n), iterations=I, fast_iterations=FAST,
                                 full_prob=FULL_PROB, temp_plies=8, seed=SEED, keep_tree=True, tree_nodes=TREE_NODES)
        sp.advance(args.warmup)
        us, ended, car, plies = split_by_ply_ends(sp, KEEP, args.reps * args.rounds)
        row = classes(us, ended, envs)
        moved = plies[1:] != plies[:-1]
        most = [int(car[r, moved[r], 0].max()) if moved[r].any() else -1 for r in range(len(us))]
        kept = np.concatenate([car[r, moved[r], 0] for r in range(len(us))]) if moved.any() else np.zeros(0)
        row["nodes_kept"] = {"plies": int(len(kept)), "mean": mean(kept.tolist()), "max": int(kept.max()) if len(kept) else 0,
                             "share_truncated": round(float((kept == TREE_NODES - I).mean()), 4) if len(kept) else 0.0}
        row["by_most_nodes_a_row_carried"] = {}
        for label, lo, hi in (("1-8", 1, 8), ("9-64", 9, 64), ("65-256", 65, 256), ("257", 257, 257)):
            xs = sorted(u for u, q in zip(us, most) if lo <= q <= hi)
            row["by_most_nodes_a_row_carried"][label] = {"launches": len(xs), "mean_us": mean(xs),
                                                         "median_us": round(xs[len(xs) // 2], 2) if xs else None}
        row["mean_us_all_launches"] = mean(us)
        out[name_of((m, n, k))] = row
    print("RESULT " + json.dumps(out), flush=True)


def peaked(args):
    """this build (B = 8 nodes in flight in the carry's copy loop) and, with ``--carry-lib LABEL=PATH``, builds with another
    B: fresh processes that alternate, every process repeating the same rounds of the same games"""
    import subprocess

    libs = {"B=8 (this build)": None}
    for spec in args.carry_lib:
        label, path = spec.split("=", 1)
        libs["B=" + label] = os.path.abspath(path)
    out = {label: [] for label in libs}
    for _ in range(args.processes):
        for label, path in libs.items():
            env = dict(os.environ)
            if path:
                env["MNK_HIP_LIB"] = path
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(args.warmup),
                                   "--rounds", str(args.rounds), "--reps", str(args.reps)], env=env, check=True,
                                  capture_output=True, text=True, timeout=600)
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            out[label].append(json.loads(line[7:]))
            print(label, line[7:], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--carry-lib", action="append", default=[], metavar="B=PATH",
                    help="a build of the library with -DMNK_KEEP_CARRY_B=B, for the peaked comparison")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmnk_hip.so, for the plain comparison")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per build in the plain comparison")
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=400, help="launches per repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1500, help="launches of the run whose carried trees are counted")
    ap.add_argument("--only", choices=("plain", "peaked", "launch", "carry", "carried"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_search_selfplay_async_keep.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    if not os.environ.get("MNK_HIP_LIB"):
        entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    if args.worker:
        return worker_peaked(args)
    out = {}
    if os.path.exists(args.out):  # (--only: the other parts stay as they were measured)
        with open(args.out) as f:
            out.update(json.load(f))
    # (plain and peaked first: their fresh processes start before this one has touched the GPU)
    for part, fn in (("plain", opts.plain), ("peaked", peaked), ("launch", launch), ("carry", carry), ("carried", carried)):
        if args.only in (None, part):
            out[part] = fn(args)
            if part not in ("plain", "peaked"):
                out["device"] = torch.cuda.get_device_name(0)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
