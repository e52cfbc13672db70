"""Developer tool: what the flat Monte Carlo player (MonteCarloPolicy / mnk_sample_playouts) costs, and how strong it is.

Timing: ``MonteCarloPolicy.act`` on N rows of random mid-game positions (up to half the board filled by uniformly random
play, tests/tactical_rule.random_positions), timed with device events around ``reps`` back-to-back calls after a warm-up;
µs per call, playouts/s (|L| * P per row) and plies/s.  The kernel does not count its plies: the mean playout length
comes from the numpy restatement (tests/playout_rule.py) on a sample of the same rows, plies/s = playouts/s * that mean.

Strength: ``tournament.play_match`` W / D / L of MC(16), MC(64), MC(256) against RandomPolicy and TacticalPolicy(k) on
9x9x5, 1024 games each (half as black), plus MC(256) against MC(16) and Random against Tactical.

usage: python tools/exp_playouts.py [--reps 20] [--no-strength] [--out profiles/exp_playouts.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests")]
CASES = ((9, 9, 5, 1024, 64), (3, 3, 3, 1024, 256), (19, 19, 5, 256, 32), (9, 9, 5, 1, 1024), (9, 9, 5, 4096, 16))


def timing(m, n, k, rows, P, reps):
    import numpy as np
    import torch

    from playout_rule import playout_counts
    from selfplay.policy import MonteCarloPolicy
    from tactical_rule import random_positions

    obs_np = random_positions(m, n, k, rows, np.random.default_rng(m * n + P), max_fill=0.5)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
    pol = MonteCarloPolicy(k, P, seed=1)
    for _ in range(3):
        pol.act(obs)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        pol.act(obs)
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    legal = int(((obs_np[:, 0] == 0) & (obs_np[:, 1] == 0)).sum())
    playouts = legal * P
    sample = min(rows, 4)
    plies = []
    p_sample = min(P, 4)
    playout_counts(obs_np[:sample], k, p_sample, seed=1, plies=plies)
    legal_s = int(((obs_np[:sample, 0] == 0) & (obs_np[:sample, 1] == 0)).sum())
    mean_len = plies[0] / max(1, legal_s * p_sample)
    return {"board": f"{m}x{n}x{k}", "rows": rows, "playouts": P, "us_per_call": round(us, 2),
            "playouts_per_s": float("%.4g" % (playouts / us * 1e6)), "mean_plies_per_playout": round(mean_len, 2),
            "plies_per_s": float("%.4g" % (playouts * mean_len / us * 1e6))}


def strength(m, n, k, games):
    from selfplay.policy import MonteCarloPolicy, RandomPolicy, TacticalPolicy
    from selfplay.tournament import play_match

    out = []
    pairs = [(f"MC({p})", f"{opp}", MonteCarloPolicy(k, p, seed=10 + p),
              RandomPolicy(m * n, seed=2) if opp == "Random" else TacticalPolicy(k, seed=3))
             for p in (16, 64, 256) for opp in ("Random", "Tactical")]
    pairs.append(("MC(256)", "MC(16)", MonteCarloPolicy(k, 256, seed=7), MonteCarloPolicy(k, 16, seed=8)))
    pairs.append(("Random", "Tactical", RandomPolicy(m * n, seed=5), TacticalPolicy(k, seed=6)))
    for a, b, pa, pb in pairs:
        t = time.time()
        res = play_match(pa, pb, (m, n, k), games, device="cuda:0")
        out.append({"board": f"{m}x{n}x{k}", "player": a, "opponent": b, "games": games, "wins": res["wins"],
                    "draws": res["draws"], "losses": res["losses"], "score": round(res["score"], 4),
                    "seconds": round(time.time() - t, 2)})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-strength", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as entry

    entry.build_hip()
    res = {"timing": [], "strength": []}
    for m, n, k, rows, P in CASES:
        res["timing"].append(timing(m, n, k, rows, P, args.reps))
        print(json.dumps(res["timing"][-1]), flush=True)
    if not args.no_strength:
        res["strength"] = strength(9, 9, 5, 1024) + strength(3, 3, 3, 1024)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
