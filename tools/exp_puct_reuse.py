"""Developer tool: what keeping the PUCT tree between plies (PUCTSearchPolicy(reuse=True) / mnk_puct_rebase) costs and
what it buys.

Cost: ``SearchSelfPlay(reuse=True)`` with the conv-net evaluator of tools/exp_puct.py on 9x9x5 x 1 024 rows and 19x19x5 x
256 rows, J = 256, tree_nodes = 513.  Every ``mnk_puct_rebase`` launch is bracketed with device events (the stream is
busy before and after it, so the bracket holds the kernel and little else); the ply is timed the same way, and its time
over J + 1 is the cost of one iteration (evaluator call + ``mnk_puct_step``) in the same run.  ``whole``: the same
position searched twice, so that every row carries the most a rebase may carry (tree_nodes - J nodes).

Gain: 9x9x5 self-play with the heuristic evaluator of tests/test_gpu_puct.py (priors over the tactical candidates, value
from four playouts) at J = 64 and J = 256: the visits a ply's search starts with; and over 256 games each (half as black)
the score of reuse(J) against fresh(J) and of reuse(J / 2) against fresh(J).

usage: python tools/exp_puct_reuse.py [--plies 6] [--games 256] [--out profiles/exp_puct_reuse.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
# (m, n, k, rows, J, tree_nodes)
COST_CASES = ((9, 9, 5, 1024, 256, 513), (19, 19, 5, 256, 256, 513))


class Bracket:
    """device events around every launch of one entry point"""

    def __init__(self, name):
        import mnk_hip

        self.name, self.lib, self.inner, self.pairs = name, mnk_hip, mnk_hip.call, []

    def __enter__(self):
        import torch

        def call(name, *args):
            if name != self.name:
                return self.inner(name, *args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = self.inner(name, *args)
            e1.record()
            self.pairs.append((e0, e1))
            return rc

        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.inner

    def pop_us(self):
        import torch

        torch.cuda.synchronize()
        out = [a.elapsed_time(b) * 1e3 for a, b in self.pairs]
        del self.pairs[:]
        return out


def cost(m, n, k, rows, J, tree_nodes, plies):
    import torch
    from exp_puct import evaluator

    from selfplay.search_selfplay import SearchSelfPlay

    sp = SearchSelfPlay(m, n, k, rows, evaluator=evaluator("conv", m * n), iterations=J, temp_plies=8, seed=1, reuse=True,
                        tree_nodes=tree_nodes)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rebase, ply_us, nodes, share = [], [], [], []
    with Bracket("mnk_puct_rebase") as br:
        sp.play(1)
        br.pop_us()
        for _ in range(plies):
            e0.record()
            sp.play(1)
            e1.record()
            rebase += br.pop_us()
            ply_us.append(e0.elapsed_time(e1) * 1e3)
            c = sp.carried.cpu()
            nodes.append(float(c[:, 0].float().mean()))
            share.append(float((c[:, 0] > 0).float().mean()))
        # the most a rebase may carry: the same roots again, every row keeps tree_nodes - J nodes
        obs = {"observation": sp.obs.clone(), "action_mask": sp.mask.clone()}
        whole = []
        for _ in range(3):
            sp.policy.act(obs, carried=sp.carried)
            whole += br.pop_us()
        kept = float(sp.carried[:, 0].float().mean())
    return {"board": f"{m}x{n}x{k}", "rows": rows, "J": J, "tree_nodes": tree_nodes, "evaluator": "conv",
            "us_per_iteration": round(statistics.median(ply_us) / (J + 1), 2),
            "rebase_us_selfplay": round(statistics.median(rebase), 1), "rebase_us_selfplay_max": round(max(rebase), 1),
            "nodes_kept_selfplay": round(statistics.mean(nodes), 1), "rows_continued": round(statistics.mean(share), 3),
            "rebase_us_whole": round(statistics.median(whole[1:]), 1), "nodes_kept_whole": round(kept, 1),
            "bytes_per_kept_node": 12 + 6 * m * n}


def carried_visits(J, plies, envs=256):
    from test_gpu_puct import heuristic_evaluator

    from selfplay.search_selfplay import SearchSelfPlay

    sp = SearchSelfPlay(9, 9, 5, envs, evaluator=heuristic_evaluator(5), iterations=J, seed=2, reuse=True)
    visits, nodes = [], []
    for _ in range(plies):
        sp.play(1)
        c = sp.carried.cpu().float()
        visits.append(float(c[:, 1].mean()))
        nodes.append(float(c[:, 0].mean()))
    return {"board": "9x9x5", "envs": envs, "J": J, "plies": plies, "evaluator": "heuristic",
            "mean_carried_root_visits": round(statistics.mean(visits[1:]), 1),
            "mean_carried_nodes": round(statistics.mean(nodes[1:]), 1),
            "share_of_J": round(statistics.mean(visits[1:]) / J, 3)}


def match(J_reuse, J_fresh, games, seed):
    from test_gpu_puct import heuristic_evaluator

    from selfplay.policy import PUCTSearchPolicy
    from selfplay.tournament import play_match

    a = PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=J_reuse, seed=seed, reuse=True)
    b = PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=J_fresh, seed=seed + 1)
    res = play_match(a, b, (9, 9, 5), games, device="cuda:0")
    p = res["score"]
    return {"board": "9x9x5", "reuse_J": J_reuse, "fresh_J": J_fresh, "games": games, "wins": res["wins"],
            "losses": res["losses"], "draws": res["draws"], "score": round(p, 4),
            "standard_error": round((max(p * (1 - p), 1e-9) / games) ** 0.5, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=6)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct_reuse.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    out = {"device": torch.cuda.get_device_name(0), "rebase": [], "carried": [], "matches": []}
    for case in COST_CASES:
        out["rebase"].append(cost(*case, args.plies))
        print(json.dumps(out["rebase"][-1]), flush=True)
    for J in (64, 256):
        out["carried"].append(carried_visits(J, 40))
        print(json.dumps(out["carried"][-1]), flush=True)
    for i, J in enumerate((64, 256)):
        for Jr in (J, J // 2):
            out["matches"].append(match(Jr, J, args.games, 10 + 4 * i + (Jr != J) * 2))
            print(json.dumps(out["matches"][-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
