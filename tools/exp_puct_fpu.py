"""Developer tool: what first-play urgency (PUCTSearchPolicy(fpu=...)) costs per step, what it changes in the tree and
what it does to the player's strength.

``--cost``: on 9x9x5 x 1 024 and 19x19x5 x 256 rows of random mid-game positions with the conv net of tools/exp_puct.py,
``act`` at I = 256 with L = 1 and 4, the solver off and on, without and with ``fpu=0.2``, in ONE process: every policy is
built and warmed up first, then ``--reps`` passes over the policies in turn, device events around every step launch in the
busy stream (the evaluator's kernels run between them) and around the act.  Reported: the median step launch of the plain
policy (``k_puct_step`` / ``k_puct_step_leaves`` / ``k_puct_step_solver``) and of the FPU one (``k_puct_step_fpu``), their
difference, and the difference as a share of one iteration (evaluator + step) of the same run.  The two policies search
different trees: the difference holds the second pass over the child row AND whatever the other tree's shape costs
(``last_leaf_depth_*``: the mean depth of the last leaf the rows selected, read from the workspace).

``--tree``: 19x19x5 x 256 rows, I = 256, the heuristic evaluator of tests/test_gpu_puct.py: the distinct root children
visited, split by the sign of ``root_value``, without and with ``fpu=0.2``.

``--strength``: ``fpu=0.2`` against plain at equal I in {64, 256} on 9x9x5 with that evaluator, 256 games, half as black:
score and standard error.

``--kernels [--parent DIR]``: needs no GPU.  Compiles mnk_puct.hip and the three mnk_search_selfplay_async*.hip units to
gfx950 assembly with the compiler's resource report (``-S -Rpass-analysis=kernel-resource-usage``, the flags of
``__graft_entry__.build_hip``) and writes profiles/exp_puct_fpu_kernels.md: VGPRs, scratch and LDS of every new variant
beside its sibling's and, with ``--parent`` (the csrc directory of a checkout of the parent commit), which existing kernels'
instructions differ from the parent's (compared line by line, block labels renumbered).

usage: python tools/exp_puct_fpu.py [--cost] [--tree] [--strength] [--reps 5] [--out profiles/exp_puct_fpu.json]
       python tools/exp_puct_fpu.py --kernels [--parent DIR] [--work DIR]"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
CSRC = os.path.join(ROOT, "rl-selfplay-mnk_amd", "csrc")
SHAPES = (("9x9x5 x 1024", 9, 9, 5, 1024), ("19x19x5 x 256", 19, 19, 5, 256))
LEAVES, I, FPU = (1, 4), 256, 0.2
STEPS = ("mnk_puct_step", "mnk_puct_step_leaves", "mnk_puct_step_solver", "mnk_puct_step_fpu")
UNITS = ("mnk_puct", "mnk_search_selfplay_async", "mnk_search_selfplay_async_leaves", "mnk_search_selfplay_async_gumbel")


# ----------------------------------------------------------------------------- cost
def cost(shape, reps):
    import numpy as np
    import torch

    from exp_puct import evaluator
    from exp_search_selfplay_async import LaunchEvents
    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions

    name, m, n, k, rows = shape
    obs_np = random_positions(m, n, k, rows, np.random.default_rng(m * n + I), max_fill=0.5)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
    ev = evaluator("conv", m * n)
    keys = [(L, s, f) for L in LEAVES for s in (False, True) for f in (None, FPU)]
    pols = {key: PUCTSearchPolicy(k, evaluator=ev, iterations=I, seed=1, leaves=key[0], solver=key[1], fpu=key[2])
            for key in keys}
    for pol in pols.values():  # warm-up: every batch shape, the buffers
        for _ in range(2):
            pol.act(obs)
    torch.cuda.synchronize()
    # the depth of the last leaf every row selected (slot 0's, the second word of a row's workspace): how deep the two trees are
    depth = {}
    for key, pol in pols.items():
        words = pol._bufs[1].view(torch.int32)
        depth[key] = words[1::len(words) // rows][:rows].float().mean().item()
    step_us, act_us = {key: [] for key in keys}, {key: [] for key in keys}
    for _ in range(reps):
        for key, pol in pols.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with LaunchEvents(STEPS) as events:
                e0.record()
                pol.act(obs)
                e1.record()
            (launches,) = events.us().values()  # (a policy calls one step entry point)
            step_us[key] += launches[1:-1]  # (without the root's backup and the move)
            act_us[key].append(e0.elapsed_time(e1) * 1e3)
    out = []
    for L in LEAVES:
        for solver in (False, True):
            plain, fpu = (L, solver, None), (L, solver, FPU)
            p, f = statistics.median(step_us[plain]), statistics.median(step_us[fpu])
            iteration = statistics.median(act_us[plain]) / (I // L + 1)
            out.append({"shape": name, "iterations": I, "leaves": L, "solver": solver, "step_us_plain": round(p, 2),
                        "step_us_fpu": round(f, 2), "step_us_more": round(f - p, 2),
                        "iteration_us_plain": round(iteration, 1), "more_as_share_of_iteration": round((f - p) / iteration, 4),
                        "act_us_plain": round(statistics.median(act_us[plain]), 1),
                        "act_us_fpu": round(statistics.median(act_us[fpu]), 1),
                        "last_leaf_depth_plain": round(depth[plain], 2), "last_leaf_depth_fpu": round(depth[fpu], 2)})
    return out


# ----------------------------------------------------------------------------- the tree
def tree():
    import numpy as np
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions
    from test_gpu_puct import heuristic_evaluator

    m, n, k, rows = 19, 19, 5, 256
    obs_np = random_positions(m, n, k, rows, np.random.default_rng(19), max_fill=0.3)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
    out = []
    for fpu in (None, FPU):
        pol = PUCTSearchPolicy(k, evaluator=heuristic_evaluator(k), iterations=I, seed=3, fpu=fpu)
        visits = torch.zeros((rows, m * n), dtype=torch.int32, device="cuda:0")
        value = torch.zeros(rows, device="cuda:0")
        pol.act(obs, visits=visits, root_value=value)
        distinct, value = (visits > 0).sum(dim=1).float().cpu(), value.cpu()
        row = {"board": "19x19x5", "rows": rows, "iterations": I, "fpu": fpu}
        for sign, sel in (("root_value<0", value < 0), ("root_value>=0", value >= 0)):
            row[sign] = {"rows": int(sel.sum()), "distinct_children_mean": round(distinct[sel].mean().item(), 2) if sel.any() else None,
                         "distinct_children_median": distinct[sel].median().item() if sel.any() else None,
                         "top_child_share_mean": round((visits.max(dim=1).values.float().cpu()[sel] / I).mean().item(), 4)
                         if sel.any() else None}
        out.append(row)
    return out


# ----------------------------------------------------------------------------- strength
def strength():
    from selfplay import tournament
    from selfplay.policy import PUCTSearchPolicy
    from test_gpu_puct import heuristic_evaluator

    out, games = [], 256
    for iters in (64, 256):
        a = PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=iters, seed=14, fpu=FPU)
        b = PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=iters, seed=15)
        res = tournament.play_match(a, b, (9, 9, 5), games, device="cuda:0")
        w, d, l = res["wins"], res["draws"], res["losses"]
        score = (w + 0.5 * d) / games
        se = math.sqrt(max((w + 0.25 * d) / games - score * score, 0.0) / games)
        out.append({"board": "9x9x5", "iterations": iters, "games": games, "wins": w, "draws": d, "losses": l,
                    "score": round(score, 4), "standard_error": round(se, 4),
                    "standard_errors_above_half": round((score - 0.5) / se, 2) if se else None})
    return out


# ----------------------------------------------------------------------------- the kernels (no GPU)
def compile_units(csrc, work, tag):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S",
             "-Rpass-analysis=kernel-resource-usage"]
    procs = []
    for unit in UNITS:
        res = open(os.path.join(work, f"{tag}_{unit}.res"), "w")
        procs.append(subprocess.Popen([hipcc] + flags + [unit + ".hip", "-o", os.path.join(work, f"{tag}_{unit}.s")],
                                      cwd=csrc, stderr=res))
    for pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, pr.args)


def resources(path):
    """{mangled name: {"VGPRs": .., "ScratchSize": .., "LDS": .., "SGPRs": .., "Occupancy": ..}} of a resource report"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def bodies(path):
    """{mangled name: [instruction lines, comments dropped, block labels renumbered]} of an assembly file"""
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, cur = m.group(1), []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name], cur = cur, None
            else:
                s = re.sub(r"\.LBB\d+_\d+", ".L", line.split(";")[0].rstrip())
                if s.strip() and not s.lstrip().startswith("."):
                    cur.append(s)
    return out


def demangled(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, (re.sub(r"\(.*", "", x).replace("void ", "") for x in res.stdout.split("\n"))))


def kernels(parent, work, out_path):
    compile_units(CSRC, work, "new")
    if parent:
        compile_units(parent, work, "parent")
    lines = ["# First-play urgency: registers of the new kernels, and what became of the existing ones", "",
             "Taken without a GPU by `python tools/exp_puct_fpu.py --kernels --parent <parent csrc>`: the units compiled to",
             "gfx950 assembly with `-O3 -ffp-contract=off -S -Rpass-analysis=kernel-resource-usage`; registers, scratch and",
             "LDS from the compiler's resource report, instructions counted in the assembly.", "",
             "## The new variants beside their siblings", "",
             "| kernel | VGPRs | sibling | sibling's VGPRs | instructions | sibling's | LDS B | scratch B/lane | VGPR spills | SGPRs "
             "kept in VGPR lanes, sibling's |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    names = {}
    for unit in UNITS[:2]:
        res, asm = resources(os.path.join(work, f"new_{unit}.res")), bodies(os.path.join(work, f"new_{unit}.s"))
        dm = demangled(list(res))
        by_name = {v: k for k, v in dm.items()}
        names.update(dm)
        for mangled, plain in dm.items():
            args = re.search(r"<(.*)>", plain).group(1).split(", ")
            if plain.startswith("k_puct_step_fpu"):
                sib = ("k_puct_step_solver" if args[3] == "true" else "k_puct_step_leaves") + "<" + ", ".join(args[:3]) + ">"
            elif re.match(r"k_search_selfplay_advance_(opts|keep)<", plain) and args[4] == "true":
                sib = plain.split("<")[0] + "<" + ", ".join(args[:4]) + ", false>"  # (FPU: the kernels' last template flag)
            else:
                continue
            r, s = res[mangled], res[by_name[sib]]
            lines.append(f"| `{plain}` | {r['VGPRs']} | `{sib.split('<')[0]}` | {s['VGPRs']} | {len(asm[mangled])} | "
                         f"{len(asm[by_name[sib]])} | {r['LDS Size']} | {r['ScratchSize']} | "
                         f"{r['VGPRs Spill']} | {r['SGPRs Spill']}, {s['SGPRs Spill']} |")
    if parent:
        lines += ["", "## The existing kernels against the parent's", "",
                  "| unit | kernels in the parent | identical | differ | instructions of those, parent / now | same VGPRs | new kernels |",
                  "|---|---|---|---|---|---|---|"]
        moved = []
        for unit in UNITS:
            a, b = bodies(os.path.join(work, f"parent_{unit}.s")), bodies(os.path.join(work, f"new_{unit}.s"))
            ra, rb = resources(os.path.join(work, f"parent_{unit}.res")), resources(os.path.join(work, f"new_{unit}.res"))
            differ = [k for k in a if k in b and a[k] != b[k]]
            lines.append(f"| {unit}.hip | {len(a)} | {sum(1 for k in a if k in b and a[k] == b[k])} | {len(differ)} | "
                         f"{sum(len(a[k]) for k in differ)} / {sum(len(b[k]) for k in differ)} | "
                         f"{sum(1 for k in a if k in b and ra[k]['VGPRs'] == rb[k]['VGPRs'])} of {len(a)} | "
                         f"{sum(1 for k in b if k not in a)} |")
            moved += [(unit, k, len(a[k]), len(b[k]), ra[k]["VGPRs"], rb[k]["VGPRs"], rb[k]["ScratchSize"]) for k in differ]
        if moved:
            lines += ["", "A kernel listed below has the parent's name, parameter list, registers and LDS; its body became a device",
                      "function that the kernel with first-play urgency inlines too, and the compiler laid the same operations",
                      "out differently (commutative operands swapped, independent instructions reordered, some blocks placed",
                      "elsewhere)."]
            dm = demangled([k for _, k, *_ in moved])
            lines += ["", "| kernel whose instructions differ | instructions parent / now | VGPRs parent / now | scratch now |",
                      "|---|---|---|---|"]
            lines += [f"| `{dm[k]}` | {x} / {y} | {va} / {vb} | {sc} |" for _, k, x, y, va, vb, sc in moved]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct_fpu.json"))
    for name in ("cost", "tree", "strength", "kernels"):
        ap.add_argument("--" + name, action="store_true")
    ap.add_argument("--parent", help="--kernels: the csrc directory of a checkout of the parent commit")
    ap.add_argument("--work", help="--kernels: where the assembly goes (default: a temporary directory)")
    args = ap.parse_args()
    if args.kernels:
        md = os.path.join(ROOT, "profiles", "exp_puct_fpu_kernels.md")
        if args.work:
            os.makedirs(args.work, exist_ok=True)
            kernels(args.parent, args.work, md)
        else:
            with tempfile.TemporaryDirectory() as work:
                kernels(args.parent, work, md)
        return
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    data = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            data = json.load(f)
    data["device"] = torch.cuda.get_device_name(0)
    every = not (args.cost or args.tree or args.strength)
    if args.cost or every:
        data["cost"] = [row for shape in SHAPES for row in cost(shape, args.reps)]
    if args.tree or every:
        data["tree"] = tree()
    if args.strength or every:
        data["strength"] = strength()
    for part in ("cost", "tree", "strength"):
        for row in data.get(part, ()):
            print(part, json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
