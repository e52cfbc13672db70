"""Developer tool: the kernels of the PUCT player (csrc/mnk_puct.hip), built from one step body and the pieces of
csrc/mnk_puct_tree.h, and the advance kernels that share those pieces, against the parent commit's copies: the same
resources, and the same time.

``--kernels --parent DIR`` (needs no GPU; DIR: the csrc directory of a checkout of the parent commit): mnk_puct.hip and the
three mnk_search_selfplay_async*.hip units of both trees compiled to gfx950 assembly with the compiler's resource report
(tools/exp_puct_fpu.py's ``compile_units``), and every kernel beside the parent's of the same role -- the parent's
``k_puct_begin<..>`` and ``k_puct_rebase<..>`` are the ``_leaves`` kernels now, its ``k_puct_step_leaves<..>``,
``k_puct_step_solver<..>`` and ``k_puct_step_fpu<.., S>`` are ``k_puct_step_leaves<.., S, FPU>``: static LDS, scratch, VGPR
spills and waves per SIMD are gates, instruction counts are reported, and whether a unit's assembly is the parent's.  Writes
profiles/exp_puct_step_pieces_kernels.md.

``--parent-lib PATH`` (the GPU): us per launch, device events around every launch in the busy stream, of the entry points
of ``PUCTSearchPolicy.act`` with the trivial evaluator of tools/exp_puct.py on 9x9x5 x 1 024 and 19x19x5 x 256 rows of
``random_positions`` at I = 256 (the Gumbel row: I = 32, m = 16), of this build against the parent's library in fresh
processes that alternate (tools/exp_search_selfplay_async_opts.py's harness).  The bar for every row and shape: this build's
mean is no higher than the parent's maximum over its repetitions.  Writes profiles/exp_puct_step_pieces.json.

usage: python tools/exp_puct_step_pieces.py --kernels --parent DIR [--work DIR]
       python tools/exp_puct_step_pieces.py --parent-lib PATH [--processes 2] [--reps 5]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
UNITS = ("mnk_puct", "mnk_search_selfplay_async", "mnk_search_selfplay_async_leaves", "mnk_search_selfplay_async_gumbel")
PROFILES = os.path.join(ROOT, "profiles")
SHAPES = ((9, 9, 5, 1024), (19, 19, 5, 256))
I, FPU = 256, 0.2
# row: (the entry point measured, the policy's options)
ROWS = {"step": ("mnk_puct_step", {}),
        "step_leaves": ("mnk_puct_step_leaves", {"leaves": 4}),
        "step_solver": ("mnk_puct_step_solver", {"leaves": 4, "solver": True}),
        "step_fpu": ("mnk_puct_step_fpu", {"leaves": 4, "fpu": FPU}),
        "step_fpu_solver": ("mnk_puct_step_fpu", {"leaves": 4, "fpu": FPU, "solver": True}),
        "step_gumbel": ("mnk_puct_step_gumbel", {"gumbel": 16, "iterations": 32}),
        "begin": ("mnk_puct_begin", {}),
        "rebase": ("mnk_puct_rebase", {"reuse": True})}
GROWTH_LOOKED_AT = 0.023  # the largest growth the first-play-urgency change was accepted with on these kernels


# ----------------------------------------------------------------------------- the kernels (no GPU)
def now_name(parent_name):
    """the name the kernel of the parent's role has now"""
    m = re.match(r"k_puct_(begin|rebase)<(.*)>$", parent_name)
    if m:
        return f"k_puct_{m.group(1)}_leaves<{m.group(2)}>"
    m = re.match(r"k_puct_step_(leaves|solver)<(.*)>$", parent_name)
    if m:
        return f"k_puct_step_leaves<{m.group(2)}, {'true' if m.group(1) == 'solver' else 'false'}, false>"
    m = re.match(r"k_puct_step_fpu<(.*)>$", parent_name)
    return f"k_puct_step_leaves<{m.group(1)}, true>" if m else parent_name


def kernels(parent, work):
    import exp_puct_fpu as fpu

    fpu.UNITS = UNITS
    fpu.compile_units(os.path.join(ROOT, "rl-selfplay-mnk_amd", "csrc"), work, "new")
    fpu.compile_units(parent, work, "parent")
    rows, bad, same_unit, counts = [], [], {}, {}
    for unit in UNITS:
        ra, rb = (fpu.resources(os.path.join(work, f"{tag}_{unit}.res")) for tag in ("parent", "new"))
        aa, ab = (fpu.bodies(os.path.join(work, f"{tag}_{unit}.s")) for tag in ("parent", "new"))
        da, db = fpu.demangled(list(ra)), fpu.demangled(list(rb))
        by_name = {v: k for k, v in db.items()}
        assert sorted(set(now_name(v) for v in da.values())) == sorted(by_name), unit  # (every kernel has its role's parent)
        same_unit[unit] = set(aa) == set(ab) and all(aa[k] == ab[k] for k in aa)
        counts[unit] = (len(da), len(db))
        for mangled, name in da.items():
            other = by_name[now_name(name)]
            p, q, x, y = ra[mangled], rb[other], len(aa[mangled]), len(ab[other])
            gates = (q["LDS Size"] == p["LDS Size"] and q["ScratchSize"] == 0 and q["VGPRs Spill"] == 0
                     and q["Occupancy"] >= p["Occupancy"])
            rows.append((unit, name, now_name(name), p, q, x, y, gates))
            if not gates:
                bad.append(f"{name} -> {now_name(name)}")
    grown = [r for r in rows if r[6] > r[5] * (1 + GROWTH_LOOKED_AT)]
    lines = ["# The PUCT player's kernels from one step body and shared pieces: resources against the parent's copies", "",
             "Taken without a GPU by `python tools/exp_puct_step_pieces.py --kernels --parent <parent csrc>`: the four units",
             "compiled to gfx950 assembly with `-O3 -ffp-contract=off -S -Rpass-analysis=kernel-resource-usage`; registers,",
             "scratch, LDS and waves per SIMD from the compiler's resource report, instructions counted in the assembly.  The",
             "gates: the parent's static LDS, scratch 0, no VGPR spill, no fewer waves per SIMD.  A row is a kernel of the",
             "parent beside the kernel that has its role now (the `_leaves` begin and rebase kernels stand in two rows each).", "",
             "Kernels per unit, parent / now: " + ", ".join(f"{u}.hip {a} / {b}" for u, (a, b) in counts.items()) + ".",
             "Assembly identical to the parent's, kernel for kernel: "
             + ", ".join(f"{u}.hip {'yes' if s else 'no'}" for u, s in same_unit.items()) + ".",
             f"{len(rows)} rows; {len(rows) - len(bad)} pass every gate"
             + (f"; FAILING: {', '.join('`' + b + '`' for b in bad)}" if bad else "") + ".",
             f"Instructions, all rows: {sum(r[5] for r in rows)} in the parent, {sum(r[6] for r in rows)} now "
             f"({100.0 * (sum(r[6] for r in rows) / sum(r[5] for r in rows) - 1):+.2f} %); "
             f"{len(grown)} rows grew by more than {100 * GROWTH_LOOKED_AT:.1f} %.", "",
             "| the parent's kernel | now | waves/SIMD parent / now | VGPRs parent / now | SGPRs parent / now | LDS B parent / now | "
             "scratch now | VGPR spills now | instructions parent / now | change |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for unit, name, now, p, q, x, y, gates in rows:
        lines.append(f"| `{name}` | {'same name' if now == name else '`' + now + '`'} | {p['Occupancy']} / {q['Occupancy']} | "
                     f"{p['VGPRs']} / {q['VGPRs']} | {p['TotalSGPRs']} / {q['TotalSGPRs']} | {p['LDS Size']} / {q['LDS Size']} | "
                     f"{q['ScratchSize']} | {q['VGPRs Spill']} | {x} / {y} | "
                     f"{100.0 * (y / x - 1):+.1f} %{'' if gates else ' GATE'} |")
    text = "\n".join(lines) + "\n"
    notes = os.path.join(PROFILES, "exp_puct_step_pieces_kernels_notes.md")
    if os.path.exists(notes):  # (what a person wrote about the kernels that grew: kept beside the table, appended to it)
        text += "\n" + open(notes).read()
    with open(os.path.join(PROFILES, "exp_puct_step_pieces_kernels.md"), "w") as f:
        f.write(text)
    print(text)
    return 1 if bad else 0


# ----------------------------------------------------------------------------- the launches (the GPU)
def name_of(shape):
    return "x".join(map(str, shape[:3]))


def played(obs, actions):
    """the rows after their move, as the next side to move sees them"""
    import torch

    b, _, m, n = obs.shape
    stone = torch.zeros((b, m * n), device=obs.device).scatter_(1, actions.view(-1, 1), 1.0).view(b, m, n)
    return torch.stack([obs[:, 1], obs[:, 0] + stone], dim=1)


def worker(args):
    """(a fresh process per build: the library is loaded once) one JSON line {row: {board: [us per launch, ...]}}"""
    import numpy as np
    import torch

    from exp_puct import evaluator
    from exp_search_selfplay_async import LaunchEvents, mean
    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions

    out = {}
    for row, (entry_point, options) in ROWS.items():
        out[row] = {}
        for m, n, k, rows in SHAPES:
            obs = torch.from_numpy(random_positions(m, n, k, rows, np.random.default_rng(m * n + I), max_fill=0.5)).to("cuda:0")
            kw = dict({"iterations": I}, **options)
            pol = PUCTSearchPolicy(k, evaluator=evaluator("trivial", m * n), seed=1, **kw)

            def act_pair():  # (reuse: the second act continues the first one's tree, one ply on; the first starts afresh)
                a = pol.act({"observation": obs})
                if pol.reuse:
                    pol.act({"observation": played(obs, a)})

            us = []
            for rep in range(args.warmup + args.reps):
                with LaunchEvents((entry_point,)) as ev:
                    for _ in range(args.acts):
                        act_pair()
                launches = ev.us()[entry_point]
                if pol.reuse:
                    launches = launches[1::2]  # (the second act of each pair)
                if rep >= args.warmup:
                    us.append(mean(launches))
            out[row][name_of((m, n, k))] = us
    print("RESULT " + json.dumps(out), flush=True)


def launches(args):
    import exp_search_selfplay_async_opts as opts

    builds = {"this": None, "parent": os.path.abspath(args.parent_lib)}
    runs = {b: {} for b in builds}
    for _ in range(args.processes):
        for build, path in reversed(list(builds.items())):  # parent, this, parent, this, ...
            env = dict(os.environ)
            if path:
                env["MNK_HIP_LIB"] = path
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(args.warmup),
                                   "--acts", str(args.acts), "--reps", str(args.reps)], env=env, check=True,
                                  capture_output=True, text=True, timeout=240)
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            for row, boards in json.loads(line[7:]).items():
                for board, us in boards.items():
                    runs[build].setdefault((row, board), []).extend(us)
    rows = []
    for (row, board), us in runs["this"].items():
        this, par = opts.spread(us), opts.spread(runs["parent"][(row, board)])
        out = {"row": row, "entry_point": ROWS[row][0], "options": ROWS[row][1], "board": board,
               "iterations": ROWS[row][1].get("iterations", I), "acts_per_repetition": args.acts, "this_us_per_launch": this,
               "parent_us_per_launch": par, "this_mean_no_higher_than_parent_max": this["mean"] <= par["max"]}
        print(json.dumps(out), flush=True)
        rows.append(out)
    with open(args.out, "w") as f:
        json.dump({"launches": rows}, f, indent=1)
    return 0 if all(r["this_mean_no_higher_than_parent_max"] for r in rows) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--parent", help="--kernels: the csrc directory of a checkout of the parent commit")
    ap.add_argument("--work", help="--kernels: where the assembly goes (default: a temporary directory)")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmnk_hip.so")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per build")
    ap.add_argument("--warmup", type=int, default=1, help="repetitions thrown away")
    ap.add_argument("--acts", type=int, default=4, help="acts (reuse: pairs of acts) per repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(PROFILES, "exp_puct_step_pieces.json"))
    args = ap.parse_args()
    if args.kernels:
        if not args.parent:
            ap.error("--kernels needs --parent")
        if args.work:
            os.makedirs(args.work, exist_ok=True)
            return kernels(args.parent, args.work)
        with tempfile.TemporaryDirectory() as work:
            return kernels(args.parent, work)
    if args.worker:
        return worker(args)
    if not args.parent_lib:
        ap.error("the comparison needs --parent-lib")
    return launches(args)


if __name__ == "__main__":
    sys.exit(main())
