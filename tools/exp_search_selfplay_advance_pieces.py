"""Developer tool: the advance kernels of per-row search self-play, built from the shared pieces of
csrc/mnk_search_selfplay_advance.h, against the parent commit's copies: the same resources, and the same time.

``--kernels --parent DIR`` (needs no GPU; DIR: the csrc directory of a checkout of the parent commit): the three
mnk_search_selfplay_async*.hip units of both trees compiled to gfx950 assembly with the compiler's resource report
(tools/exp_puct_fpu.py's ``compile_units``), and every kernel beside the parent's of the same name -- the parent's
``k_.._opts_fpu<.., S>`` is ``k_.._opts<.., S, true>`` now, its ``k_.._opts<.., S>`` is ``<.., S, false>``, and the same
for keep: static LDS, scratch, VGPR spills and waves per SIMD are gates, instruction counts are reported.  Writes
profiles/exp_search_selfplay_advance_pieces_kernels.md.

``--parent-lib PATH`` (the GPU): us per launch, device events around every launch in the busy stream with the trivial
evaluator, of the five kernel bodies -- plain, opts (noise and the solver on), keep, leaves (L = 4), gumbel -- on the shapes
of tools/exp_search_selfplay_async.py at I = 256, fast 32, ``full_prob`` 0.25, of this build against the parent's library
in fresh processes that alternate (tools/exp_search_selfplay_async_opts.py's harness).  The bar for every body and shape:
this build's mean is no higher than the parent's maximum over its repetitions.  Writes
profiles/exp_search_selfplay_advance_pieces.json.

usage: python tools/exp_search_selfplay_advance_pieces.py --kernels --parent DIR [--work DIR]
       python tools/exp_search_selfplay_advance_pieces.py --parent-lib PATH [--processes 2] [--reps 5]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
UNITS = ("mnk_search_selfplay_async", "mnk_search_selfplay_async_leaves", "mnk_search_selfplay_async_gumbel")
PROFILES = os.path.join(ROOT, "profiles")
# body: (the entry point the player calls, the player's options)
BODIES = {"plain": ("mnk_search_selfplay_advance", {}),
          "opts": ("mnk_search_selfplay_advance_opts", {"root_noise": None, "solver": True}),  # (root_noise: the shape's)
          "keep": ("mnk_search_selfplay_advance_keep", {"keep_tree": True}),
          "leaves": ("mnk_search_selfplay_advance_leaves", {"leaves": 4}),
          "gumbel": ("mnk_search_selfplay_advance_gumbel", {"gumbel": 16})}
GROWTH_LOOKED_AT = 0.023  # the largest growth the first-play-urgency change was accepted with on these kernels


# ----------------------------------------------------------------------------- the kernels (no GPU)
def now_name(parent_name):
    """the name a kernel of the parent has now"""
    m = re.match(r"(k_search_selfplay_advance_(?:opts|keep))(_fpu)?<(.*)>$", parent_name)
    return f"{m.group(1)}<{m.group(3)}, {'true' if m.group(2) else 'false'}>" if m else parent_name


def kernels(parent, work):
    import exp_puct_fpu as fpu

    fpu.UNITS = UNITS
    fpu.compile_units(os.path.join(ROOT, "rl-selfplay-mnk_amd", "csrc"), work, "new")
    fpu.compile_units(parent, work, "parent")
    rows, bad = [], []
    for unit in UNITS:
        ra, rb = (fpu.resources(os.path.join(work, f"{tag}_{unit}.res")) for tag in ("parent", "new"))
        aa, ab = (fpu.bodies(os.path.join(work, f"{tag}_{unit}.s")) for tag in ("parent", "new"))
        da, db = fpu.demangled(list(ra)), fpu.demangled(list(rb))
        by_name = {v: k for k, v in db.items()}
        assert len(da) == len(db) and sorted(now_name(v) for v in da.values()) == sorted(by_name), unit
        for mangled, name in da.items():
            other = by_name[now_name(name)]
            p, q, x, y = ra[mangled], rb[other], len(aa[mangled]), len(ab[other])
            gates = (q["LDS Size"] == p["LDS Size"] and q["ScratchSize"] == 0 and q["VGPRs Spill"] == 0
                     and q["Occupancy"] >= p["Occupancy"])
            rows.append((unit, now_name(name), p, q, x, y, gates))
            if not gates:
                bad.append(now_name(name))
    grown = [r for r in rows if r[5] > r[4] * (1 + GROWTH_LOOKED_AT)]
    lines = ["# The advance kernels from shared pieces: resources against the parent's copies", "",
             "Taken without a GPU by `python tools/exp_search_selfplay_advance_pieces.py --kernels --parent <parent csrc>`:",
             "the three units compiled to gfx950 assembly with `-O3 -ffp-contract=off -S",
             "-Rpass-analysis=kernel-resource-usage`; registers, scratch, LDS and waves per SIMD from the compiler's resource",
             "report, instructions counted in the assembly.  The gates: the parent's static LDS, scratch 0, no VGPR spill, no",
             "fewer waves per SIMD.", "",
             f"{len(rows)} kernels; {len(rows) - len(bad)} pass every gate"
             + (f"; FAILING: {', '.join('`' + b + '`' for b in bad)}" if bad else "") + ".",
             f"Instructions, all kernels: {sum(r[4] for r in rows)} in the parent, {sum(r[5] for r in rows)} now "
             f"({100.0 * (sum(r[5] for r in rows) / sum(r[4] for r in rows) - 1):+.2f} %); "
             f"{len(grown)} kernels grew by more than {100 * GROWTH_LOOKED_AT:.1f} %.", "",
             "| kernel | waves/SIMD parent / now | VGPRs parent / now | SGPRs parent / now | LDS B parent / now | scratch now | "
             "VGPR spills now | instructions parent / now | change |",
             "|---|---|---|---|---|---|---|---|---|"]
    for unit, name, p, q, x, y, gates in rows:
        lines.append(f"| `{name}` | {p['Occupancy']} / {q['Occupancy']} | {p['VGPRs']} / {q['VGPRs']} | "
                     f"{p['TotalSGPRs']} / {q['TotalSGPRs']} | {p['LDS Size']} / {q['LDS Size']} | {q['ScratchSize']} | "
                     f"{q['VGPRs Spill']} | {x} / {y} | {100.0 * (y / x - 1):+.1f} %{'' if gates else ' GATE'} |")
    text = "\n".join(lines) + "\n"
    notes = os.path.join(PROFILES, "exp_search_selfplay_advance_pieces_kernels_notes.md")
    if os.path.exists(notes):  # (what a person wrote about the kernels that grew: kept beside the table, appended to it)
        text += "\n" + open(notes).read()
    with open(os.path.join(PROFILES, "exp_search_selfplay_advance_pieces_kernels.md"), "w") as f:
        f.write(text)
    print(text)
    return 1 if bad else 0


# ----------------------------------------------------------------------------- the launches (the GPU)
def worker(args):
    """(a fresh process per build: the library is loaded once) one JSON line {body: {board: [us per launch, ...]}}"""
    import exp_search_selfplay_async_opts as opts

    out = {}
    for body, (entry_point, options) in BODIES.items():
        out[body] = {}
        for shape in opts.SHAPES:
            kw = dict(options)
            if "root_noise" in kw:
                kw["root_noise"] = opts.NOISE[opts.name_of(shape)]
            sp = opts.player(shape, "trivial", **kw)
            out[body][opts.name_of(shape)] = opts.launch_us(sp, entry_point, args.warmup, args.rounds, args.reps)
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
                                   "--rounds", str(args.rounds), "--reps", str(args.reps)], env=env, check=True,
                                  capture_output=True, text=True, timeout=600)
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            for body, boards in json.loads(line[7:]).items():
                for board, us in boards.items():
                    runs[build].setdefault((body, board), []).extend(us)
    rows = []
    for (body, board), us in runs["this"].items():
        this, par = opts.spread(us), opts.spread(runs["parent"][(body, board)])
        row = {"body": body, "entry_point": BODIES[body][0], "options": BODIES[body][1], "board": board,
               "iterations": opts.I, "fast_iterations": opts.FAST, "full_prob": opts.FULL_PROB,
               "launches_per_repetition": args.rounds, "this_us_per_launch": this, "parent_us_per_launch": par,
               "this_mean_no_higher_than_parent_max": this["mean"] <= par["max"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
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
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=400, help="launches per repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(PROFILES, "exp_search_selfplay_advance_pieces.json"))
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
