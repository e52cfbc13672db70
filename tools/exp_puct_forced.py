"""Developer tool: what forced playouts and policy target pruning (PUCTSearchPolicy(forced=k)) cost per step, and what
they do to the policy target under root noise.

``--cost``: on 9x9x5 x 1 024 and 19x19x5 x 256 rows of random mid-game positions with the conv net of tools/exp_puct.py,
``act`` at I = 256 with L = 1 and 4 and ``root_noise=(0.3, 0.25)``, without and with ``forced=2``, in ONE process: every
policy is built and warmed up first, then ``--reps`` passes over the policies in turn, device events around every step
launch in the busy stream (the evaluator's kernels run between them) and around the act.  Reported: the median step launch
of the plain policy (``mnk_puct_step`` / ``mnk_puct_step_leaves``) and of the forced one (``mnk_puct_step_forced``), their
difference, the difference as a share of one iteration (evaluator + step) of the same run, and the ``last`` step -- the
move, which holds the pruning -- on its own.  The two policies search different trees: the difference holds the forced test
AND whatever the other tree's shape costs.

``--targets``: 9x9x5 x 256 rows, I = 64, ``root_noise=(0.3, 0.25)``, the heuristic evaluator of tests/test_gpu_puct.py: the
policy target of plain PUCT, of forced playouts without pruning (``raw_visits``) and with it (``visits``) -- per root the
number of cells with a non-zero target, and the share of the target's mass on cells that plain PUCT WITHOUT noise never
visits from the same position.  It says nothing about strength or training.

``--kernels [--parent DIR]``: needs no GPU.  Compiles mnk_puct.hip and the three mnk_search_selfplay_async*.hip units (the
two that changed, and the two others that include mnk_puct_tree.h) to gfx950 assembly with the compiler's resource report
(``-S -Rpass-analysis=kernel-resource-usage``, the flags of ``__graft_entry__.build_hip``) and writes
profiles/exp_puct_forced_kernels.md: VGPRs, scratch and LDS of every new instantiation beside its sibling's and, with
``--parent`` (the csrc directory of a checkout of the parent commit), which existing kernels' instructions differ from the
parent's (compared line by line, block labels renumbered).  k_puct_step_leaves and k_search_selfplay_advance_opts gained a
template flag, FORCED, so the parent's ``k<.., SOLVER, FPU>`` is held against ``k<.., SOLVER, FPU, false>``.

usage: python tools/exp_puct_forced.py [--cost] [--targets] [--reps 5] [--out profiles/exp_puct_forced.json]
       python tools/exp_puct_forced.py --kernels [--parent DIR] [--work DIR]"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from exp_puct_fpu import CSRC, UNITS, bodies, compile_units, demangled, resources  # noqa: E402

SHAPES = (("9x9x5 x 1024", 9, 9, 5, 1024), ("19x19x5 x 256", 19, 19, 5, 256))
LEAVES, I, FORCED, NOISE = (1, 4), 256, 2.0, (0.3, 0.25)
STEPS = ("mnk_puct_step", "mnk_puct_step_leaves", "mnk_puct_step_forced")
FLAGGED = ("k_puct_step_leaves", "k_search_selfplay_advance_opts")  # the kernels with the new template flag, the last one


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
    keys = [(L, f) for L in LEAVES for f in (None, FORCED)]
    pols = {key: PUCTSearchPolicy(k, evaluator=ev, iterations=I, seed=1, leaves=key[0], root_noise=NOISE, forced=key[1])
            for key in keys}
    for pol in pols.values():  # warm-up: every batch shape, the buffers
        for _ in range(2):
            pol.act(obs)
    torch.cuda.synchronize()
    step_us, last_us, act_us = ({key: [] for key in keys} for _ in range(3))
    for _ in range(reps):
        for key, pol in pols.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with LaunchEvents(STEPS) as events:
                e0.record()
                pol.act(obs)
                e1.record()
            (launches,) = events.us().values()  # (a policy calls one step entry point)
            step_us[key] += launches[1:-1]  # (without the root's backup and the move)
            last_us[key].append(launches[-1])
            act_us[key].append(e0.elapsed_time(e1) * 1e3)
    out = []
    for L in LEAVES:
        plain, forced = (L, None), (L, FORCED)
        p, f = statistics.median(step_us[plain]), statistics.median(step_us[forced])
        lp, lf = statistics.median(last_us[plain]), statistics.median(last_us[forced])
        iteration = statistics.median(act_us[plain]) / (I // L + 1)
        out.append({"shape": name, "iterations": I, "leaves": L, "step_us_plain": round(p, 2), "step_us_forced": round(f, 2),
                    "step_us_more": round(f - p, 2), "iteration_us_plain": round(iteration, 1),
                    "more_as_share_of_iteration": round((f - p) / iteration, 4), "last_step_us_plain": round(lp, 2),
                    "last_step_us_forced": round(lf, 2), "last_step_us_more": round(lf - lp, 2),
                    "act_us_plain": round(statistics.median(act_us[plain]), 1),
                    "act_us_forced": round(statistics.median(act_us[forced]), 1)})
    return out


# ----------------------------------------------------------------------------- the targets
def targets():
    import numpy as np
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions
    from test_gpu_puct import heuristic_evaluator

    m, n, k, rows, iters = 9, 9, 5, 256, 64
    obs_np = random_positions(m, n, k, rows, np.random.default_rng(9), max_fill=0.3)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}

    def act(**kw):
        pol = PUCTSearchPolicy(k, evaluator=heuristic_evaluator(k), iterations=iters, seed=3, **kw)
        visits = torch.zeros((rows, m * n), dtype=torch.int32, device="cuda:0")
        raw = torch.zeros_like(visits) if "forced" in kw else None
        pol.act(obs, visits=visits, **({"raw_visits": raw} if raw is not None else {}))
        return visits.cpu().double(), None if raw is None else raw.cpu().double()

    quiet, _ = act()  # plain PUCT without noise: the cells it never visits
    plain, _ = act(root_noise=NOISE)
    pruned, raw = act(root_noise=NOISE, forced=FORCED)
    never = quiet == 0
    out = []
    for name, v in (("plain", plain), ("forced, no pruning (raw_visits)", raw), ("forced, pruned (visits)", pruned)):
        mass = v.sum(dim=1).clamp(min=1)
        out.append({"board": "9x9x5", "rows": rows, "iterations": iters, "root_noise": list(NOISE), "target": name,
                    "cells_with_a_target_mean": round((v > 0).sum(dim=1).double().mean().item(), 2),
                    "cells_with_a_target_median": (v > 0).sum(dim=1).double().median().item(),
                    "visits_in_the_target_mean": round(v.sum(dim=1).mean().item(), 2),
                    "share_of_mass_on_cells_plain_puct_without_noise_never_visits_mean":
                        round(((v * never).sum(dim=1) / mass).mean().item(), 4)})
    return out


# ----------------------------------------------------------------------------- the kernels (no GPU)
def plain_args(plain):
    return re.search(r"<(.*)>", plain).group(1).split(", ")


def kernels(parent, work, out_path):
    compile_units(CSRC, work, "new")
    if parent:
        compile_units(parent, work, "parent")
    lines = ["# Forced playouts: registers of the new kernels, and what became of the existing ones", "",
             "Taken without a GPU by `python tools/exp_puct_forced.py --kernels --parent <parent csrc>`: the units compiled",
             "to gfx950 assembly with `-O3 -ffp-contract=off -S -Rpass-analysis=kernel-resource-usage`; registers, scratch",
             "and LDS from the compiler's resource report, instructions counted in the assembly.", "",
             "## The new instantiations beside their siblings (FORCED = false)", "",
             "| kernel | VGPRs | sibling's VGPRs | instructions | sibling's | LDS B | scratch B/lane | VGPR spills | SGPRs "
             "kept in VGPR lanes, sibling's |",
             "|---|---|---|---|---|---|---|---|---|"]
    scratch = []
    for unit in UNITS[:2]:
        res, asm = resources(os.path.join(work, f"new_{unit}.res")), bodies(os.path.join(work, f"new_{unit}.s"))
        dm = demangled(list(res))
        by_name = {v: k for k, v in dm.items()}
        for mangled, plain in dm.items():
            if plain.split("<")[0] not in FLAGGED or plain_args(plain)[-1] != "true":
                continue
            sib = plain.split("<")[0] + "<" + ", ".join(plain_args(plain)[:-1]) + ", false>"
            r, s = res[mangled], res[by_name[sib]]
            scratch.append(r["ScratchSize"])
            lines.append(f"| `{plain}` | {r['VGPRs']} | {s['VGPRs']} | {len(asm[mangled])} | {len(asm[by_name[sib]])} | "
                         f"{r['LDS Size']} | {r['ScratchSize']} | {r['VGPRs Spill']} | {r['SGPRs Spill']}, {s['SGPRs Spill']} |")
    lines += ["", f"New instantiations: {len(scratch)}; with scratch: {sum(1 for x in scratch if x)}."]
    if parent:
        lines += ["", "## The existing kernels against the parent's", "",
                  "| unit | kernels in the parent | identical | differ | instructions of those, parent / now | same VGPRs | new kernels |",
                  "|---|---|---|---|---|---|---|"]
        moved = []
        for unit in UNITS:
            a, b = bodies(os.path.join(work, f"parent_{unit}.s")), bodies(os.path.join(work, f"new_{unit}.s"))
            ra, rb = resources(os.path.join(work, f"parent_{unit}.res")), resources(os.path.join(work, f"new_{unit}.res"))
            da, db = demangled(list(a)), demangled(list(b))
            by_name = {v: k for k, v in db.items()}
            # the parent's kernel under its name now: the same, or with the new flag off
            now = {k: k if k in b else by_name.get(da[k][:-1] + ", false>") for k in a}
            assert all(now.values()), [da[k] for k in a if not now[k]]
            differ = [k for k in a if a[k] != b[now[k]]]
            lines.append(f"| {unit}.hip | {len(a)} | {len(a) - len(differ)} | {len(differ)} | "
                         f"{sum(len(a[k]) for k in differ)} / {sum(len(b[now[k]]) for k in differ)} | "
                         f"{sum(1 for k in a if ra[k]['VGPRs'] == rb[now[k]]['VGPRs'])} of {len(a)} | "
                         f"{len(b) - len(set(now.values()))} |")
            moved += [(da[k], len(a[k]), len(b[now[k]]), ra[k]["VGPRs"], rb[now[k]]["VGPRs"], rb[now[k]]["ScratchSize"])
                      for k in differ]
        if moved:
            lines += ["", "| kernel whose instructions differ | instructions parent / now | VGPRs parent / now | scratch now |",
                      "|---|---|---|---|"]
            lines += [f"| `{name}` | {x} / {y} | {va} / {vb} | {sc} |" for name, x, y, va, vb, sc in moved]
        else:
            lines += ["", "No existing kernel's instructions differ from the parent's."]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct_forced.json"))
    for name in ("cost", "targets", "kernels"):
        ap.add_argument("--" + name, action="store_true")
    ap.add_argument("--parent", help="--kernels: the csrc directory of a checkout of the parent commit")
    ap.add_argument("--work", help="--kernels: where the assembly goes (default: a temporary directory)")
    args = ap.parse_args()
    if args.kernels:
        md = os.path.join(ROOT, "profiles", "exp_puct_forced_kernels.md")
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
    every = not (args.cost or args.targets)
    if args.cost or every:
        data["cost"] = [row for shape in SHAPES for row in cost(shape, args.reps)]
    if args.targets or every:
        data["targets"] = targets()
    for part in ("cost", "targets"):
        for row in data.get(part, ()):
            print(part, json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
