"""Writes tests/golden/puct_rules_parent.npz: what the numpy rules of the PUCT player (tests/puct_*_rule.py and the per-row
tests/search_selfplay_async_*_rule.py) answered BEFORE they were restated as one search with options
(tests/puct_search_rule.py).  The file was produced once, with the tests/ directory of the commit before that restatement
first on the path, and is not to be written again from a later tree: tests/test_puct_rules_pinned_cpu.py recomputes every
entry with the rules as they stand and holds it against the file, array for array.

The rules are imported by the names they had then -- LeavesPuct, ReusePuct, SolverPuct, FpuPuct, ForcedPuct, puct_leaves,
puct_solver, the cases modules' references -- so that this file runs unchanged on either tree.

An entry is a search (or, for the reuse forms, one act of a sequence; for the per-row forms, a whole run) and holds
``actions``, ``visits``, ``root_value`` and, where the form has them, ``carried``, ``proof`` and ``raw_visits``, and
``leaves``: the SHA-256 of the (leaf_obs, leaf_mask) batches the evaluator saw, in order, which pins the selections.  A
per-row run holds the SHA-256 of every round's leaf batch, its statistics and ring and, where the rule records them, its
``plies``.  An entry's arrays are named "<group>/<case>/<field>" (``unpack``).

What it covers: every reference of tests/puct_leaves_cases.py, puct_solver_cases.py, puct_forced_cases.py and
near_tie_cases.py over the grids their GPU tests use; both sides of the comparisons of tests/test_puct_solver_cpu.py,
test_puct_fpu_cpu.py and test_puct_forced_cpu.py that hold a class against the class it was built on, on their inputs; and
the whole cross solver x fpu x forced x L in {1, 2, 4} x temperature on 3x3x3 and 4x4x3 at I = 16 over three acts of a kept
tree, the last one deterministic.

usage: python tests/golden/make_golden_puct_rules.py [--tests DIR]   (from the repository root; needs no GPU; DIR: the
tests/ directory whose rules are to be recorded, by default this tree's)"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "puct_rules_parent.npz")
if __name__ == "__main__":
    TESTS = os.path.abspath(sys.argv[2]) if sys.argv[1:2] == ["--tests"] else os.path.dirname(HERE)
    sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import near_tie_cases as nt  # noqa: E402
import puct_forced_cases as fc  # noqa: E402
import puct_leaves_cases as lc  # noqa: E402
import puct_solver_cases as sc  # noqa: E402
import search_selfplay_async_fpu_cases as afc  # noqa: E402
import search_selfplay_async_keep_cases as akc  # noqa: E402
from puct_forced_rule import ForcedPuct  # noqa: E402
from puct_fpu_rule import FpuPuct  # noqa: E402
from puct_reuse_rule import ReusePuct  # noqa: E402
from puct_rule import puct  # noqa: E402
from puct_solver_rule import SolverPuct, puct_solver  # noqa: E402
from tactical_rule import random_positions  # noqa: E402

try:
    from puct_reuse_cases import advance, exact_np, start  # noqa: E402
except ImportError:  # (the tree before the restatement kept them in a GPU test)
    from test_gpu_puct_reuse import advance, exact_np, start  # noqa: E402

FIELDS = ("actions", "visits", "root_value", "carried", "proof")


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def leaves_sha(leaves):
    return sha(x for lo, lm in leaves for x in (np.asarray(lo, np.float32), np.asarray(lm, bool)))


def act(out, leaves, raw=None, **more):
    """the fields of one act: ``out`` is (actions, visits, root_value[, carried[, proof]])"""
    entry = dict(zip(FIELDS, (np.asarray(x) for x in out)), leaves=leaves_sha(leaves), **more)
    if raw is not None:
        entry["raw_visits"] = np.asarray(raw)
    return entry


def run_state(rule, **more):
    """the fields of a per-row run: the rule at its end"""
    entry = dict(stats=rule.stats.copy(), row_plies=rule.row_plies.copy(), records=np.array([rule.fast_records, rule.full_records]),
                 ring=sha([rule.ring_planes, rule.ring_visits, rule.ring_z]), **more)
    if hasattr(rule, "plies"):  # (row, ply, full, forces, root, n', the counts played from, the move) per ply
        entry["plies"] = np.array([(i, p, full, forces, move) for i, p, full, forces, _, _, _, move in rule.plies], np.int64)
        entry["plies_boards"] = sha(x for rec in rule.plies for x in (rec[4], np.asarray(rec[5], np.int64), np.asarray(rec[6], np.int64)))
    if hasattr(rule, "carried"):
        entry["carried"] = rule.carried.copy()
    return entry


# ----------------------------------------------------------------------------- the cases modules
def leaves_entries():
    for name, L in lc.PARAMS:
        _, out, seen, trace = lc.reference(name, L)
        yield f"leaves/{name}-{L}", act(out, seen, trace=np.array([[t["void"], t["shared"], t["repeat"], t["live"]] for t in trace]))


def solver_entries():
    for name in sc.CASES:
        for L in sc.LEAVES:
            for t in (0, 1):
                _, out, seen = sc.reference(name, L, t)
                yield f"solver/{name}-{L}-{t}", act(out, seen)
    for solver in (True, False):
        seen = []  # (``misled_reference(solver)`` with the leaves)
        rule = SolverPuct(sc.MISLED_BOARD[2], sc.MISLED_I, sc.C_PUCT, sc.misled_np, 1, seed=sc.SEED, solver=solver, leaves=seen)
        yield f"solver/misled-{solver}", act(rule.act(sc.MISLED_OBS, deterministic=True), seen)
    for case in range(len(sc.REUSE_CASES)):
        for distance in (1, 2):
            plies, decided = sc.reuse_reference(case, distance)
            for ply, (_, out, seen) in enumerate(plies):
                yield f"solver/reuse-{case}-{distance}-{ply}", act(out, seen, decided=np.array(decided))


def forced_async_run(case):
    """``puct_forced_cases.async_run(case)`` round by round: (the rule at the end, the SHA-256 of every round's leaves)"""
    rule, _, ev = fc.new_async_rule(case)
    obs, mask = rule.view()
    rounds = []
    for _ in range(fc.ASYNC_CASES[case][3]):
        obs, mask, _ = rule.advance(*ev(obs, mask))
        rounds.append(leaves_sha([(obs, mask)]))
    return rule, np.stack(rounds)


def forced_entries():
    tag = lambda fpu: "n" if fpu is None else "f"  # noqa: E731
    for name in fc.BOARDS:
        for L, solver, fpu, t in fc.OPTIONS:
            _, out, seen, rule = fc.reference(name, L, solver, fpu, t)
            yield f"forced/{name}-{L}-{solver}-{tag(fpu)}-{t}", act(out, seen, rule.raw_visits)
    for L, solver, fpu in [(1, False, None), (4, False, None), (4, True, None), (4, True, fc.FPU)]:
        _, out, seen, _ = fc.reference("9x9x5", L, solver, fpu, 0, None)
        yield f"forced/off-9x9x5-{L}-{solver}-{tag(fpu)}", act(out, seen)
    for L, fpu in fc.LOSS_OPTIONS:
        _, out, seen, rule = fc.loss_reference(L, fpu)
        yield f"forced/loss-{L}-{tag(fpu)}", act(out, seen, rule.raw_visits)
    for which in fc.EDGES:
        for L in (1, 4):
            _, out, seen, rule = fc.edge_reference(which, L)
            yield f"forced/edge-{which}-{L}", act(out, seen, rule.raw_visits)
    for name in fc.FLOOR_NAMES:
        _, out, seen, rule = fc.floor_reference(name)
        yield f"forced/floor-{name}", act(out, seen, rule.raw_visits)
    for L, solver in fc.REUSE:
        for ply, (_, out, seen, raw, n0) in enumerate(fc.reuse_reference(L, solver)):
            yield f"forced/reuse-{L}-{solver}-{ply}", act(out, seen, raw, n0=np.array(n0))
    for case in range(len(fc.ASYNC_CASES)):
        rule, rounds = forced_async_run(case)
        yield f"forced/async-{case}", run_state(rule, rounds=rounds)


def near_tie_entries():
    cases = [(name, form, None) for name, form in nt.LOCKSTEP]
    cases += [(name, form, table) for name, form in nt.SECOND for table in nt.tables_of(name, form)[1:]]
    for name, form, table in cases:
        for ply, a in enumerate(nt.reference(name, form, table)):
            more = {} if a["policy"] is None else dict(policy=a["policy"], gscore=a["gscore"])
            yield f"near_tie/{name}-{form}-{table}-{ply}", act(a["out"], a["leaves"], a["raw"], **more)
    for name, form in nt.ASYNC:
        rule, trace = nt.async_run(name, form)
        yield f"near_tie/async-{name}-{form}", run_state(rule, rounds=np.stack([sha([obs]) for obs in trace]))


def per_row_entries():
    """the per-row runs of the first-play urgency and kept-tree cases (their GPU tests follow these launch for launch)"""
    for case in range(len(afc.CASES)):
        yield f"async_fpu/{case}", run_state(afc.mixed_run(case))
    for case in range(len(akc.MIXED)):
        yield f"async_keep/{case}", run_state(akc.mixed_run(case))


# ----------------------------------------------------------------------------- a class against the class it was built on
def built_on_entries():
    """both sides of the comparisons that the restatement turns into a class compared with itself"""
    # tests/test_puct_solver_cpu.py: SolverPuct(solver=False) against LeavesPuct (the other side: "leaves/<name>-<L>"),
    # against puct() and against ReusePuct
    for name, L in [("3x3x3", 1), ("3x3x3", 4), ("4x6x3", 2), ("4x6x3", 16), ("9x9x5", 1), ("9x9x5", 8), ("19x19x5", 4),
                    ("round", 8)]:
        (m, n, k), _, I, _ = lc.CASES[name]
        seen = []
        out = SolverPuct(k, I, 1.25, exact_np(m * n), L, seed=43, env_id0=7, leaves=seen, solver=False).act(lc.positions(name), step=2)
        yield f"built_on/solver_off-{name}-{L}", act(out, seen)
    m, n, k, I = 4, 6, 3, 24
    for t in (0, 1):
        obs = random_positions(m, n, k, 10, np.random.default_rng(5), max_fill=0.7)
        seen = []
        out = puct(obs, k, I, 1.25, exact_np(m * n), seed=5, step=3, env_id0=2, temperature=t, leaves=seen)
        yield f"built_on/first_rule-{t}", act(out, seen)
        seen = []
        out = puct_solver(obs, k, I, 1.25, exact_np(m * n), 1, seed=5, step=3, env_id0=2, temperature=t, solver=False, leaves=seen)
        yield f"built_on/solver_off_one_leaf-{t}", act(out[:3], seen, proof=out[3])
    for (m, n, k), rows, J, distance in [((3, 3, 3), 6, 10, 1), ((4, 6, 3), 5, 12, 2)]:
        for side in ("reuse", "solver_off"):
            seen = []
            rule = (ReusePuct(k, J, 1.25, exact_np(m * n), None, 41, 5, leaves=seen) if side == "reuse" else
                    SolverPuct(k, J, 1.25, exact_np(m * n), 1, reuse=True, seed=41, env_id0=5, solver=False, leaves=seen))
            obs, resets = start(m, n, k, rows, m * 100 + n * 10 + k + distance), np.zeros(rows, np.int64)
            for ply in range(8):
                del seen[:]
                out = rule.act(obs, step=ply)
                yield f"built_on/kept-{side}-{m}x{n}x{k}-{ply}", act(out, seen)
                obs = advance(obs, out[0], k, distance, resets)
    # tests/test_puct_fpu_cpu.py: FpuPuct(fpu=None) against SolverPuct
    for name, L, solver in [("3x3x3", 1, True), ("5x5x4", 4, False), ("9x9x5", 4, True)]:
        (m, n, k), _, I = sc.CASES[name]
        for side, cls in (("solver", SolverPuct), ("fpu_none", FpuPuct)):
            seen = []
            out = cls(k, I, sc.C_PUCT, exact_np(m * n), L, seed=sc.SEED, env_id0=sc.ENV_ID0, leaves=seen, solver=solver).act(sc.positions(name), step=2)
            yield f"built_on/{side}-{name}-{L}-{solver}", act(out, seen)
    # tests/test_puct_forced_cpu.py: ForcedPuct(forced=None) against FpuPuct
    for name, L, solver, fpu in [("3x3x3", 1, True, None), ("5x5x4", 4, False, fc.FPU), ("9x9x5", 4, True, fc.FPU)]:
        (m, n, k), I, _, _ = fc.BOARDS[name]
        for side in ("fpu", "forced_none"):
            seen = []
            rule = (FpuPuct(k, I, fc.C_PUCT, fc.evaluator_of(name), L, seed=fc.SEED, env_id0=fc.ENV_ID0, leaves=seen, solver=solver,
                            fpu=fpu) if side == "fpu" else fc.new_rule(name, L, solver, fpu, forced=None, seen=seen))
            yield f"built_on/{side}-{name}-{L}-{solver}", act(rule.act(fc.rows_of(name), step=2), seen)


# ----------------------------------------------------------------------------- every combination of the options
def cross_entries():
    """3x3x3 and 4x4x3, I = 16, five rows: the smallest boards and budgets at which a walk reaches terminal nodes, fills a
    tree and carries a subtree.  Three acts of a kept tree, the last one deterministic"""
    for m, n, k in ((3, 3, 3), (4, 4, 3)):
        for solver in (False, True):
            for fpu in (None, (0.25, 0.5)):
                for forced in (None, 2.0):
                    for L in (1, 2, 4):
                        for t in (0, 1):
                            seen = []
                            rule = ForcedPuct(k, 16, 1.25, exact_np(m * n), L, reuse=True, seed=9, env_id0=3, temperature=t, leaves=seen,
                                              solver=solver, fpu=fpu, forced=forced)
                            obs, resets = start(m, n, k, 5, m * n + L), np.zeros(5, np.int64)
                            for ply in range(3):
                                del seen[:]
                                out = rule.act(obs, step=ply, deterministic=ply == 2)
                                raw = rule.raw_visits if forced is not None else None
                                key = f"cross/{m}x{n}x{k}-{solver}-{fpu is not None}-{forced is not None}-{L}-{t}-{ply}"
                                yield key, act(out, seen, raw)
                                obs = advance(obs, out[0], k, 1, resets)


GROUPS = (leaves_entries, solver_entries, forced_entries, near_tie_entries, per_row_entries, built_on_entries, cross_entries)


def entries():
    """{"<group>/<case>/<field>": array} of every entry, from the rules on the path"""
    out = {}
    for group in GROUPS:
        for key, entry in group():
            assert not any(f"{key}/{field}" in out for field in entry), key
            out.update({f"{key}/{field}": np.asarray(value) for field, value in entry.items()})
    return out


def pack(data):
    """the entries as few arrays (a zip member costs more than most of these arrays hold): per group and field, every
    entry's array flattened and joined, beside the entries' names and shapes"""
    columns = {}
    for key, value in data.items():
        group, case, field = key.split("/")
        columns.setdefault(f"{group}/{field}", []).append((case, value))
    out = {}
    for column, cells in columns.items():
        assert len({value.dtype for _, value in cells}) == 1 and all(value.ndim <= 2 for _, value in cells), column
        out[column] = np.concatenate([value.ravel() for _, value in cells])
        out[column + "/cases"] = np.array([case for case, _ in cells])
        out[column + "/shapes"] = np.array([value.shape + (-1,) * (2 - value.ndim) for _, value in cells], np.int64)
    return out


def unpack(packed):
    """``pack`` undone: {"<group>/<case>/<field>": array}"""
    out = {}
    for column in (name for name in packed if name.count("/") == 1):
        flat, at = packed[column], 0
        group, field = column.split("/")
        for case, shape in zip(packed[column + "/cases"], packed[column + "/shapes"]):
            shape = tuple(int(x) for x in shape if x >= 0)
            size = int(np.prod(shape, dtype=np.int64))
            out[f"{group}/{case}/{field}"] = flat[at:at + size].reshape(shape)
            at += size
        assert at == len(flat), column
    return out


if __name__ == "__main__":
    import puct_solver_rule

    data = entries()
    np.savez_compressed(OUT, **pack(data))
    with np.load(OUT) as z:
        again = unpack({name: z[name] for name in z.files})
    assert data.keys() == again.keys() and all(np.array_equal(data[key], again[key]) and data[key].dtype == again[key].dtype
                                               for key in data)
    print(f"{OUT}: {len(data)} arrays from {os.path.dirname(puct_solver_rule.__file__)}, {os.path.getsize(OUT)} bytes")
