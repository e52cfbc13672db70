"""The near-tie cases of the PUCT forms, shared by tests/test_near_tie_cpu.py (which shows with the rules alone that every
case notices each planted rounding defect it can) and tests/test_gpu_near_tie.py (which runs them on the device): the boards,
budgets and positions, the constants -- none of them dyadic --, the ``ulps`` and table seed of the evaluator
(tests/near_tie_evaluator.py) chosen per case, and the rules' answers, computed once per process.

A lockstep case is (board name, form).  The forms: "plain" (tests/puct_rule.py), "leaves" (puct_leaves_rule.py), "solver"
(puct_solver_rule.py), "fpu" (puct_fpu_rule.py), "forced" and "all" -- four leaves, the solver, first-play urgency, forced
playouts and root noise at once -- (puct_forced_rule.py), "reuse1" / "reuse2" (three plies of puct_reuse_rule.py with the next
root one or two plies on) and "gumbel" (puct_gumbel_rule.py).  The per-row cases are below them."""
import functools

import numpy as np

import puct_rule
from near_tie_evaluator import near_np
from puct_forced_rule import AsyncOptsForcedRule, ForcedPuct
from puct_fpu_rule import AsyncKeepFpuRule, AsyncOptsFpuRule, FpuPuct
from puct_gumbel_rule import gumbel_puct
from puct_leaves_rule import LeavesPuct
from puct_noise_rule import root_noise
from puct_reuse_rule import ReusePuct
from puct_solver_rule import PROOF_UNKNOWN, SolverPuct
from search_selfplay_async_gumbel_rule import AsyncGumbelRule
from search_selfplay_async_keep_rule import AsyncKeepRule
from search_selfplay_async_leaves_rule import AsyncLeavesRule
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_async_rule import AsyncSelfPlayRule
from tactical_rule import random_positions

C_PUCT, FPU, K_FORCED, NOISE = 1.1, (0.3, 0.45), 1.7, (0.3, 0.25)
SEED, ENV_ID0, STEP = 47, 5, 2
REUSE_PLIES, CONSIDERED = 3, 4
#        name       board        rows  I   ulps  table seed
BOARDS = {"3x3x3": ((3, 3, 3), 5, 32, 2, 0),       # one pass per lane, NW = 1, a partial workgroup
          "4x6x3": ((4, 6, 3), 5, 48, 2, 0),       # the generic form
          "9x9x5": ((9, 9, 5), 5, 48, 2, 0),       # C > 64: the arg-max crosses passes and lanes
          "19x19x5": ((19, 19, 5), 3, 16, 2, 0)}   # multi-word, six passes
# (name, form): (ulps, table seed) where the board's own choice lets a planted defect through (tests/test_near_tie_cpu.py
# says which; found there by its search over the seeds 0 .. 79 and ulps in {2, 4, 8})
CHOICE = {("3x3x3", "leaves"): (4, 0), ("3x3x3", "fpu"): (8, 0), ("3x3x3", "all"): (8, 1), ("3x3x3", "gumbel"): (2, 2),
          ("4x6x3", "fpu"): (8, 0), ("4x6x3", "all"): (4, 0), ("4x6x3", "gumbel"): (4, 0),
          ("19x19x5", "plain"): (8, 0), ("19x19x5", "leaves"): (4, 0), ("19x19x5", "solver"): (8, 0),
          ("19x19x5", "fpu"): (8, 0), ("19x19x5", "forced"): (8, 0), ("19x19x5", "reuse1"): (4, 0),
          ("19x19x5", "reuse2"): (4, 0), ("19x19x5", "gumbel"): (8, 0), ("19x19x5", "all"): (8, 12)}
# a second table for the case no single table of ulps 2, 4, 8 and seeds 0 .. 79 makes notice every defect: (8, 12) above
# shows the reassociated term, the f64 score, the reversed backups and the fused urgency, (4, 12) the low square root.  The
# case runs under both, on the CPU and on the device
SECOND = {("19x19x5", "all"): (4, 12)}
FORMS = ("plain", "leaves", "solver", "fpu", "forced", "all", "reuse1", "reuse2", "gumbel")
LOCKSTEP = [(name, form) for name in BOARDS for form in FORMS]


def leaves_of(name, form):
    return {"leaves": 16 if name == "9x9x5" else 4, "all": 4}.get(form, 1)


def choice(name, form):
    return CHOICE.get((name, form), BOARDS[name][3:])


def tables_of(name, form):
    """the (ulps, table seed) choices the case runs under: its own and, for one case, a second"""
    return [choice(name, form)] + ([SECOND[name, form]] if (name, form) in SECOND else [])


def rows_of(name):
    """an empty board, then positions up to three tenths full"""
    (m, n, k), rows, _, _, _ = BOARDS[name]
    obs = random_positions(m, n, k, rows, np.random.default_rng(sum(map(ord, name))), max_fill=0.3)
    obs[0] = 0
    return obs


def noised(evaluator, L, step=STEP, given=None):
    """the evaluator with root noise on the rows i * L of its first call: the rule's own (tests/puct_noise_rule.py), or
    ``given`` -- a kernel's, float32 [N * L, C]"""
    calls = [0]

    def evaluate(leaf_obs, leaf_mask):
        priors, values = evaluator(leaf_obs, leaf_mask)
        if calls[0] == 0:
            priors = priors.copy()
            priors[::L] = (root_noise(priors, leaf_mask, *NOISE, SEED, step, ENV_ID0, leaves=L) if given is None
                           else given[::L])
        calls[0] += 1
        return priors, values

    return evaluate


TODAY = (1.25, (0.25, 0.5), 2.0)  # c, fpu and forced of the older tests: every one dyadic


def run(name, form, evaluator=None, gscore=None, noise=None, today=False, L=None, table=None):
    """the rule of a lockstep case on its rows: a list, one entry per act (three for the reuse forms, else one), of
    dict(obs, out = (actions, visits, root_value, carried, proof), raw = n' or None, policy = the Gumbel root's improved
    policy or None, gscore, leaves = every evaluation's (leaf_obs, leaf_mask)).  ``evaluator``: instead of the case's own;
    ``gscore`` / ``noise``: a kernel's Gumbel scores / noised root priors to search with; ``today``: the dyadic evaluator
    of tests/puct_reuse_cases.py and the constants of the older tests in the place of the case's; ``L``: leaves per row
    other than the case's; ``table``: (ulps, table seed) other than the case's first"""
    (m, n, k), rows, I, _, _ = BOARDS[name]
    C, L = m * n, L or leaves_of(name, form)
    ev = evaluator or near_np(C, *(table or choice(name, form)))
    C_PUCT, FPU, K_FORCED = (globals()[x] for x in ("C_PUCT", "FPU", "K_FORCED"))
    if today:
        from puct_reuse_cases import exact_np

        ev, (C_PUCT, FPU, K_FORCED) = exact_np(C), TODAY
    obs, seen = rows_of(name), []
    kw = dict(seed=SEED, env_id0=ENV_ID0, leaves=seen)
    none = (np.zeros((rows, 2), np.int32), np.full(rows, PROOF_UNKNOWN, np.int8))

    def act(out, **more):
        return dict(obs=obs, out=tuple(out), raw=None, policy=None, gscore=None, leaves=list(seen), **more)

    if form == "plain":
        return [act(puct_rule.puct(obs, k, I, C_PUCT, ev, step=STEP, **kw) + none)]
    if form == "leaves":
        return [act(LeavesPuct(k, I, C_PUCT, ev, L, **kw).act(obs, step=STEP) + none[1:])]
    if form == "solver":
        return [act(SolverPuct(k, I, C_PUCT, ev, **kw).act(obs, step=STEP))]
    if form == "fpu":
        return [act(FpuPuct(k, I, C_PUCT, ev, fpu=FPU, **kw).act(obs, step=STEP))]
    if form in ("forced", "all"):
        if form == "all":
            ev = noised(ev, L, given=noise)
        rule = ForcedPuct(k, I, C_PUCT, ev, L, solver=form == "all", fpu=FPU if form == "all" else None, forced=K_FORCED, **kw)
        out = rule.act(obs, step=STEP)
        return [dict(act(out), raw=rule.raw_visits)]
    if form == "gumbel":
        a, visits, value, policy, gs = gumbel_puct(obs, k, I, C_PUCT, ev, CONSIDERED, step=STEP, gscore=gscore, **kw)
        return [dict(act((a, visits, value) + none), policy=policy, gscore=gs)]
    from puct_reuse_cases import advance

    distance = {"reuse1": 1, "reuse2": 2}[form]
    rule, acts, resets = ReusePuct(k, I, C_PUCT, ev, None, SEED, ENV_ID0, leaves=seen), [], np.zeros(rows, np.int64)
    for ply in range(REUSE_PLIES):
        del seen[:]
        out = rule.act(obs, step=ply)
        acts.append(act(out + none[1:]))
        obs = advance(obs, out[0], k, distance, resets)
    return acts


@functools.lru_cache(maxsize=None)
def reference(name, form, table=None):
    """``run`` of the case as it stands, computed once ("gumbel" and "all" with the rule's own scores and noise: the GPU
    test runs those two again on the kernel's)"""
    return run(name, form, table=table)


def differs(a, b):
    """whether two results of ``run`` differ in a row: visits, actions, root_value bits, n', or an evaluation's leaves"""
    for x, y in zip(a, b):
        if len(x["leaves"]) != len(y["leaves"]):
            return True
        if any(not (np.array_equal(lo, wo) and np.array_equal(lm, wm)) for (lo, lm), (wo, wm) in zip(x["leaves"], y["leaves"])):
            return True
        if any(not np.array_equal(np.asarray(g).view(np.uint32) if np.asarray(g).dtype == np.float32 else g,
                                  np.asarray(w).view(np.uint32) if np.asarray(w).dtype == np.float32 else w)
               for g, w in zip(x["out"], y["out"])):
            return True
        if x["raw"] is not None and not np.array_equal(x["raw"], y["raw"]):
            return True
    return False


# ----------------------------------------------------------------------------- the per-row cases
# one per advance kernel, on 3x3x3 and 9x9x5: five rows, mixed budgets (a ply is full with probability 3/4)
ASYNC_ROWS, ASYNC_FULL, ASYNC_FAST, ASYNC_THRESHOLD, ASYNC_TEMP, ASYNC_SEED = 5, 8, 4, 3 * 2 ** 30, 2, 6
#               kernel         the player's options
ASYNC_FORMS = {"advance": {},
               "opts": dict(root_noise=NOISE, solver=True),
               "keep": dict(keep_tree=True, tree_nodes=2 * ASYNC_FULL + 1),
               "leaves": dict(leaves=4),
               "gumbel": dict(gumbel=CONSIDERED),
               "opts_fpu": dict(solver=True, fpu=FPU),
               "keep_fpu": dict(keep_tree=True, tree_nodes=2 * ASYNC_FULL + 1, fpu=FPU),
               "opts_forced": dict(solver=True, fpu=FPU, forced=K_FORCED)}
#                board      rounds: enough for a game to end and for fast and full plies (tests/test_near_tie_cpu.py)
ASYNC_BOARDS = {"3x3x3": 80, "9x9x5": 200}
ASYNC = [(name, form) for name in ASYNC_BOARDS for form in ASYNC_FORMS]


def async_rounds(name, form):
    return ASYNC_BOARDS[name] // (2 if form == "leaves" else 1)


def async_start(name):
    """None (the empty board) on 3x3x3; on 9x9x5 the computed late start of the other per-row tests: rows a few stones
    short of a drawn board, so that games end within the run"""
    from search_selfplay_async_keep_cases import start_state

    return None if name == "3x3x3" else start_state(BOARDS[name][0], "late")


def new_async_rule(name, form):
    m, n, k = BOARDS[name][0]
    state = async_start(name)
    N = ASYNC_ROWS if state is None else len(state[1])
    args = (m, n, k, N, m * n, ASYNC_FULL, ASYNC_FAST, ASYNC_THRESHOLD, C_PUCT)
    if form == "gumbel":
        rule = AsyncGumbelRule(*args, ASYNC_SEED, CONSIDERED, env_id0=ENV_ID0)
    else:
        cls = {"advance": AsyncSelfPlayRule, "opts": AsyncOptsRule, "keep": AsyncKeepRule, "leaves": AsyncLeavesRule,
               "opts_fpu": AsyncOptsFpuRule, "keep_fpu": AsyncKeepFpuRule, "opts_forced": AsyncOptsForcedRule}[form]
        rule = cls(*args, ASYNC_TEMP, ASYNC_SEED, ENV_ID0, **ASYNC_FORMS[form])
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule


def async_evaluator(name, form):
    m, n, _ = BOARDS[name][0]
    return near_np(m * n, *BOARDS[name][3:])


@functools.lru_cache(maxsize=None)
def async_run(name, form):
    """the rule's run of a per-row case with its own noise and Gumbel scores: (the rule at the end, every round's leaf_obs)"""
    rule, ev = new_async_rule(name, form), async_evaluator(name, form)
    obs, mask = rule.view()
    trace = []
    for _ in range(async_rounds(name, form)):
        obs, mask, _ = rule.advance(*ev(obs, mask))
        trace.append(obs)
    return rule, trace
