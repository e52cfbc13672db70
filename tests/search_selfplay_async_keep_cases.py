"""The cases of per-row search self-play that keeps its trees, shared by tests/test_search_selfplay_async_keep_cpu.py (which
chooses and checks the seeds with the rule) and tests/test_gpu_search_selfplay_async_keep.py (which runs them on the
device).  No torch here: dtypes are named by strings."""
import functools
import os

import numpy as np

from search_selfplay_async_keep_rule import AsyncKeepRule
from search_selfplay_async_rule import exact_np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_selfplay_async_starts.npz")
FULL, FAST, THRESHOLD = 6, 2, 3 * 2 ** 30  # the mixed budgets: a ply is full with probability 3/4
ENV_ID0 = 3
NOISE = (0.3, 0.25)

# board, rows, leaf dtype, dtype of priors and values, device key word, temp_plies, rounds, start ("golden": a stored env
# state near the end of games), seed, root_noise, noise_on_fast, solver, tree_nodes (8: keep_nodes = 2, children are
# dropped on every carried ply), evaluator.  7x7x4 has no built-in variant (the generic form); 8x3x3 shares 3x3x3's.  On
# 19x19 six iterations under the dyadic evaluator never visit a child twice (an unvisited cell of prior 1 scores 3 at
# n = 6, above any value), so nothing but the child itself would ever be kept: that case searches under the peaked one.
MIXED = [
    ((3, 3, 3), 7, "float32", "float32", False, 2, 130, None, 6, NOISE, False, True, 13, "exact"),
    ((9, 9, 5), 5, "bfloat16", "float32", False, 6, 600, None, 6, NOISE, True, False, 8, "exact"),
    ((7, 7, 4), 5, "uint8", "float32", True, 4, 500, None, 6, None, False, True, 13, "exact"),
    ((8, 3, 3), 7, "float32", "bfloat16", False, 2, 300, None, 6, None, False, False, 8, "exact"),
    ((19, 19, 5), 3, "float32", "float32", False, 4, 150, "golden", 6, None, False, False, 13, "peaked"),
    ((16, 15, 5), 5, "float32", "float32", False, 4, 150, "golden", 6, None, False, True, 13, "exact"),
    # the solver under keep_nodes = 2: the child that proved a carried root is dropped by the truncation while an older
    # sibling stays, and the root then starts unknown (twice in this run; five roots keep their proof)
    ((3, 3, 3), 7, "float32", "float32", False, 2, 200, None, 6, None, False, True, 8, "exact"),
    # the generic forms of sixteen and of thirty-two words (ten and 21 words a plane), from a computed start
    ((17, 17, 5), 5, "uint8", "float32", False, 4, 150, "late", 6, None, False, True, 13, "peaked"),
    ((25, 25, 5), 5, "float32", "bfloat16", False, 4, 150, "late", 6, NOISE, False, False, 13, "peaked"),
]
TRUNCATED_SOLVER = 6  # the case of the comment above it


LATE_ROWS = 5  # the rows of a "late" start


def start_state(board, start):
    """None, a stored state ("golden") or a computed one ("late": ``late_start`` of
    tests/search_selfplay_async_fpu_cases.py, LATE_ROWS rows -- no fixture, so any board)"""
    if start is None:
        return None
    m, n, k = board
    if start == "late":
        from search_selfplay_async_fpu_cases import late_start  # (that module imports this one)

        return late_start(m, n, k, LATE_ROWS)
    with np.load(GOLDEN) as z:
        return z[f"{m}x{n}x{k}_planes"], z[f"{m}x{n}x{k}_meta"]


def new_rule(board, N, temp, seed, start, noise, on_fast, solver, tree_nodes, full=FULL, fast=FAST, threshold=THRESHOLD,
             T=None, env_id0=ENV_ID0, keep_tree=True):
    m, n, k = board
    rule = AsyncKeepRule(m, n, k, N, T or m * n, full, fast, threshold, 1.25, temp, seed, env_id0, root_noise=noise,
                         noise_on_fast=on_fast, solver=solver, keep_tree=keep_tree, tree_nodes=tree_nodes)
    state = start_state(board, start)
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule


@functools.lru_cache(maxsize=None)
def mixed_run(case):
    """the rule's run of MIXED[case] with its own noise: the rule at the end (its ``trace`` is what the conditions read)"""
    board, N, _, _, _, temp, rounds, start, seed, noise, on_fast, solver, tree_nodes, evaluator = MIXED[case]
    rule = new_rule(board, N, temp, seed, start, noise, on_fast, solver, tree_nodes)
    ev = EVALUATORS[evaluator](rule.C)
    obs, mask = rule.view()
    for _ in range(rounds):
        obs, mask, _ = rule.advance(*ev(obs, mask))
    return rule


def conditions(rule):
    """what a mixed case must show, from the rule's trace: (a carried ply with more than one node kept, a ply that
    started fresh after a game ended, a truncation, a carried root that kept the proof it had when carried)"""
    kept = [t for t in rule.trace if t[3] > 0]
    return (any(t[3] > 1 for t in kept), any(t[3] == 0 for t in rule.trace) and rule.stats[0] > 0,
            any(t[3] == t[6] for t in kept), any(t[7] != 0 for t in kept))


def dropped_proofs(rule):
    """the carried plies whose root was proven as a child and starts unknown although a child of its own was kept"""
    return sum(1 for t in rule.trace if t[5] and not t[7] and t[3] > 1)


# ----------------------------------------------------------------------------- the marking's chunk boundary
CHUNK_BOARD, CHUNK_N, CHUNK_I, CHUNK_NODES, CHUNK_PLIES, CHUNK_SEED, CHUNK_TEMP = (9, 9, 5), 3, 160, 321, 3, 3, 1


def peaked_table(C):
    """priors that are powers of two (exact in every format), each cell's half the one before it in the order a * 37 mod C,
    down to 2^-14: a search under them is narrow and deep"""
    return (2.0 ** -np.minimum((np.arange(C) * 37) % C, 14)).astype(np.float32)


def peaked_np(C):
    table = peaked_table(C)

    def evaluate(leaf_obs, leaf_mask):
        cnt = leaf_obs.astype(np.float32).reshape(len(leaf_obs), 2, -1).sum(axis=2)
        return leaf_mask.astype(np.float32) * table, ((np.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5) - 2) / 4).astype(np.float32)

    return evaluate


EVALUATORS = {"exact": exact_np, "peaked": peaked_np}


@functools.lru_cache(maxsize=None)
def chunk_run(seed=CHUNK_SEED):
    """every ply full: (rule at the end, [(leaf_obs, leaf_mask, fresh, carried) of every round])"""
    m, n, k = CHUNK_BOARD
    rule = AsyncKeepRule(m, n, k, CHUNK_N, m * n, CHUNK_I, CHUNK_I, 2 ** 32, 1.25, CHUNK_TEMP, seed, ENV_ID0,
                         keep_tree=True, tree_nodes=CHUNK_NODES)
    ev = peaked_np(rule.C)
    obs, mask = rule.view()
    out = []
    for _ in range(CHUNK_PLIES * (CHUNK_I + 1)):
        obs, mask, fresh = rule.advance(*ev(obs, mask))
        out.append((obs, mask, fresh, rule.carried.copy()))
    return rule, out
