"""The cases of the PUCT player with forced playouts and policy target pruning, shared by tests/test_puct_forced_cpu.py
(which checks with the rule alone that every case shows what it is there for), tests/test_gpu_puct_forced.py and
tests/test_gpu_search_selfplay_async_forced.py (which run them on the device): the evaluator, the boards, budgets and
positions of the lockstep cases with the rule's answer on each (tests/puct_forced_rule.py), computed once per process, and
the cases of the per-row loop.

The evaluator makes forcing matter at tiny budgets: a few "spike" cells carry a large dyadic prior, and a position in
which the opponent holds more spike cells than the side to move is valued as lost for the one who took them.  Plain PUCT
visits a spike once, finds it bad and leaves it; forced playouts return to it, and the pruning takes those visits out."""
import functools

import numpy as np

from oracle.packing import unpack_boards
from puct_forced_rule import AsyncOptsForcedRule, ForcedPuct
from puct_solver_cases import C_PUCT, ENV_ID0, SEED
from search_selfplay_async_fpu_cases import FAINT, NOISE
from search_selfplay_async_keep_cases import FAST, FULL, THRESHOLD, start_state
from tactical_rule import random_positions

K_FORCED = 2.0  # KataGo's k
FPU = (0.25, 0.5)
ROWS = 5  # not a multiple of the four rows per workgroup


# ----------------------------------------------------------------------------- the evaluator
def spikes_of(m, n, k):
    """the spike cells of a board: the cell that completes a run along row 0 from its first k - 1 cells, one past the
    middle, one before the last"""
    C = m * n
    return (k - 1, C // 2 + 1, C - 2)


def tables(C, spikes, spike, zero=None, above=None):
    """(priors f32 [C], the spike cells as 0 / 1 f32 [C]): ``spike`` on the spike cells, (a % 4 + 1) / 512 elsewhere;
    ``zero``: a cell of prior 0; ``above``: a spike cell of prior 2"""
    table = ((np.arange(C) % 4 + 1) / 512).astype(np.float32)
    mark = np.zeros(C, np.float32)
    table[list(spikes)], mark[list(spikes)] = spike, 1
    if zero is not None:
        table[zero] = 0
    if above is not None:
        table[above] = 2
    return table, mark


def spike_np(C, spikes, spike=0.25, bad=1.0, zero=None, above=None, lost=False):
    """priors: the table on the legal cells.  value: +bad when the opponent holds more spike cells than the side to move,
    -bad when fewer, else a function of the stone counts in sixteenths -- with ``lost``, +1/2: every move looks bad to
    the one who made it, and a cell of prior 0 is reached once every other has a visit.  Every number is exact in
    bfloat16"""
    table, mark = tables(C, spikes, spike, zero, above)

    def evaluate(leaf_obs, leaf_mask):
        o = leaf_obs.astype(np.float32).reshape(len(leaf_obs), 2, -1)
        own, opp = (o[:, 0] * mark).sum(axis=1), (o[:, 1] * mark).sum(axis=1)
        cnt = o.sum(axis=2)
        small = (2 - np.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5)) / 16 if not lost else np.full(len(o), 0.5)
        value = np.where(opp > own, bad, np.where(own > opp, -bad, small))
        return leaf_mask.astype(np.float32) * table, value.astype(np.float32)

    return evaluate


# ----------------------------------------------------------------------------- the lockstep cases
#          name      board     I   spike   bad
BOARDS = {"3x3x3": ((3, 3, 3), 12, 0.125, 1.0),      # one pass per lane
          "9x9x5": ((9, 9, 5), 24, 0.25, 1.0),       # 81 cells: the arg-max and the sum span two passes and the lanes
          "7x9x5": ((7, 9, 5), 16, 0.25, 1.0),       # a sibling of a built-in variant
          "5x5x4": ((5, 5, 4), 20, 0.0625, 0.75),    # the generic form
          "19x19x5": ((19, 19, 5), 8, 0.25, 1.0),    # the multi-word form
          "12x12x5": ((12, 12, 5), 8, 0.125, 1.0),   # generic, five words
          "12x13x5": ((12, 13, 5), 16, 0.25, 1.0),   # <6,13,5>: 156 cells for the variant's 169
          "16x15x5": ((16, 15, 5), 12, 0.25, 1.0),   # <8,15,5>: 240 cells for 225, a plane that fills its last word
          "7x9x7": ((7, 9, 7), 12, 0.25, 1.0),       # generic, three words: the four-word instantiation
          "17x17x5": ((17, 17, 5), 12, 0.25, 1.0),   # generic, ten words: the sixteen-word instantiation
          "25x25x5": ((25, 25, 5), 8, 0.25, 1.0)}    # generic, 21 words: the 32-word instantiation
SPIKES = {"12x12x5": 2}  # boards with fewer than three spike cells: the first of ``spikes_of``
# L, solver, fpu, temperature: the whole cross (an act of these budgets takes milliseconds)
OPTIONS = [(L, solver, fpu, t) for L in (1, 4) for solver in (False, True) for fpu in (None, FPU) for t in (0, 1)]


def rows_of(name):
    """five rows: an empty board; two positions a few stones in; a position whose side to move completes a run at the
    first spike cell (a WIN child at the root: with the solver nothing is pruned there); a position further in"""
    (m, n, k), _, _, _ = BOARDS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    obs = np.zeros((ROWS, 2, m, n), np.float32)
    obs[1:3] = random_positions(m, n, k, 2, rng, max_fill=0.25)
    obs[3, 0, 0, :k - 1] = 1
    obs[3, 1, 1, :k - 1] = 1
    obs[4] = random_positions(m, n, k, 1, rng, max_fill=0.5)[0]
    return obs


def evaluator_of(name, **kw):
    (m, n, k), _, spike, bad = BOARDS[name]
    return spike_np(m * n, spikes_of(m, n, k)[:SPIKES.get(name, 3)], spike, bad, **kw)


def new_rule(name, L, solver, fpu, temperature=0, forced=K_FORCED, seen=None, evaluator=None, **kw):
    (m, n, k), I, _, _ = BOARDS[name]
    return ForcedPuct(k, I, C_PUCT, evaluator or evaluator_of(name), L, seed=SEED, env_id0=ENV_ID0, temperature=temperature,
                      leaves=seen, solver=solver, fpu=fpu, forced=forced, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, L, solver, fpu, temperature=0, forced=K_FORCED):
    """(obs, (actions, visits, root_value, carried, proof), every evaluation's (leaf_obs, leaf_mask), the rule after the
    act) of the rule"""
    obs, seen = rows_of(name), []
    rule = new_rule(name, L, solver, fpu, temperature, forced, seen)
    return obs, rule.act(obs, step=2), seen, rule


# the further lockstep cases, on 3x3x3: a prior of 2 on a spike cell; a prior of 0 on a cell that is visited (t_a = 0, so
# F_a = 0 and the cell keeps its count by the walk as by the rule's exception)
EDGE_NAME = "3x3x3"
EDGES = {"above": dict(above=5), "zero": dict(zero=0, lost=True)}


@functools.lru_cache(maxsize=None)
def edge_reference(which, L):
    obs, seen = rows_of(EDGE_NAME), []
    rule = new_rule(EDGE_NAME, L, False, None, seen=seen, evaluator=evaluator_of(EDGE_NAME, **EDGES[which]))
    return obs, rule.act(obs, step=2), seen, rule


# the floor's t = k P (n_0 - 1) on the large generic boards: under the evaluator for which every move looks bad, with a
# spike prior of 1/8, I = 16 and four leaves, cells are pruned down to n' - F with n' >= F + 2, so that a floor taken from
# n_0 in the place of n_0 - 1 leaves other counts (tests/test_puct_forced_cpu.py plants it).  None of the cases of BOARDS
# on a board of more than 256 cells tells the two apart
FLOOR_NAMES, FLOOR_I, FLOOR_SPIKE, FLOOR_L = ("17x17x5", "25x25x5"), 16, 0.125, 4


def floor_evaluator(name, **kw):
    m, n, k = BOARDS[name][0]
    return spike_np(m * n, spikes_of(m, n, k), FLOOR_SPIKE, 1.0, lost=True, **kw)


def floor_rule(name, seen=None):
    k = BOARDS[name][0][2]
    return ForcedPuct(k, FLOOR_I, C_PUCT, floor_evaluator(name), FLOOR_L, seed=SEED, env_id0=ENV_ID0, leaves=seen, fpu=FPU,
                      forced=K_FORCED)


@functools.lru_cache(maxsize=None)
def floor_reference(name):
    obs, seen = rows_of(name), []
    rule = floor_rule(name, seen)
    return obs, rule.act(obs, step=2), seen, rule


# the solver's clause of the selection: on 9x9x5 the opponent holds four in a row along row 1 with one end free, cell 13,
# which is a spike cell beside two others.  A root move to another spike is answered at 13 -- the lowest of the reply's
# equal best scores -- which wins: the second, forced visit proves the move LOSS with two stored visits, and from
# S' = 9 on it is short of its floor, 4 < 2 * 1/4 * S'.  Clause (2) alone keeps it from being forced again.
LOSS_NAME, LOSS_SPIKES = "9x9x5", (13, 41, 79)
LOSS_OPTIONS = [(L, fpu) for L in (1, 4) for fpu in (None, FPU)]


def loss_rows():
    (m, n, k), _, _, _ = BOARDS[LOSS_NAME]
    obs = np.zeros((ROWS, 2, m * n), np.float32)
    for i in range(ROWS):
        obs[i, 1, n:n + k - 1] = 1  # the opponent's stones: row 1, columns 0 .. k - 2
        obs[i, 0, [30 + i, 47 + 2 * i, 64 - i, 75 - 3 * i]] = 1  # the side to move: four stones that threaten nothing
    return obs.reshape(ROWS, 2, m, n)


def loss_evaluator():
    (m, n, k), _, spike, bad = BOARDS[LOSS_NAME]
    return spike_np(m * n, LOSS_SPIKES, spike, bad)


@functools.lru_cache(maxsize=None)
def loss_reference(L, fpu):
    obs, seen = loss_rows(), []
    rule = new_rule(LOSS_NAME, L, True, fpu, seen=seen, evaluator=loss_evaluator())
    return obs, rule.act(obs, step=2), seen, rule


# a kept tree over three acts: (L, solver).  The rule's acts, each on the position the one before it played into
REUSE = [(1, False), (4, True)]
REUSE_NAME, REUSE_PLIES = "9x9x5", 3


REUSE_NODES = BOARDS[REUSE_NAME][1] + 5  # a ply carries at most five nodes over: children of a carried root are dropped


def reuse_rule(L, solver, seen=None):
    return new_rule(REUSE_NAME, L, solver, FPU, seen=seen, reuse=True, tree_nodes=REUSE_NODES)


@functools.lru_cache(maxsize=None)
def reuse_reference(L, solver):
    """per act: (obs, the act's outputs, its evaluations' leaves, raw_visits, the root's n_0 of every row)"""
    from puct_reuse_cases import advance

    (m, n, k), _, _, _ = BOARDS[REUSE_NAME]
    seen = []
    rule = reuse_rule(L, solver, seen)
    obs, resets, acts = rows_of(REUSE_NAME), np.zeros(ROWS, np.int64), []
    for ply in range(REUSE_PLIES):
        del seen[:]
        out = rule.act(obs, step=ply)
        acts.append((obs, out, list(seen), rule.raw_visits.copy(), [t.n[0] for t in rule.trees]))
        obs = advance(obs, out[0], k, 1, resets)
    return acts


# ----------------------------------------------------------------------------- the per-row cases
N = ROWS


def state_of(board, start):
    return start_state(board, start)  # ("late": ``late_start`` of N rows)


def free_spikes(board, state):
    """the spike cells of a per-row case: the board's own from an empty start; from a stored or late start the three
    cells that are free in the most rows (ties to the lowest cell), so that the spikes are on the board at all"""
    m, n, k = board
    if state is None:
        return spikes_of(m, n, k)
    occupied = unpack_boards(state[0], m, n).reshape(-1, 2, m * n).any(axis=1)
    free = (~occupied).sum(axis=0)
    order = sorted(range(m * n), key=lambda a: (-int(free[a]), a))
    return tuple(sorted(order[:3]))


# board, start, temp_plies, rounds, seed, root_noise, noise_on_fast, solver, fpu.  FULL / FAST budgets and round counts
# are those of tests/search_selfplay_async_fpu_cases.py; the rows are N, or as many as a stored start state has.
ASYNC_CASES = [
    ((3, 3, 3), None, 2, 130, 6, NOISE, False, True, None),
    ((3, 3, 3), None, 2, 130, 6, None, False, False, FPU),
    ((9, 9, 5), "late", 4, 150, 6, NOISE, False, False, FPU),
    ((7, 9, 5), "golden", 4, 150, 6, NOISE, True, True, None),
    ((19, 19, 5), "golden", 4, 150, 6, FAINT, False, True, FPU),
    ((12, 12, 5), "golden", 4, 150, 6, None, False, False, None),
    ((7, 7, 4), None, 4, 500, 6, NOISE, False, True, FPU),
    # the variants <6,13,5> and <8,15,5> and the four-word generic form.  (Noise only where no stored row is two stones
    # short of a drawn board, as in tests/search_selfplay_async_fpu_cases.py.)
    ((12, 13, 5), "golden", 4, 150, 6, None, False, True, FPU),
    ((16, 15, 5), "golden", 4, 150, 6, None, False, False, FPU),
    ((7, 9, 7), "late", 4, 150, 6, NOISE, False, True, None),
    # the generic forms of sixteen and of thirty-two words: ten and 21 words a plane
    ((17, 17, 5), "late", 4, 150, 6, NOISE, False, True, FPU),
    ((25, 25, 5), "late", 4, 150, 6, NOISE, False, True, FPU),
]


def rows_in(state):
    return N if state is None else len(state[1])


def async_evaluator(board, state):
    m, n, k = board
    return spike_np(m * n, free_spikes(board, state))


def new_async_rule(case, forced=K_FORCED):
    """(the rule of ASYNC_CASES[case] on its start state, that state or None, its evaluator)"""
    board, start, temp, _, seed, noise, on_fast, solver, fpu = ASYNC_CASES[case]
    m, n, k = board
    state = state_of(board, start)
    rule = AsyncOptsForcedRule(m, n, k, rows_in(state), m * n, FULL, FAST, THRESHOLD, C_PUCT, temp, seed, ENV_ID0,
                               root_noise=noise, noise_on_fast=on_fast, solver=solver, fpu=fpu, forced=forced)
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule, state, async_evaluator(board, state)


@functools.lru_cache(maxsize=None)
def async_run(case, forced=K_FORCED):
    """the rule's run of ASYNC_CASES[case] alone, with its own noise"""
    rule, _, ev = new_async_rule(case, forced)
    obs, mask = rule.view()
    for _ in range(ASYNC_CASES[case][3]):
        obs, mask, _ = rule.advance(*ev(obs, mask))
    return rule


def assert_every_option_was_used(case, rule):
    """what tests/search_selfplay_async_fpu_cases.py asks of its cases: a game ends, fast and full plies are recorded, the
    rows are out of step; with the solver a ply ends by proof, with noise a root takes it"""
    _, _, _, _, _, noise, _, solver, _ = ASYNC_CASES[case]
    assert not rule.errors and rule.N % 4
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0
    assert len(set(rule.row_plies.tolist())) > 1
    assert sum(1 for rec in rule.proven_plies if rec[4]) > 0 or not solver
    assert rule.noised_roots > 0 or not noise
