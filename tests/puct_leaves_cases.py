"""What the CPU and the GPU tests of the PUCT player with several leaves per evaluation share: the boards, budgets and
positions the GPU test runs (tests/test_gpu_puct_leaves.py), and the rule's answer on each, computed once per process.
The CPU test (tests/test_puct_leaves_cpu.py) checks from the rule's trace alone that these inputs reach the paths a kernel
can go wrong on: void slots, terminal leaves repeated within a round, slots that share a prefix -- and a case with none."""
import functools

import numpy as np

from puct_leaves_rule import LeavesPuct
from puct_reuse_cases import exact_np
from tactical_rule import random_positions

C_PUCT, SEED, ENV_ID0 = 1.25, 43, 7
#        name      board        rows  I     the L of the case
CASES = {
    "3x3x3": ((3, 3, 3), 23, 32, (1, 2, 4, 8, 16)),      # NW = 1; half-full boards: terminals everywhere, trees that run out
    "4x6x3": ((4, 6, 3), 14, 48, (1, 2, 4, 8, 16)),      # the generic form, not square
    "9x9x5": ((9, 9, 5), 6, 48, (1, 2, 4, 8, 16)),       # C > 64: two trips of every per-cell loop; a built-in variant
    "19x19x5": ((19, 19, 5), 3, 32, (4, 16)),            # C = 361; fewer rows than a workgroup holds
    "round": ((9, 9, 5), 5, 8, (8,)),                    # I = L: a single round
    "long": ((9, 9, 5), 1, 2048, (16,)),                 # the largest budget and the most leaves, one row
    # boards that share a built-in variant with a board of another row count (tests/test_gpu_variant_siblings.py)
    "8x3x3": ((8, 3, 3), 16, 32, (4, 16)),               # <1,3,3> with 24 cells
    "7x9x5": ((7, 9, 5), 8, 48, (4, 16)),                # <3,9,5> with 63 cells
    "16x15x5": ((16, 15, 5), 4, 32, (4,)),               # <8,15,5> with 240 cells: a plane that fills its last word
    "12x13x5": ((12, 13, 5), 3, 32, (4,)),               # <6,13,5> with 156 cells; a partial workgroup
    "18x19x5": ((18, 19, 5), 3, 32, (4,)),               # <12,19,5> with 342 cells; a partial workgroup
    # the generic forms of four and of eight words
    "7x9x7": ((7, 9, 7), 3, 16, (4,)),                   # three words
    "12x12x5": ((12, 12, 5), 3, 16, (4,)),               # five words
    # the generic forms of sixteen and of thirty-two words
    "17x17x5": ((17, 17, 5), 3, 8, (1, 4)),              # ten words; 289 cells: five trips, leaf rows of 289 bytes
    "25x25x5": ((25, 25, 5), 3, 8, (1, 4)),              # 21 words, an odd count; 625 cells: ten trips
}
LARGE = {"17x17x5": "uint8", "25x25x5": "bfloat16"}      # and the leaf dtype each takes in the GPU test's dtype case
PARAMS = [(name, L) for name, (_, _, _, Ls) in CASES.items() for L in Ls]


def positions(name):
    (m, n, k), rows, _, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "3x3x3":  # half-full: four or five stones, no run yet
        out = []
        while len(out) < rows:
            o = random_positions(m, n, k, 1, rng, max_fill=0.6)[0]
            if 4 <= o.sum() <= 5:
                out.append(o)
        obs = np.stack(out)
    else:
        obs = random_positions(m, n, k, rows, rng, max_fill=0.5 if name in ("4x6x3", "8x3x3") else 0.25)
    if name in ("4x6x3", "9x9x5"):  # an empty board, and a full one (no legal cell: void slots only)
        obs[0] = 0
        obs[1, 0].reshape(-1)[::2], obs[1, 1].reshape(-1)[::2] = 1, 0
        obs[1, 0].reshape(-1)[1::2], obs[1, 1].reshape(-1)[1::2] = 0, 1
    return obs


@functools.lru_cache(maxsize=None)
def reference(name, L, temperature=0):
    """(obs, (actions, visits, root_value), every evaluation's (leaf_obs, leaf_mask), the per-row trace) of the rule"""
    (m, n, k), _, I, _ = CASES[name]
    obs, seen = positions(name), []
    rule = LeavesPuct(k, I, C_PUCT, exact_np(m * n), L, seed=SEED, env_id0=ENV_ID0, temperature=temperature, leaves=seen)
    out = rule.act(obs, step=2)
    return obs, out[:3], seen, rule.trace
