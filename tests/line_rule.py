"""Brute-force statement of what wins on an m x n board with runs of k (test helper), and of which boards share one
ahead-of-time kernel variant.

The host dispatch picks a row of ``MNK_BUILTIN_BOARDS`` (csrc/mnk_emit.h) by (n, k, NW) with NW = ceil(m * (n + 1) / 32)
32-bit words per plane -- never by m -- so a row <NW, n, k> serves every board of that width, run length and word count:
its SIBLINGS.  Such a board has no run-time specialised twin to disagree with (mnk_jit_prepare returns early), so its
only check is an independent rule.  This one enumerates cells: no convolution stencils (the oracle), no shifted bit
strings (the kernels), no outward run counting (tactical_rule).

  lines(m, n, k)   every set of k collinear in-board cells, in the four directions
  wraps(m, n, k)   every set of k cells at a constant flat-index stride of 1, n - 1, n or n + 1 that is NOT a line: what
                   would win if a run wrapped round a board edge
"""
import functools
import os
import re

import numpy as np

EMIT_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-selfplay-mnk_amd", "csrc", "mnk_emit.h")
_DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))
MAX_M = 64  # no plane is longer than 1 024 bits: far beyond any sibling


def words(m: int, n: int) -> int:
    """32-bit words of one plane: rows of n cells and one guard bit"""
    return (m * (n + 1) + 31) // 32


def builtin_rows():
    """[(NW, n, k, C)] of the ``MNK_BUILTIN_BOARDS`` line, in its order"""
    with open(EMIT_H) as f:
        (line,) = [ln for ln in f if re.match(r"\s*#define\s+MNK_BUILTIN_BOARDS\(X\)", ln)]
    rows = [tuple(int(v) for v in row) for row in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", line)]
    assert rows, "MNK_BUILTIN_BOARDS has no row"
    return rows


def siblings(row):
    """every m whose m x n x k board dispatches to ``row`` = (NW, n, k, C): k <= m and the same word count"""
    nw, n, k = row[0], row[1], row[2]
    return [m for m in range(k, MAX_M + 1) if words(m, n) == nw]


def sibling_boards(square=True, non_square=True):
    """[(m, n, k)] over every row, smallest m first within a row"""
    out = []
    for row in builtin_rows():
        for m in siblings(row):
            if (m == row[1] and square) or (m != row[1] and non_square):
                out.append((m, row[1], row[2]))
    return out


@functools.lru_cache(maxsize=None)
def lines(m: int, n: int, k: int):
    """sorted tuple of k-tuples of flat cell indices (ascending along the direction of travel)"""
    out = []
    for dr, dc in _DIRS:
        for r in range(m):
            for c in range(n):
                r1, c1 = r + (k - 1) * dr, c + (k - 1) * dc
                if 0 <= r1 < m and 0 <= c1 < n:
                    out.append(tuple((r + j * dr) * n + (c + j * dc) for j in range(k)))
    return tuple(sorted(set(out)))


@functools.lru_cache(maxsize=None)
def wraps(m: int, n: int, k: int):
    """k cells at a constant flat stride that a line scan on the flat index would accept and the board does not"""
    real = {frozenset(ln) for ln in lines(m, n, k)}
    out = set()
    if k < 2:
        return ()
    for stride in sorted({1, n - 1, n, n + 1} - {0}):
        for start in range(m * n - (k - 1) * stride):
            cells = tuple(start + j * stride for j in range(k))
            if frozenset(cells) not in real:
                out.add(cells)
    return tuple(sorted(out))


def last_word_cells(m: int, n: int):
    """the cells whose bit (cell + cell // n: one guard bit per row) lies in the top 32-bit word of the plane"""
    top = words(m, n) - 1
    return [cell for cell in range(m * n) if (cell + cell // n) >> 5 == top]


def plane_of(cells, m: int, n: int) -> np.ndarray:
    p = np.zeros(m * n, dtype=np.float32)
    p[list(cells)] = 1.0
    return p.reshape(m, n)


def has_line(plane: np.ndarray, k: int) -> bool:
    """the rule itself on one bool / 0-1 plane [m, n]: some line of k cells is all stones"""
    m, n = plane.shape
    flat = np.asarray(plane).reshape(-1) != 0
    return any(all(flat[c] for c in ln) for ln in lines(m, n, k))


def cases(m: int, n: int, k: int):
    """[(cells, wins)]: every line (wins) and every wrap (does not)"""
    return [(ln, True) for ln in lines(m, n, k)] + [(w, False) for w in wraps(m, n, k)]


def check_scan(scan, m: int, n: int, k: int):
    """``scan(plane[m, n] of 0/1, k) -> bool`` against every line and wrap of the board; the list of (cells, wanted, got)
    it gets wrong (empty: the scan agrees with the rule on all of them)"""
    bad = []
    for cells, want in cases(m, n, k):
        got = bool(scan(plane_of(cells, m, n), k))
        if got != want:
            bad.append((cells, want, got))
    return bad
