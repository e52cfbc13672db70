"""CPU: the brute-force line rule (tests/line_rule.py) on every board that reaches a built-in kernel variant.

1. ``siblings`` of the rows of MNK_BUILTIN_BOARDS are the boards DESIGN.md's table lists.
2. The oracle's win test agrees with the rule on every line and every wrap of all of them (through ``env.step``, the
   line's last cell played as the move, black and white).
3. The checker has teeth: restated bit-string scans with ONE planted defect each are rejected by at least one line or
   wrap on at least one sibling board; the boards whose plane fills its last 32-bit word exactly (8x3, 16x15) reject the
   top-word mutants.
"""
import numpy as np
import pytest
import torch

import line_rule as lr
from oracle.env_torch import OracleVectorEnv

TABLE = {(1, 3, 3): [3, 4, 5, 6, 7, 8], (3, 9, 5): [7, 8, 9], (6, 13, 5): [12, 13], (8, 15, 5): [15, 16], (12, 19, 5): [18, 19]}
BOARDS = lr.sibling_boards()


def test_builtin_rows_are_read_from_the_source():
    rows = lr.builtin_rows()
    assert len(rows) >= 5 and len(set(rows)) == len(rows)
    for nw, n, k, c in rows:
        assert c == n * n and nw == lr.words(n, n) and k <= n  # every row is named after its square board


def test_siblings_are_the_boards_of_the_table():
    got = {row[:3]: lr.siblings(row) for row in lr.builtin_rows()}
    for key, ms in TABLE.items():
        assert got[key] == ms, key
    assert len(BOARDS) == sum(len(v) for v in got.values())
    assert (16, 15, 5) in BOARDS and (8, 3, 3) in BOARDS and (18, 19, 5) in BOARDS
    # the full-last-word boards: 256 and 32 bits
    assert 16 * 16 == 32 * lr.words(16, 15) and 8 * 4 == 32 * lr.words(8, 3)


def test_lines_and_wraps_on_a_board_small_enough_to_count_by_hand():
    # 3x3x3: 3 rows, 3 columns, 2 diagonals
    assert len(lr.lines(3, 3, 3)) == 8
    assert (0, 4, 8) in lr.lines(3, 3, 3) and (2, 4, 6) in lr.lines(3, 3, 3)
    w = lr.wraps(3, 3, 3)
    assert (1, 2, 3) in w and (2, 3, 4) in w            # a row run over the right edge
    assert (1, 3, 5) in w and (0, 2, 4) in w            # stride n - 1 that leaves the anti-diagonal
    assert (1, 5, 9) not in w and all(max(c) < 9 for c in w)
    assert not {frozenset(c) for c in w} & {frozenset(c) for c in lr.lines(3, 3, 3)}
    # m x n x k line count: rows m(n-k+1) + columns n(m-k+1) + 2 diagonals (m-k+1)(n-k+1)
    for m, n, k in BOARDS:
        want = m * (n - k + 1) + n * (m - k + 1) + 2 * (m - k + 1) * (n - k + 1)
        assert len(lr.lines(m, n, k)) == want, (m, n, k)
        assert len(lr.wraps(m, n, k)) > 0
    assert lr.last_word_cells(8, 3) == list(range(24)) and lr.last_word_cells(3, 3) == list(range(9))
    assert lr.last_word_cells(16, 15) == list(range(210, 240))     # rows 14 and 15: bits 224 .. 254
    assert lr.last_word_cells(9, 9) == list(range(58, 81))         # bits 64 .. 89


def oracle_outcomes(m, n, k, side):
    """(want, reward, done) of every line / wrap with its last cell played by ``side`` through OracleVectorEnv.step"""
    cs = lr.cases(m, n, k)
    env = OracleVectorEnv(m, n, k, len(cs))
    acts = np.zeros(len(cs), dtype=np.int64)
    for i, (cells, _) in enumerate(cs):
        plane = lr.plane_of(cells[:-1], m, n)
        env.boards[i, side] = torch.from_numpy(plane)
        acts[i] = cells[-1]
    env.current_player[:] = side
    env.move_counts[:] = k - 1
    _, rew, done = env.step(torch.from_numpy(acts))
    return np.array([w for _, w in cs]), rew.numpy(), done.numpy()


@pytest.mark.parametrize("m,n,k", BOARDS)
def test_oracle_wins_on_every_line_and_on_no_wrap(m, n, k):
    for side in (0, 1):
        want, rew, done = oracle_outcomes(m, n, k, side)
        assert want.any() and not want.all()
        assert np.array_equal(done, want) and np.array_equal(rew, want.astype(np.float32)), (m, n, k, side)


# ----------------------------------------------------------------------------- planted defects
def _bits(plane, stride_row, rows=None, cols=None):
    m, n = plane.shape
    x = 0
    for r in range(m if rows is None else min(m, rows)):
        for c in range(n):
            if plane[r, c] != 0:
                x |= 1 << (r * stride_row + c)
    return x


def _runs(x, strides, length):
    for s in strides:
        y = x
        for j in range(1, length):
            y &= x >> (j * s)
        if y:
            return True
    return False


def scan_good(plane, k):
    """the kernels' formulation, restated: rows of n cells and a guard bit, AND of k shifted copies in four strides"""
    n = plane.shape[1]
    return _runs(_bits(plane, n + 1), (1, n, n + 1, n + 2), k)


def scan_no_guard(plane, k):
    n = plane.shape[1]
    return _runs(_bits(plane, n), (1, n - 1, n, n + 1), k)


def scan_square(plane, k):
    n = plane.shape[1]
    return _runs(_bits(plane, n + 1, rows=n), (1, n, n + 1, n + 2), k)


def scan_last_row_dropped(plane, k):
    m, n = plane.shape
    return _runs(_bits(plane, n + 1, rows=m - 1), (1, n, n + 1, n + 2), k)


def scan_short_runs(plane, k):
    n = plane.shape[1]
    return _runs(_bits(plane, n + 1), (1, n, n + 1, n + 2), k - 1)


def scan_top_word_modulo_mask(plane, k):
    """the valid bits of the top word taken as (1 << (bits % 32)) - 1: nothing is left of a word that is full"""
    m, n = plane.shape
    total = m * (n + 1)
    nw = lr.words(m, n)
    keep = (1 << (32 * (nw - 1))) - 1 | ((1 << (total % 32)) - 1) << (32 * (nw - 1))
    return _runs(_bits(plane, n + 1) & keep, (1, n, n + 1, n + 2), k)


def scan_top_word_last_bit(plane, k):
    """the valid mask one bit short: the highest cell of the plane -- on a full last word bit 30 of the top word, the
    one below the last row's guard bit -- is lost"""
    m, n = plane.shape
    keep = (1 << (m * (n + 1) - 2)) - 1
    return _runs(_bits(plane, n + 1) & keep, (1, n, n + 1, n + 2), k)


MUTANTS = {"no guard column": scan_no_guard, "board taken as n x n": scan_square, "last row dropped": scan_last_row_dropped,
           "runs of k - 1": scan_short_runs, "top word, modulo mask": scan_top_word_modulo_mask,
           "top word, last bit": scan_top_word_last_bit}


def test_the_restated_scan_passes_on_every_sibling():
    for m, n, k in BOARDS:
        assert lr.check_scan(scan_good, m, n, k) == [], (m, n, k)
        assert lr.check_scan(lambda p, kk: lr.has_line(p, kk), m, n, k) == []


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_planted_defect_is_rejected(name):
    rejecting = {b: lr.check_scan(MUTANTS[name], *b) for b in BOARDS}
    rejecting = {b: bad for b, bad in rejecting.items() if bad}
    assert rejecting, f"no sibling board notices: {name}"
    non_square = [b for b in rejecting if b[0] != b[1]]
    if name == "no guard column":       # accepts wraps, never misses a line
        assert all(not want and got for bad in rejecting.values() for _, want, got in bad) and len(rejecting) == len(BOARDS)
    if name == "runs of k - 1":
        assert all(not want and got for bad in rejecting.values() for _, want, got in bad) and len(rejecting) == len(BOARDS)
    if name == "board taken as n x n":  # only a board taller than wide has rows to lose: the square controls cannot see it
        assert set(rejecting) == {b for b in BOARDS if b[0] > b[1]} and non_square
    if name == "last row dropped":
        assert len(rejecting) == len(BOARDS)
    if name.startswith("top word"):
        assert (16, 15, 5) in rejecting and (8, 3, 3) in rejecting
    if name == "top word, modulo mask":  # seen by the full-last-word boards alone
        assert set(rejecting) == {b for b in BOARDS if b[0] * (b[1] + 1) % 32 == 0} == {(8, 3, 3), (16, 15, 5)}


def test_top_word_mutants_fail_on_lines_that_end_in_the_last_word():
    for b in ((16, 15, 5), (8, 3, 3)):
        top = set(lr.last_word_cells(b[0], b[1]))
        for name in ("top word, modulo mask", "top word, last bit"):
            bad = lr.check_scan(MUTANTS[name], *b)
            assert bad and all(want and not got and set(cells) & top for cells, want, got in bad), (b, name)
