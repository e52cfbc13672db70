"""CPU: the one-ply tactical player (take a win, else block one, else play at random) -- the numpy restatement of the
rule in tests/tactical_rule.py against the reference's own win test (tests/golden/tactical_positions.npz) and hand-built
positions; the C ABI of the three new entry points (header, binding, host argument checks) and their run-time compiled
variants, which hiprtc builds without a GPU."""
import os

import numpy as np
import pytest

from oracle import philox
from oracle.packing import unpack_boards
from player_cases import board, check_header_and_binding, header_constants, lib  # noqa: F401 (lib: the fixture)
from tactical_rule import completions, tactical_moves, tactical_sets

NEW = ("mnk_selfplay_step_tactical", "mnk_selfplay_step_tactical_logits", "mnk_sample_tactical")


def cells(mask_row, n):
    return sorted((int(c) // n, int(c) % n) for c in np.flatnonzero(mask_row))


# ----------------------------------------------------------------------------- the rule against the reference
@pytest.mark.parametrize("tag", ["3x3x3", "4x6x3", "6x7x4", "9x9x5", "19x19x5"])
def test_rule_reproduces_the_reference_win_test(golden_dir, tag):
    """W and B of every fixture position equal the cells where the REFERENCE env declared a win for the side to move /
    the other side after that cell was played on a copy (tests/golden/make_golden_tactical.py)"""
    data = np.load(os.path.join(golden_dir, "tactical_positions.npz"))
    m, n, k = (int(v) for v in tag.split("x"))
    obs = unpack_boards(data[tag + "_planes"], m, n)
    s, win, block = tactical_sets(obs, k)
    assert np.array_equal(win, data[tag + "_win_mover"] != 0)
    assert np.array_equal(block, data[tag + "_win_other"] != 0)
    assert win.any() and block.any() and (~win.any(1)).any()  # the fixture covers all three branches
    legal = ((obs[:, 0] == 0) & (obs[:, 1] == 0)).reshape(len(obs), -1)
    want = np.where(win.any(1, keepdims=True), win, np.where(block.any(1, keepdims=True), block, legal))
    want = np.where(want.any(1, keepdims=True), want, True)
    assert np.array_equal(s, want)


# ----------------------------------------------------------------------------- hand-built positions
def test_win_beats_block():
    obs = board(["xx.", "oo.", "..."])
    s, win, block = tactical_sets(obs, 3)
    assert cells(win[0], 3) == [(0, 2)] and cells(block[0], 3) == [(1, 2)]
    assert cells(s[0], 3) == [(0, 2)]
    assert all(tactical_moves(obs, 3, x)[0] == 2 for x in (0, 1 << 31, 0xFFFFFFFF))


def test_block_when_there_is_no_win():
    obs = board(["x..", "oo.", "x.."])
    s, win, _ = tactical_sets(obs, 3)
    assert not win.any() and cells(s[0], 3) == [(1, 2)]


def test_several_winning_cells_are_drawn_in_action_order():
    obs = board([".xxxx.", "oooo..", "......"])   # an open four: both ends win; the opponent's four is never blocked
    s, win, block = tactical_sets(obs, 5)
    assert cells(win[0], 6) == [(0, 0), (0, 5)] and cells(block[0], 6) == [(1, 4)]
    assert tactical_moves(obs, 5, 0)[0] == 0                          # deterministic: the first cell of S
    assert tactical_moves(obs, 5, (1 << 31) - 1)[0] == 0              # r = mulhi32(x, 2)
    assert tactical_moves(obs, 5, 1 << 31)[0] == 5


def test_double_threat_of_the_opponent_blocks_one_of_them():
    obs = board(["oo.oo", ".....", "x...x", ".....", "....."])  # the gap completes both halves: one cell, two runs
    _, _, block = tactical_sets(obs, 3)
    assert cells(block[0], 5) == [(0, 2)]
    obs = board(["oo...", "o....", ".....", "..x..", "....x"])     # two separate threats: both cells are candidates
    s, win, block = tactical_sets(obs, 3)
    assert not win.any() and cells(block[0], 5) == [(0, 2), (2, 0)] and np.array_equal(s, block)


def test_overline_counts():
    obs = board(["xx.xx....", "........."])
    _, win, _ = tactical_sets(obs, 4)
    assert cells(win[0], 9) == [(0, 2)]   # a run of five through the cell with k = 4
    _, win, _ = tactical_sets(obs, 5)
    assert cells(win[0], 9) == [(0, 2)]   # exactly five


def test_k1_and_one_row_boards():
    obs = board([".x.o..."])
    s, win, _ = tactical_sets(obs, 1)
    assert cells(win[0], 7) == [(0, 0), (0, 2), (0, 4), (0, 5), (0, 6)] and np.array_equal(s, win)
    obs = board(["xx.o.x."])                 # a row: the gap wins
    assert cells(tactical_sets(obs, 3)[1][0], 7) == [(0, 2)]
    obs = board(["..x", "x..", "..."])       # row ends do not join the next row (the kernels' guard column)
    assert not tactical_sets(obs, 3)[1].any()


def test_directions_and_full_board():
    for rows, cell in ((["x..", ".x.", "..."], (2, 2)), (["..x", ".x.", "..."], (2, 0)), (["x..", "x..", "..."], (2, 0))):
        assert cells(tactical_sets(board(rows), 3)[1][0], 3) == [cell]
    full = board(["xox", "oxo", "oxo"])
    s, win, block = tactical_sets(full, 3)
    assert s.all() and not win.any() and not block.any()   # no legal cell: all C cells, like RandomPolicy's guard
    assert tactical_moves(full, 3, 0xFFFFFFFF)[0] == 8


def test_quiet_positions_play_the_random_move():
    """where neither side can complete a run, the tactical move IS the uniformly random one drawn from the same u32"""
    rng = np.random.default_rng(3)
    obs = np.zeros((64, 2, 9, 9), dtype=np.float32)
    for i in range(64):
        cells_ = rng.choice(81, size=6, replace=False)
        obs[i, 0].reshape(-1)[cells_[:3]] = 1
        obs[i, 1].reshape(-1)[cells_[3:]] = 1
    x = philox.rand_u32(9, np.arange(64, dtype=np.uint64), 4, philox.STREAM_OPP)
    legal = ((obs[:, 0] == 0) & (obs[:, 1] == 0)).reshape(64, -1)
    assert np.array_equal(tactical_moves(obs, 5, x), philox.pick_legal(legal, x))


def test_completions_match_brute_force():
    rng = np.random.default_rng(7)
    for m, n, k in ((4, 6, 3), (6, 7, 4), (5, 5, 1), (1, 6, 1), (7, 5, 5)):
        st = rng.random((40, m, n)) < 0.4
        empty = (rng.random((40, m, n)) < 0.5) & ~st
        got = completions(st, empty, k)
        for b in range(40):
            for r in range(m):
                for c in range(n):
                    ok = False
                    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                        run = 1
                        for sgn in (1, -1):
                            rr, cc = r + sgn * dr, c + sgn * dc
                            while 0 <= rr < m and 0 <= cc < n and st[b, rr, cc]:
                                run += 1
                                rr, cc = rr + sgn * dr, cc + sgn * dc
                        ok |= run >= k
                    assert got[b, r, c] == (ok and empty[b, r, c])


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_tactical_entry_points_and_the_binding_matches(lib):
    for name in NEW:
        check_header_and_binding(lib, name)
    assert lib.SIGNATURES["mnk_selfplay_step_tactical"] == lib.SIGNATURES["mnk_selfplay_step_random"]
    assert lib.SIGNATURES["mnk_selfplay_step_tactical_logits"] == lib.SIGNATURES["mnk_selfplay_step_random_logits"]
    assert (lib.JIT_API_SP_TACTICAL, lib.JIT_API_SP_TACTICAL_DRAW, lib.JIT_API_SAMPLE_TACTICAL, lib.JIT_API_COUNT) == (19, 20, 23, 24)
    assert lib.jit_api_tactical_draw_kind(None) == 22
    consts = header_constants()
    assert consts["MNK_JIT_API_SP_TACTICAL"] == "19" and consts["MNK_JIT_API_SAMPLE_TACTICAL"] == "23"
    assert consts["MNK_JIT_API_COUNT"] == "24"


def test_tactical_kernels_specialise_at_run_time_without_a_gpu(lib):
    import torch

    handle = lib.load()
    tactical = (lib.JIT_API_SP_TACTICAL, lib.JIT_API_SAMPLE_TACTICAL)
    boards = {(12, 12, 5): tactical + tuple(lib.jit_api_tactical_draw_kind(d) for d in (torch.float32, torch.bfloat16, None)),
              (6, 7, 4): tactical + (lib.jit_api_tactical_draw_kind(None),),
              (10, 33, 5): tactical,                                                      # rows of more than 31 cells
              (25, 25, 5): tactical + (lib.jit_api_tactical_draw_kind(torch.float32),)}  # 21 words, 625 cells
    for (m, n, k), kinds in boards.items():
        for kind in kinds:
            size = handle.mnk_jit_compile_api(m, n, k, kind)
            assert size > 4096, (m, n, k, kind, (handle.mnk_jit_last_error() or b"").decode())


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """null state, bad geometry and a bad dtype are host-side errors (the fake device pointers are never dereferenced:
    nothing is launched when a check fails, and N = 0 launches nothing either)"""
    h = lib.load()
    p = 0x1000  # a non-NULL pointer that must never be touched
    step = lambda fn, planes, m=9, n=9, k=5, obs_dtype=0, actions=p, N=8: getattr(h, fn)(
        planes, p, N, m, n, k, actions, p, p, None, 1, 2, None, 0, p, p, None, obs_dtype, None, None, None, None, None, None, 0,
        None)
    for fn in ("mnk_selfplay_step_tactical",):
        assert step(fn, None) == -1
        assert step(fn, p, actions=None) == -1
        assert step(fn, p, obs_dtype=7) == -1
        assert step(fn, p, k=6, m=5, n=5) == -2
        assert step(fn, p, n=1) == -2
        assert step(fn, p, N=0) == 0
    logits = lambda planes, mask=p, dtype=0, N=8, acts=p: h.mnk_selfplay_step_tactical_logits(
        planes, p, N, 9, 9, 5, None, dtype, mask, 1, None, 0, None, 0, 0, acts, None, p, p, None, 1, 2, None, 0, p, p, None, 0,
        None, None, None, None, None, None, 0, None)
    assert logits(None) == -1 and logits(p, mask=None) == -1 and logits(p, acts=None) == -1 and logits(p, dtype=5) == -1
    assert logits(p, N=0) == 0
    sample = lambda obs, dtype=0, m=9, n=9, k=5, acts=p, N=8: h.mnk_sample_tactical(
        obs, dtype, N, m, n, k, 1, None, 0, None, 0, 0, acts, None, None)
    assert sample(None) == -1 and sample(p, acts=None) == -1 and sample(p, dtype=3) == -1 and sample(p, dtype=-1) == -1
    assert sample(p, N=-1) == -1
    assert sample(p, k=10) == -2 and sample(p, m=40, n=40) == -2
    assert sample(p, N=0) == 0
