"""CPU: the flat Monte Carlo player -- the numpy restatement of the rule in tests/playout_rule.py against the reference's
own win test (tests/golden/tactical_positions.npz: a cell where the side to move wins at once is won by every playout and
always lies in S) and hand-built positions; the C ABI of ``mnk_sample_playouts`` (header, binding, host argument checks,
which reject before anything is enqueued)."""
import os

import numpy as np
import pytest

from oracle import philox
from oracle.packing import unpack_boards
from player_cases import board, check_header_and_binding, header_constants, lib  # noqa: F401 (lib: the fixture)
from playout_rule import STREAM_PLAYOUT, best_sets, has_run, playout_counts, playout_moves


# ----------------------------------------------------------------------------- the rule against the reference
@pytest.mark.parametrize("tag", ["3x3x3", "4x6x3", "6x7x4", "9x9x5", "19x19x5"])
def test_winning_cells_win_every_playout_and_lie_in_S(golden_dir, tag):
    """the cells where the REFERENCE env declared a win for the side to move (tests/golden/make_golden_tactical.py) have
    W == P and Lo == 0, and S holds them (the player never misses a win in one ply)"""
    data = np.load(os.path.join(golden_dir, "tactical_positions.npz"))
    m, n, k = (int(v) for v in tag.split("x"))
    obs = unpack_boards(data[tag + "_planes"], m, n)
    win = data[tag + "_win_mover"] != 0
    rows = np.flatnonzero(win.any(1))[:24]  # positions with a winning cell (a bounded number: the restatement is numpy)
    obs, win = obs[rows], win[rows]
    P = 3
    w, lo = playout_counts(obs, k, P, seed=11, step=2, env_id0=5)
    assert (w[win] == P).all() and (lo[win] == 0).all()
    s = best_sets(obs, w, lo)
    assert s[win].all()
    acts, _, _ = playout_moves(obs, k, P, seed=11, step=2, env_id0=5, deterministic=True)
    # the move scores P as a winning cell does (a cell that only happened to win its P playouts ties with it)
    assert ((w - lo)[np.arange(len(rows)), acts] == P).all()


# ----------------------------------------------------------------------------- hand-built positions
def test_full_board_draws_over_all_cells():
    full = board(["xox", "oxo", "oxo"])
    w, lo = playout_counts(full, 3, 8, seed=1)
    assert not w.any() and not lo.any() and not best_sets(full, w, lo).any()
    x = philox.rand_u32(1, np.zeros(1, np.uint64), 0, philox.STREAM_SAMPLE)
    acts, _, _ = playout_moves(full, 3, 8, seed=1)
    assert acts[0] == philox.mulhi32(x, 9)[0]      # r = mulhi32(x, C): cell r
    assert playout_moves(full, 3, 8, seed=1, deterministic=True)[0][0] == 0


def test_one_legal_cell():
    obs = board(["xox", "oxo", "o.o"])             # x to move, one cell left: it completes no run -- a draw
    P = 5
    w, lo = playout_counts(obs, 3, P, seed=2)
    assert w.sum() == 0 and lo.sum() == 0
    assert playout_moves(obs, 3, P, seed=2)[0][0] == 7
    obs = board(["xo.", "xo.", "..."])             # a win at (2, 0), and o wins at (2, 1) if it is left open
    w, lo = playout_counts(obs, 3, 16, seed=3)
    assert w[0, 6] == 16 and lo[0, 6] == 0


def test_single_immediate_win_is_always_taken():
    obs = board(["xx..", "oo.o", "....", "...."])  # 4x4x3: (0, 2) wins now; everything else lets o win at (1, 2) first
    for seed in range(4):
        acts, w, lo = playout_moves(obs, 3, 8, seed=seed, step=seed)
        assert acts[0] == 2 and w[0, 2] == 8 and lo[0, 2] == 0
        assert (w[0] - lo[0])[[c for c in range(16) if c != 2 and obs[0, :, c // 4, c % 4].sum() == 0]].max() < 8


def test_deterministic_pick_is_the_first_best_cell():
    obs = board(["x..", "...", "..o"])
    acts, w, lo = playout_moves(obs, 3, 32, seed=4, deterministic=True)
    s = best_sets(obs, w, lo)
    assert acts[0] == np.flatnonzero(s[0])[0]
    x = philox.rand_u32(4, np.zeros(1, np.uint64), 0, philox.STREAM_SAMPLE)
    assert playout_moves(obs, 3, 32, seed=4)[0][0] == philox.pick_legal(s, x)[0]


def test_finished_games_are_scanned_on_the_whole_plane():
    """a run of the other side already on the board: the first reply (t = 0) ends the playout with its win, whatever
    cell it plays -- a win test around the placed stone only would play on"""
    obs = board(["ooo.", "x...", "x...", "...."])   # 4x4x3: o already has three in a row
    w, lo = playout_counts(obs, 3, 6, seed=5)
    legal = (obs[0, 0] == 0) & (obs[0, 1] == 0)
    winning = np.zeros((4, 4), bool)
    winning[3, 0] = True                             # x completes its own column: a win at ply -1
    assert (w[0][winning.reshape(-1)] == 6).all()
    others = (legal & ~winning).reshape(-1)
    assert (lo[0][others] == 6).all() and (w[0][others] == 0).all()


def test_counter_layout_and_streams():
    """playout j of cell a draws its t-th reply at u = ((step * C + a) * P + j) * C4 + t on stream PLAYOUT (4): the
    other side's first reply on an empty 4x4 board after x takes cell a is pick_legal over the 15 free cells"""
    assert STREAM_PLAYOUT == 4
    obs = np.zeros((1, 2, 4, 4), np.float32)
    P, step, a, j = 3, 7, 5, 2
    u = ((step * 16 + a) * P + j) * 16
    x = philox.rand_u32(9, np.array([3], np.uint64), np.uint64(u), STREAM_PLAYOUT)
    free = np.ones((1, 16), bool)
    free[0, a] = False
    reply = philox.pick_legal(free, x)[0]
    assert reply != a and 0 <= reply < 16
    # with k = 1 every playout is won at ply -1 (the draws themselves are checked bit for bit against the kernel on the GPU)
    w, lo = playout_counts(obs, 1, P, seed=9, step=step, env_id0=3)
    assert (w == P).all() and not lo.any()


def test_has_run_counts_overlines_and_all_directions():
    p = np.zeros((5, 5, 5), bool)
    p[0, 1, 0:5] = True                        # a row of 5
    p[1, 0:4, 2] = True                        # a column of 4
    p[2, [0, 1, 2], [0, 1, 2]] = True          # a diagonal of 3
    p[3, [0, 1, 2], [4, 3, 2]] = True          # an anti-diagonal of 3
    p[4, 0, [0, 1, 3, 4]] = True               # a gap
    assert has_run(p, 4).tolist() == [True, True, False, False, False]
    assert has_run(p, 3).tolist() == [True, True, True, True, False]
    assert has_run(p, 2).tolist() == [True] * 5


def test_tic_tac_toe_centre_is_best_on_an_empty_board():
    acts, w, lo = playout_moves(np.zeros((1, 2, 3, 3), np.float32), 3, 256, seed=1, deterministic=True)
    assert acts[0] == 4 and (w[0] - lo[0]).argmax() == 4


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_mnk_sample_playouts_and_the_binding_matches(lib):
    check_header_and_binding(lib, "mnk_sample_playouts")
    assert lib.JIT_API_COUNT == 24
    consts = header_constants()
    assert consts["MNK_STREAM_PLAYOUT"] == "4" == str(lib.STREAM_PLAYOUT)
    assert consts["MNK_PLAYOUTS_MAX"] == "4096" == str(lib.PLAYOUTS_MAX)


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000  # a non-NULL pointer that must never be touched

    def sample(obs=p, dtype=0, N=8, m=9, n=9, k=5, P=64, step=0, acts=p):
        return lib.call("mnk_sample_playouts", obs, dtype, N, m, n, k, P, 1, None, step, None, 0, 0, acts, None, None)

    for bad in (dict(obs=None), dict(acts=None), dict(N=-1), dict(dtype=3), dict(dtype=-1), dict(P=0), dict(P=-5),
                dict(P=4097)):
        with pytest.raises(lib.MnkHipError, match="mnk_sample_playouts"):
            sample(**bad)
    # the counter range: q = u >> 2 < 2^56, i.e. (step + 1) * C * P * C4 <= 2^58
    per_step = 81 * 64 * 84
    with pytest.raises(lib.MnkHipError):
        sample(step=(1 << 58) // per_step)
    with pytest.raises(lib.MnkHipError):
        sample(step=(1 << 64) - 1)
    with pytest.raises(lib.MnkHipError):
        sample(m=3, n=3, k=3, P=4096, step=(1 << 58) // (9 * 4096 * 12))
    for geom in (dict(k=10), dict(m=40, n=40), dict(n=1, m=4, k=1)):
        with pytest.raises(lib.MnkHipError, match="geometry|status -2"):
            sample(**geom)
    assert sample(N=0) == 0
    assert sample(N=0, P=4096, step=(1 << 58) // per_step // 64 - 1) == 0
