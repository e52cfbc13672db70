"""CPU: the constructors of tests/line_cases.py -- positions that take every line and every would-be wrap of a board
through a rollout (one free cell) and through a replayed action log (forced sequences).

1. Coverage: no line is left out on any board with k >= 3, no wrap with k >= 4; the k = 3 boards leave out at most the
   wraps counted in ``K3_WRAPS_LEFT_OUT`` (printed); k <= 2 has no one-free-cell cases.
2. The oracle agrees with the brute-force rule on all of them: ``step``, ``random_rollout`` (whose draw must find the one
   free cell) and ``replay_actions`` win exactly where the rule does, black and white -- on the built-in boards and on
   boards with k = 1 ... 16, the first wins the oracle meets at k >= 8.
3. The cases have teeth: restated scans with one planted defect are rejected.
"""
import numpy as np
import pytest
import torch

import line_cases as lc
import line_rule as lr
import test_line_rule_cpu as tl
from oracle.env_torch import OracleVectorEnv
from oracle.rollout import random_rollout, replay_actions

BOARDS = lr.sibling_boards() + lc.OFF_LIST
FILLED = [b for b in BOARDS if b[2] >= 3]


def test_the_board_table():
    assert len(set(BOARDS)) == len(BOARDS)
    assert not set(lc.OFF_LIST) & set(lr.sibling_boards())
    assert {b[2] for b in lc.OFF_LIST} == {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16}
    assert all(lr.words(m, n) <= 16 for m, n, _ in BOARDS) and lr.words(22, 17) == 13 and lr.words(22, 22) == 16


def test_no_line_is_left_out_and_no_wrap_with_k_of_four_or_more():
    for board in FILLED:
        m, n, k = board
        cs = lr.cases(m, n, k)
        keep, mine, theirs, free, wins, left = lc.one_free_cell(m, n, k)
        assert len(keep) + len(left) == len(cs) and np.array_equal(wins, np.array([cs[i][1] for i in keep]))
        assert not any(cs[i][1] for i in left), (board, [cs[i] for i in left if cs[i][1]][:4])
        allowed = lc.K3_WRAPS_LEFT_OUT.get(board, 0) if k == 3 else 0
        print(f"{m}x{n}x{k}: {int(wins.sum())} lines and {int((~wins).sum())} wraps filled, {len(left)} wraps left out (at most {allowed})")
        assert len(left) <= allowed, (board, len(left))
        assert wins.any() and not wins.all()
        # what the constructor promises, restated with the one-plane rule on a sample of the cases
        for i in list(range(0, len(keep), max(1, len(keep) // 7)))[:8]:
            a, b = mine[i].reshape(m, n), theirs[i].reshape(m, n)
            assert not lr.has_line(a, k) and not lr.has_line(b, k) and not a.reshape(-1)[free[i]] and not b.reshape(-1)[free[i]]
            after = a.copy()
            after.reshape(-1)[free[i]] = True
            assert lr.has_line(after, k) == bool(wins[i]) and set(cs[keep[i]][0]) <= set(np.flatnonzero(after.reshape(-1)))
    for k in (1, 2):
        with pytest.raises(ValueError):
            lc.one_free_cell(5, 5, k)


@pytest.mark.parametrize("m,n,k", FILLED)
def test_oracle_on_the_one_free_cell_boards(m, n, k):
    """``step`` with the free cell as the move and ``random_rollout`` over one ply, with the counters at the stone count
    (the last cell: a win or a draw) and at k - 1 (done == win)"""
    keep, mine, theirs, free, wins, _ = lc.one_free_cell(m, n, k)
    c, nenv = m * n, len(keep)
    for side in (0, 1):
        for counts in (c - 1, k - 1):
            for how in ("step", "rollout"):
                env = OracleVectorEnv(m, n, k, nenv)
                env.boards.copy_(torch.from_numpy(lc.boards_of(mine, theirs, side, m, n)))
                env.current_player[:] = side
                env.move_counts[:] = counts
                if how == "step":
                    _, rew, done = env.step(torch.from_numpy(free.copy()))
                    rew, done = rew.numpy(), done.numpy()
                else:
                    _, meta, stats = random_rollout(env, seed=3, step0=0, steps=1, env_id0=5)
                    assert np.array_equal((meta[0] & 0xFFFF).astype(np.int64), free), (m, n, k, side, how)
                    rew, done = ((meta[0] >> 16) & 0xFF).astype(np.float32), ((meta[0] >> 24) & 1).astype(bool)
                    nwin = int(wins.sum())
                    full = counts == c - 1
                    assert stats.tolist() == [nenv if full else nwin, nwin * (1 - side), nwin * side, (nenv - nwin) * full,
                                              (nenv if full else nwin) * (counts + 1)]
                wrong = np.flatnonzero((rew == 1.0) != wins)
                assert wrong.size == 0, (m, n, k, side, how, [lr.cases(m, n, k)[keep[i]] for i in wrong[:4]])
                assert np.array_equal(done, wins | (counts == c - 1))


@pytest.mark.parametrize("m,n,k", BOARDS)
def test_oracle_replay_of_the_forced_sequences(m, n, k):
    cs = lr.cases(m, n, k)
    wins = np.array([w for _, w in cs])
    for side in (0, 1):
        if k == 1 and side == 1:
            with pytest.raises(ValueError):
                lc.sequences(m, n, k, side)
            continue
        acts = lc.sequences(m, n, k, side)
        t_done = lc.completing_ply(k, side)
        assert acts.shape == (lc.sequence_length(k, side), len(cs)) and acts.shape[0] % 4 == 0 and acts.shape[0] >= t_done + 3
        assert np.array_equal(acts[side:t_done + 1:2].T, np.array([cells for cells, _ in cs]))
        planes, meta = replay_actions(OracleVectorEnv(m, n, k, len(cs)), acts.copy())
        done, rew, mover = (meta >> 24) & 1, (meta >> 16) & 0xFF, (meta >> 25) & 1
        assert not done[:t_done].any() and (mover[t_done] == side).all()
        wrong = np.flatnonzero((rew[t_done] == 1) != wins)
        assert wrong.size == 0, (m, n, k, side, [cs[i] for i in wrong[:4]])
        assert np.array_equal(done[t_done] == 1, wins)
        # every ply was legal: the board before it (the record row, mover's word | other's word << 32) has the cell free
        bit = acts + acts // n
        occ = (planes & np.uint64(0xFFFFFFFF)) | (planes >> np.uint64(32))
        at = np.take_along_axis(occ, (bit >> 5)[:, None, :], axis=1)[:, 0, :]
        assert not ((at >> (bit & 31).astype(np.uint64)) & np.uint64(1)).any(), (m, n, k, side)
        if k > 3:  # the padding is quiet (with k <= 3 a crowded small board may have no quiet cell left)
            assert not done[t_done + 1:].any()


# ----------------------------------------------------------------------------- planted defects
def scan_top_word_dropped(plane, k):
    m, n = plane.shape
    keep = (1 << (32 * (lr.words(m, n) - 1))) - 1
    return tl._runs(tl._bits(plane, n + 1) & keep, (1, n, n + 1, n + 2), k)


def scan_blind_from_eight(plane, k):
    return k < 8 and tl.scan_good(plane, k)


def run_doubling(plane, k, tail=True):
    """``bs_has_run`` restated on one big integer: doubling steps while 2 len <= k, then the AND with the plane itself
    where len + 1 == k, else the general tail by (k - len) d -- which ``tail=False`` leaves out as a scan that finds nothing"""
    n = plane.shape[1]
    b = tl._bits(plane, n + 1)
    for d in (1, n + 1, n + 2, n):
        x, length = b, 1
        while 2 * length <= k:
            x &= x >> (length * d)
            length *= 2
        if length + 1 == k:
            x &= b >> (length * d)
        elif length < k:
            x = x & (x >> ((k - length) * d)) if tail else 0
        if x:
            return True
    return False


TAIL = {b for b in BOARDS if b[2] & (b[2] - 1) and b[2] not in (3, 5, 9)}  # neither a power of two nor one more


def test_wrong_scans_are_rejected_by_the_rule_and_by_the_filled_boards():
    assert TAIL == {(22, 6, 6), (7, 9, 7), (22, 22, 10), (16, 21, 12)}
    mutants = {"flat index": tl.scan_no_guard, "top word dropped": scan_top_word_dropped, "blind from k = 8": scan_blind_from_eight,
               "no general tail": lambda p, k: run_doubling(p, k, tail=False)}
    rejected = {name: set() for name in mutants}
    for board in BOARDS:
        m, n, k = board
        assert lr.check_scan(run_doubling, m, n, k) == [] and lr.check_scan(tl.scan_good, m, n, k) == []
        for name, scan in mutants.items():
            bad = lr.check_scan(scan, m, n, k)
            missed = {cells for cells, want, _ in bad if want}
            if k >= 3 and missed:  # a line the scan misses on the sparse board stays missed on the filled one
                keep, mine, _, free, _, _ = lc.one_free_cell(m, n, k)
                cs = lr.cases(m, n, k)
                for i in [i for i in range(len(keep)) if cs[keep[i]][0] in missed][:40]:
                    after = mine[i].copy()
                    after[free[i]] = True
                    assert not scan(after.reshape(m, n), k), (board, name, cs[keep[i]])
            if bad:
                rejected[name].add(board)
    assert rejected["flat index"] == {b for b in BOARDS if b[2] >= 2}
    assert rejected["blind from k = 8"] == {b for b in BOARDS if b[2] >= 8} and len(rejected["blind from k = 8"]) == 5
    assert rejected["no general tail"] == TAIL
    assert rejected["top word dropped"] == set(BOARDS)
