"""Positions that take every line and every would-be wrap of a board (tests/line_rule.py) through a ROLLOUT kernel and
through the replay of an action log (test helper; numpy only).

A rollout draws its own moves, so a case cannot hand it the completing cell.  Two constructions get round that:

  one free cell     a board that is full but for ``cells[-1]``: the mover holds ``cells[:-1]``, every other cell takes a
                    two-colour periodic filler.  The draw has one legal cell, so any random word picks it (the trick of
                    test_sample_legal_reaches_every_cell_and_every_rank) -- in every kernel form, the ones that cannot be
                    fed actions included.  A filler is accepted for a case only if the brute-force rule says that neither
                    colour holds a line before the move and that the mover holds one after it iff the case wins.
  forced sequence   an action log from the empty board: the winner-to-be plays ``cells`` in order, the other side plays
                    quiet cells (none on ``cells``, no line for it), then a few quiet plies pad the log to a multiple of
                    four (the log's word).  After a win the game has restarted, so the padding is chosen on the oracle's
                    own state.

The rule is ``line_rule.lines`` (cells enumerated, nothing shifted or convolved), evaluated for many planes at once.
"""
import functools

import numpy as np

import line_rule as lr

# Boards without a built-in kernel variant, one or more per path of the run-doubling scan (bs_has_run, csrc/mnk_device.h):
# k a power of two (doubling steps only), len + 1 == k (k = 3, 5, 9: AND with the plane itself), the general tail
# ((k - len) * d) -- and k = 1, where the scan has no step at all
OFF_LIST = [(5, 5, 1), (2, 22, 2), (22, 2, 2), (9, 9, 4), (9, 19, 8), (22, 17, 16),  # 22x17: 13 words, word moves of 4
            (3, 61, 3),                                                               # a 62-bit row: shifts >= 32 at len = 1
            (12, 12, 5), (9, 9, 9), (22, 6, 6), (7, 9, 7), (22, 22, 10), (16, 21, 12)]
# the most wraps of a k = 3 board that no filler of ``fillers`` may leave unfilled (every line fills on every board, and
# every wrap with k >= 4); the forced sequences cover them
K3_WRAPS_LEFT_OUT = {(4, 6, 3): 12, (3, 61, 3): 2, **{(m, 3, 3): 2 * (m - 3) for m in range(3, 9)}}


@functools.lru_cache(maxsize=None)
def _line_index(m: int, n: int, k: int) -> np.ndarray:
    return np.array(lr.lines(m, n, k), dtype=np.int64).reshape(-1, k)


def holds_line(planes, m: int, n: int, k: int) -> np.ndarray:
    """``lr.has_line`` for a batch: planes bool [B, m * n] -> bool [B]"""
    planes = np.asarray(planes).reshape(len(planes), m * n) != 0
    idx = _line_index(m, n, k)
    out = np.zeros(len(planes), dtype=bool)
    for lo in range(0, len(planes), 256):  # (bounds the [B, lines, k] gather)
        out[lo:lo + 256] = planes[lo:lo + 256][:, idx].all(axis=2).any(axis=1)
    return out


# ----------------------------------------------------------------------------- a. one free cell
def fillers(m: int, n: int, k: int):
    """[(name, bool [m * n])]: two-colour periodic patterns, True = the mover's colour, either colour as the mover's.
    (a r + b c + s) mod 4 < 2 has no run longer than two in a direction whose step changes it; k = 3 adds patterns of
    period two and 2 x 2 blocks shifted row by row, whose runs are one or two long."""
    r, c = np.divmod(np.arange(m * n), n)
    out = []
    for a, b in ((1, 2), (2, 1), (1, 1), (1, 3), (3, 1), (1, 0), (0, 1), (2, 3), (3, 2)):
        for s in range(4):
            out.append((f"({a}r+{b}c+{s})%4<2", (a * r + b * c + s) % 4 < 2))
    if k == 3:
        for s in range(2):
            out.append((f"(r+c+{s})%2", (r + c + s) % 2 == 0))
            out.append((f"(r+{s})%2", (r + s) % 2 == 0))
            out.append((f"(c+{s})%2", (c + s) % 2 == 0))
            for t in range(2):
                out.append((f"((r+{s})//2+c+{t})%2", ((r + s) // 2 + c + t) % 2 == 0))
                out.append((f"(r+(c+{s})//2+{t})%2", (r + (c + s) // 2 + t) % 2 == 0))
                for u in range(2):
                    out.append((f"((r+{s})//2+(c+{t})//2+{u})%2", ((r + s) // 2 + (c + t) // 2 + u) % 2 == 0))
    return out + [(f"not {name}", ~p) for name, p in out]


@functools.lru_cache(maxsize=None)
def one_free_cell(m: int, n: int, k: int):
    """One position per case of ``lr.cases`` that some filler fills.

    Returns (index, mine, theirs, free, wins, left_out): ``index`` int [B] into ``lr.cases(m, n, k)``; ``mine`` /
    ``theirs`` bool [B, m * n], the mover's and the other side's stones -- together every cell but ``free`` [B]; ``wins``
    bool [B], the rule's verdict on the mover's move to ``free``; ``left_out`` the indices no filler fills."""
    if k < 3:
        raise ValueError("no full board is free of runs of two: k <= 2 has no one-free-cell cases")
    cs = lr.cases(m, n, k)
    c = m * n
    ncase = len(cs)
    hold = np.zeros((ncase, c), dtype=bool)
    for i, (cells, _) in enumerate(cs):
        hold[i, list(cells[:-1])] = True
    free = np.array([cells[-1] for cells, _ in cs], dtype=np.int64)
    wins = np.array([w for _, w in cs], dtype=bool)
    mine = np.zeros((ncase, c), dtype=bool)
    theirs = np.zeros((ncase, c), dtype=bool)
    todo = np.ones(ncase, dtype=bool)
    rows = np.arange(ncase)
    for _, pattern in fillers(m, n, k):
        if not todo.any():
            break
        at = np.flatnonzero(todo)
        a = hold[at] | pattern[None, :]
        a[np.arange(len(at)), free[at]] = False
        b = ~a
        b[np.arange(len(at)), free[at]] = False
        after = a.copy()
        after[np.arange(len(at)), free[at]] = True
        ok = ~holds_line(a, m, n, k) & ~holds_line(b, m, n, k) & (holds_line(after, m, n, k) == wins[at])
        mine[at[ok]], theirs[at[ok]] = a[ok], b[ok]
        todo[at[ok]] = False
    keep = rows[~todo]
    assert ((mine[keep] | theirs[keep]).sum(axis=1) == c - 1).all() and not (mine[keep] & theirs[keep]).any()
    out = (keep, mine[keep], theirs[keep], free[keep], wins[keep], rows[todo])
    for a in out:
        a.setflags(write=False)  # (cached: shared by the tests)
    return out


def boards_of(mine, theirs, side: int, m: int, n: int) -> np.ndarray:
    """dense f32 [B, 2, m, n] with the mover's stones in plane ``side``"""
    out = np.zeros((len(mine), 2, m * n), dtype=np.float32)
    out[:, side] = mine
    out[:, 1 - side] = theirs
    return out.reshape(len(mine), 2, m, n)


# ----------------------------------------------------------------------------- b. forced sequences
def completing_ply(k: int, side: int) -> int:
    """the ply (from 0) at which ``side`` places its k-th stone when both sides alternate from the empty board"""
    return 2 * (k - 1) + side


def sequence_length(k: int, side: int) -> int:
    """plies of a forced log: the completing ply, at least two more, a multiple of four"""
    return (completing_ply(k, side) + 3 + 3) // 4 * 4


def quiet_cells(m: int, n: int, k: int, avoid, count: int):
    """``count`` cells off ``avoid`` that hold no line together (the rule), lowest first"""
    plane = np.zeros(m * n, dtype=bool)
    out = []
    for cell in range(m * n):
        if len(out) == count:
            break
        if cell in avoid:
            continue
        plane[cell] = True
        if holds_line(plane[None], m, n, k)[0]:
            plane[cell] = False
        else:
            out.append(cell)
    if len(out) < count:
        raise ValueError(f"{m}x{n}x{k}: no {count} quiet cells off {sorted(avoid)}")
    return out


def forced_sequences(m: int, n: int, k: int, side: int, step):
    """Action logs int64 [T, B], one column per case of ``lr.cases``: ``side`` (0 black, 1 white) plays the case's cells
    in order and completes them at ply ``completing_ply(k, side)``; the other side plays quiet cells; the plies after
    that are quiet legal cells of the position ``step`` reports.

    ``step(actions int64 [B]) -> (boards f32 [B, 2, m, n], side to move int64 [B])`` plays one ply on a fresh env batch
    of B games that restarts finished games (the oracle: the caller wraps ``OracleVectorEnv``).  White cannot complete
    anything with k = 1 (black's first stone ends the game): ``ValueError``."""
    if k == 1 and side == 1:
        raise ValueError("k = 1: the first stone wins, white never completes a line")
    cs = lr.cases(m, n, k)
    c = m * n
    t_done, total = completing_ply(k, side), sequence_length(k, side)
    acts = np.zeros((total, len(cs)), dtype=np.int64)
    others = k - 1 + side  # quiet plies of the other side before the completing ply
    for i, (cells, _) in enumerate(cs):
        quiet = quiet_cells(m, n, k, set(cells), others)
        for j in range(k):
            acts[2 * j + side, i] = cells[j]
        for j in range(others):
            acts[2 * j + 1 - side, i] = quiet[j]
    boards, mover = None, None
    for t in range(total):
        if t > t_done:  # padding: the lowest legal cell that gives its mover no line; none such: the lowest legal cell
            flat = boards.reshape(len(cs), 2, c) != 0
            legal = ~flat.any(axis=1)
            own = flat[np.arange(len(cs)), mover]
            pick = np.where(legal.any(axis=1), legal.argmax(axis=1), 0)
            todo = legal.any(axis=1)
            tried = np.zeros_like(legal)
            while todo.any():
                at = np.flatnonzero(todo)
                cand = (legal[at] & ~tried[at])
                none = ~cand.any(axis=1)
                cell = cand.argmax(axis=1)
                trial = own[at].copy()
                trial[np.arange(len(at)), cell] = True
                good = ~holds_line(trial, m, n, k) & ~none
                pick[at[good]] = cell[good]
                tried[at, cell] = True
                todo[at[good | none]] = False
            acts[t] = pick
        boards, mover = step(acts[t])
    return acts


@functools.lru_cache(maxsize=None)
def sequences(m: int, n: int, k: int, side: int) -> np.ndarray:
    """``forced_sequences`` with the padding chosen on ``OracleVectorEnv`` (step, then reset of the finished games: the
    loop of ``oracle.rollout.replay_actions``); read-only, shared by the tests"""
    import torch

    from oracle.env_torch import OracleVectorEnv

    env = OracleVectorEnv(m, n, k, len(lr.cases(m, n, k)))

    def step(actions):
        _, _, done = env.step(torch.from_numpy(actions))
        if bool(done.any()):
            env.reset(torch.nonzero(done).squeeze(1))
        return env.boards.numpy(), env.current_player.numpy()

    acts = forced_sequences(m, n, k, side, step)
    acts.setflags(write=False)
    return acts
