"""numpy restatement of the one-ply tactical player (test helper; the rule is stated in include/mnk_hip.h).

For the side to move: W = the legal cells where its stone leaves a run of >= k of its stones through that cell, B = the
same for the other side, S = W if W is not empty, else B if that is not empty, else the legal cells (all C cells on a full
board); the move is the r-th cell of S in action order with r = mulhi32(x, |S|) -- ``oracle.philox.pick_legal`` over the
mask of S.  The run test here counts stones outward from the cell along each of the four directions, a formulation of its
own (the kernels AND shifted bit strings); tests/golden/tactical_positions.npz pins it to the reference env's win test.
"""
import numpy as np
import torch

from oracle import philox

_DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))


def _shift(a, dr, dc):
    """out[:, r, c] = a[:, r + dr, c + dc], False outside the board"""
    out = np.zeros_like(a)
    _, m, n = a.shape
    r0, r1 = max(0, -dr), min(m, m - dr)
    c0, c1 = max(0, -dc), min(n, n - dc)
    if r0 < r1 and c0 < c1:
        out[:, r0:r1, c0:c1] = a[:, r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def _as_bool(obs) -> np.ndarray:
    if isinstance(obs, torch.Tensor):
        obs = obs.float().cpu().numpy()
    return np.asarray(obs) != 0


def completions(stones: np.ndarray, empty: np.ndarray, k: int) -> np.ndarray:
    """bool [B, m, n]: the empty cells where one more stone of ``stones`` makes a run of >= k through that cell"""
    stones = np.asarray(stones, dtype=bool)
    hit = np.zeros_like(stones)
    for dr, dc in _DIRS:
        count = np.zeros(stones.shape, dtype=np.int64)
        for sgn in (1, -1):
            run = np.ones_like(stones)
            for j in range(1, k):
                run &= _shift(stones, sgn * j * dr, sgn * j * dc)
                count += run
        hit |= count + 1 >= k
    return hit & np.asarray(empty, dtype=bool)


def tactical_sets(obs, k: int):
    """obs: [B, 2, m, n] canonical view (channel 0 = the side to move; non-zero = stone), numpy or torch.
    Returns (S, W, B) as bool [B, C]"""
    obs = _as_bool(obs)
    b, _, m, n = obs.shape
    mine, theirs = obs[:, 0], obs[:, 1]
    legal = ~(mine | theirs)
    win = completions(mine, legal, k).reshape(b, m * n)
    block = completions(theirs, legal, k).reshape(b, m * n)
    legal = legal.reshape(b, m * n)
    s = np.where(win.any(axis=1, keepdims=True), win, np.where(block.any(axis=1, keepdims=True), block, legal))
    s = np.where(s.any(axis=1, keepdims=True), s, True)  # full board: all C cells
    return s, win, block


def tactical_moves(obs, k: int, x) -> np.ndarray:
    """the moves drawn with one u32 per row (x = 0: deterministic, the first cell of S)"""
    s, _, _ = tactical_sets(obs, k)
    return philox.pick_legal(s, np.broadcast_to(np.asarray(x, dtype=np.uint64), (s.shape[0],)))


class PhiloxTacticalOpponent:
    """The tactical reply keyed by (seed, global env id, step) on stream OPP: what the one-launch step
    ``mnk_selfplay_step_tactical`` plays for its built-in opponent (``oracle.policies.PhiloxOpponent`` with the tactical
    set in place of the legal one).  ``OracleSelfPlay`` hands the env indices through ``act_indexed``; the test sets
    ``step`` before every wrapper call."""

    def __init__(self, k: int, seed: int, env_id0: int = 0):
        self.k, self.seed, self.env_id0, self.step = int(k), int(seed), int(env_id0), 0

    def act_indexed(self, obs, idx):
        ids = (idx.numpy() + self.env_id0).astype(np.uint64)
        x = philox.rand_u32(self.seed, ids, self.step, philox.STREAM_OPP)
        return torch.from_numpy(tactical_moves(obs["observation"], self.k, x))


def random_positions(m: int, n: int, k: int, count: int, rng, max_fill: float = 1.0, stop_at_win: bool = True):
    """canonical observations [count, 2, m, n] (float32) reached by uniformly random play from the empty board, with a
    random number of plies each (up to max_fill * m * n); a game that is won stops before the winning ply is recorded
    (when stop_at_win), so positions with threats on the board are common near the end"""
    c = m * n
    out = np.zeros((count, 2, m, n), dtype=np.float32)
    for i in range(count):
        board = np.zeros((2, m, n), dtype=bool)
        plies = int(rng.integers(0, int(max_fill * c) + 1))
        side = 0
        for _ in range(plies):
            free = np.flatnonzero(~(board[0] | board[1]).reshape(-1))
            if free.size == 0:
                break
            cell = int(rng.choice(free))
            trial = board.copy()
            trial[side].reshape(-1)[cell] = True
            if stop_at_win and completions(board[side][None], ~(board[0] | board[1])[None], k).reshape(-1)[cell]:
                break
            board = trial
            side ^= 1
        out[i, 0] = board[side]
        out[i, 1] = board[side ^ 1]
    return out
