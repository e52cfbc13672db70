"""numpy restatement of the flat Monte Carlo player (test helper; the rule is stated in include/mnk_hip.h).

For every legal cell a of a row and every j in [0, P): "me" (channel 0) plays a, then the sides alternate starting with the
other side, each playing ``oracle.philox.pick_legal`` over its legal cells with the u32 of
``u = (((step * C + a) * P + j) * C4) + t`` on stream PLAYOUT (t = 0: the other side's first reply, C4 = C rounded up to a
multiple of 4).  The game ends at the first ply after which the mover has a run of >= k stones anywhere on its plane, or
when the board is full.  W / Lo = wins / losses of "me"; the move is ``pick_legal`` over the legal cells of maximal
W - Lo with the row's u32 of stream SAMPLE at ``step``.

The win test here looks for k stones in a row over the mover's WHOLE plane, along the four directions, with array shifts
-- a formulation of its own (the kernels AND shifted bit strings).  Scanning the whole plane matters on finished games,
which ``tournament.play_batch_games`` also hands to ``act``: a run already on the board ends the playout at its owner's
next ply.  All games of a call are played together, vectorised over (row, cell, playout); games leave the batch as they
end.
"""
import numpy as np

from oracle import philox
from tactical_rule import _DIRS, _as_bool, _shift

STREAM_PLAYOUT = 4  # MNK_STREAM_PLAYOUT of include/mnk_hip.h


def has_run(plane: np.ndarray, k: int) -> np.ndarray:
    """bool [G]: does plane [G, m, n] hold k stones in a row anywhere (rows, columns, diagonals, anti-diagonals)?"""
    hit = np.zeros(plane.shape[0], dtype=bool)
    for dr, dc in _DIRS:
        run = plane.copy()  # run[r, c]: the k cells from (r, c) along (dr, dc) are all stones
        for j in range(1, k):
            run &= _shift(plane, j * dr, j * dc)
        hit |= run.reshape(len(run), -1).any(axis=1)
    return hit


def random_games(flat, side0, live, m: int, n: int, k: int, seed: int, env, base, stream: int):
    """Plays the games ``live`` (indices into ``flat``, bool [G, 2, C], updated in place) to their ends, all together: at
    its ply t a game's mover, side ``(side0 + t) & 1``, plays ``oracle.philox.pick_legal`` over the free cells with the
    u32 of ``u = base + t`` on ``stream`` (``side0`` / ``env`` / ``base``: per game).  A game ends at the first ply after
    which the mover has a run of >= k on its whole plane, or when the board is full; it leaves the batch then.
    Returns (winner int64 [G]: 1 + the side that won, 0 for a draw or a game not played here; plies played)."""
    C = m * n
    winner = np.zeros(len(flat), np.int64)
    t = played = 0
    while len(live):
        played += len(live)
        sub = flat[live]
        mover = (side0[live] + t) & 1
        free = ~(sub[:, 0] | sub[:, 1])
        x = philox.rand_u32(seed, env[live], base[live] + np.uint64(t), stream)
        a = philox.pick_legal(free, x)
        idx = np.arange(len(live))
        sub[idx, mover, a] = True
        flat[live] = sub
        won = has_run(sub[idx, mover].reshape(len(live), m, n), k)
        winner[live[won]] = 1 + mover[won]
        full = sub[:, 0].sum(1) + sub[:, 1].sum(1) >= C
        live = live[~won & ~full]
        t += 1
    return winner, played


def playout_counts(obs, k: int, P: int, seed: int, step: int = 0, env_id0: int = 0, plies: list = None):
    """obs: [B, 2, m, n] canonical view (channel 0 = the side to move; non-zero = stone), numpy or torch.
    Returns (wins, losses) as int64 [B, C]: 0 on occupied cells.  ``plies`` (a list): receives the number of plies
    played, the first ply of every playout included."""
    obs = _as_bool(obs)
    b, _, m, n = obs.shape
    C = m * n
    C4 = (C + 3) // 4 * 4
    legal = ~(obs[:, 0] | obs[:, 1]).reshape(b, C)
    rows, cells = np.nonzero(legal)                           # (row, cell) pairs in action order
    g_row = np.repeat(rows, P)
    g_cell = np.repeat(cells, P)
    g_j = np.tile(np.arange(P), len(rows))
    G = len(g_row)
    wins = np.zeros((b, C), dtype=np.int64)
    losses = np.zeros((b, C), dtype=np.int64)
    if G == 0:
        return wins, losses
    base = (((np.uint64(step) * np.uint64(C) + g_cell.astype(np.uint64)) * np.uint64(P) + g_j.astype(np.uint64))
            * np.uint64(C4))
    env = (np.int64(env_id0) + g_row).astype(np.uint64)
    # planes [G, 2, m, n]: 0 = "me", 1 = the other side; ply -1: "me" plays its cell
    planes = obs[g_row].copy()
    flat = planes.reshape(G, 2, C)
    flat[np.arange(G), 0, g_cell] = True
    won = has_run(planes[:, 0], k)
    full = flat[:, 0].sum(1) + flat[:, 1].sum(1) >= C
    # t = 0: the other side (side 1) replies
    winner, played = random_games(flat, np.ones(G, np.int64), np.flatnonzero(~won & ~full), m, n, k, seed, env, base,
                                  STREAM_PLAYOUT)
    winner[won] = 1
    if plies is not None:
        plies.append(G + played)
    np.add.at(wins, (g_row, g_cell), winner == 1)
    np.add.at(losses, (g_row, g_cell), winner == 2)
    return wins, losses


def best_sets(obs, wins, losses) -> np.ndarray:
    """bool [B, C]: S = the legal cells of maximal W - Lo (empty on a full board)"""
    obs = _as_bool(obs)
    b, _, m, n = obs.shape
    legal = ~(obs[:, 0] | obs[:, 1]).reshape(b, m * n)
    score = np.where(legal, wins - losses, np.iinfo(np.int64).min)
    return legal & (score == score.max(axis=1, keepdims=True))


def playout_moves(obs, k: int, P: int, seed: int, step: int = 0, env_id0: int = 0, deterministic: bool = False):
    """(actions int64 [B], wins, losses): the player's moves on call ``step``"""
    wins, losses = playout_counts(obs, k, P, seed, step, env_id0)
    s = best_sets(obs, wins, losses)
    ids = np.int64(env_id0) + np.arange(s.shape[0], dtype=np.int64)
    x = np.zeros(s.shape[0], np.uint64) if deterministic else philox.rand_u32(seed, ids.astype(np.uint64), step,
                                                                              philox.STREAM_SAMPLE)
    return philox.pick_legal(s, x), wins, losses
