"""Generate tests/golden/tactical_positions.npz from the imported reference.

Run in the build container only (the reference is mounted there):  python tests/golden/make_golden_tactical.py

Positions reached by uniformly random play on 3x3x3, 4x6x3, 6x7x4, 9x9x5 and 19x19x5 (plies drawn over the whole game,
so near-terminal positions with threats on the board are common) and, for every position and every legal cell, whether
the REFERENCE env (env/torch_vector_mnk_env.py:55-84, win test :106-119) declares a win when that cell is played on a
copy -- by the side to move (``win_mover``, the set W of the tactical rule) and by the other side (``win_other``, the set
B).  Only data is stored: positions bit-packed in the layout of ``oracle/packing.py`` (``<b>_planes``, canonical view:
plane 0 = the side to move), the two sets as u8 [P][C].
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.packing import pack_boards  # noqa: E402
from oracle.pin_against_reference import import_reference  # noqa: E402

BOARDS = {(3, 3, 3): 300, (4, 6, 3): 300, (6, 7, 4): 300, (9, 9, 5): 300, (19, 19, 5): 120}


def reference_wins(RefEnv, m, n, k, obs, mover_plane):
    """u8 [P, C]: for each position and legal cell, does the reference env declare a win for the owner of plane
    ``mover_plane`` of ``obs`` after that cell is played on a copy of the position"""
    p, c = obs.shape[0], m * n
    out = np.zeros((p, c), dtype=np.uint8)
    for i in range(p):
        legal = np.flatnonzero(((obs[i, 0] == 0) & (obs[i, 1] == 0)).reshape(-1))
        if legal.size == 0:
            continue
        env = RefEnv(m, n, k, num_envs=legal.size, device="cpu")
        env.boards[:, 0] = torch.from_numpy(obs[i, mover_plane]).float()   # the side that plays = black here
        env.boards[:, 1] = torch.from_numpy(obs[i, 1 - mover_plane]).float()
        env.current_player.zero_()
        env.move_counts.fill_(int(obs[i].sum()))
        _, rewards, _ = env.step(torch.from_numpy(legal).long())
        out[i, legal] = (rewards.numpy() == 1.0).astype(np.uint8)
    return out


def main():
    from tactical_rule import random_positions

    RefEnv, _, _ = import_reference()
    rng = np.random.default_rng(20261015)
    data = {}
    for (m, n, k), count in BOARDS.items():
        obs = random_positions(m, n, k, count, rng, stop_at_win=True)
        tag = f"{m}x{n}x{k}"
        data[tag + "_planes"] = pack_boards(obs, m, n)
        data[tag + "_win_mover"] = reference_wins(RefEnv, m, n, k, obs, 0)
        data[tag + "_win_other"] = reference_wins(RefEnv, m, n, k, obs, 1)
        print(tag, count, "positions;", int(data[tag + "_win_mover"].any(1).sum()), "with a winning cell,",
              int(data[tag + "_win_other"].any(1).sum()), "with a cell to block")
    data["boards"] = np.array([[m, n, k] for (m, n, k) in BOARDS], dtype=np.int64)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "tactical_positions.npz"), **data)


if __name__ == "__main__":
    main()
