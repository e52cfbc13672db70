"""GPU: the flat Monte Carlo player -- ``mnk_sample_playouts`` / ``MonteCarloPolicy.act`` bit for bit against the numpy
rule (tests/playout_rule.py) on built-in and generic boards, finished games included; ``tournament.play_match`` and the
strength ladder Random < Tactical < MC(16) < MC(64) < MC(256).  What it shares with the tree-search player:
test_gpu_players.py."""
import numpy as np
import pytest
import torch

from player_cases import MC, _score, hip, mostly_full, positions  # noqa: F401 (hip: the fixture)
from playout_rule import playout_moves
from tactical_rule import completions

pytestmark = pytest.mark.gpu
OBS_DTYPES = (torch.float32, torch.bfloat16, torch.uint8)


# ----------------------------------------------------------------------------- 1. bit for bit against the rule
@pytest.mark.parametrize("board,rows,ps", [((3, 3, 3), 40, (1, 3, 16)), ((9, 9, 5), 12, (3, 8)), ((19, 19, 5), 4, (3,)),
                                           ((4, 4, 3), 24, (1, 5, 7)), ((7, 9, 7), 8, (3, 4)),
                                           ((17, 17, 5), 5, (1, 3)), ((25, 25, 5), 5, (1, 3))])
def test_counts_and_actions_equal_the_rule(hip, board, rows, ps):
    """(3x3x3, 9x9x5, 19x19x5: built-in variants; 4x4x3, 7x9x7: the generic NW forms; 17x17x5, 25x25x5: those of sixteen
    and of thirty-two words, ten and 21 words a plane, from positions three quarters full -- the numpy rule plays every
    playout out, and from an empty 25x25 board that takes it seconds a row)"""
    m, n, k = board
    seed = m * 100 + n * 10 + k
    obs = mostly_full(m, n, k, rows, seed) if board in ((17, 17, 5), (25, 25, 5)) else positions(m, n, k, rows, seed)
    finished = [i for i in range(rows) if completions(obs[i:i + 1, 1], np.ones((1, m, n), bool), k).any()
                or completions(obs[i:i + 1, 0], np.ones((1, m, n), bool), k).any()]
    assert finished  # boards that already hold a run are in the comparison
    for P in ps:
        step, env_id0, seed = 3, 17, 1000 + P
        want_r, w, lo = playout_moves(obs, k, P, seed, step, env_id0)
        want_d, _, _ = playout_moves(obs, k, P, seed, step, env_id0, deterministic=True)
        want_counts = np.stack([w, lo], axis=1)
        for dtype in OBS_DTYPES:
            for det, want in ((False, want_r), (True, want_d)):
                got, counts = MC.act(hip, obs, k, (P,), seed, step, env_id0, dtype, det)
                assert np.array_equal(counts, want_counts), (P, dtype, det)
                assert np.array_equal(got, want), (P, dtype, det)


# ----------------------------------------------------------------------------- 2. the strength ladder
@pytest.mark.parametrize("board", [(9, 9, 5), (3, 3, 3)])
def test_strength_ordering(hip, board):
    """play_match scores of player 1 over 1024 games (half as black) with these seeds, as measured on the MI355X:
        9x9x5:  MC(64) vs Random 1.0000;  MC(64) vs Tactical 0.9697, Random vs Tactical 0.0068;  MC(256) vs MC(16) 0.9902
        3x3x3:  MC(64) vs Random 0.9526;  MC(64) vs Tactical 0.5688, Random vs Tactical 0.1147;  MC(256) vs MC(16) 0.6611
    The thresholds lie at least 5 standard errors below them: a score over 1024 games has a standard error of at most
    0.016 (5 SE: 0.08), a difference of two at most 0.022 (5 SE: 0.11)."""
    m, n, k = board
    pol = hip.policy
    mc64_random = _score(hip, pol.MonteCarloPolicy(k, 64, seed=1), pol.RandomPolicy(m * n, seed=2), board)
    mc64_tactical = _score(hip, pol.MonteCarloPolicy(k, 64, seed=3), pol.TacticalPolicy(k, seed=4), board)
    random_tactical = _score(hip, pol.RandomPolicy(m * n, seed=5), pol.TacticalPolicy(k, seed=6), board)
    mc256_mc16 = _score(hip, pol.MonteCarloPolicy(k, 256, seed=7), pol.MonteCarloPolicy(k, 16, seed=8), board)
    rates = (mc64_random, mc64_tactical, random_tactical, mc256_mc16)
    print(board, "MC64-Random %.4f MC64-Tactical %.4f Random-Tactical %.4f MC256-MC16 %.4f" % rates)
    vs_random, gap, mc256 = {(9, 9, 5): (0.9, 0.5, 0.9), (3, 3, 3): (0.85, 0.3, 0.5)}[board]
    assert mc64_random > vs_random, rates
    assert mc64_tactical > random_tactical + gap, rates  # MC(64) does better against Tactical than Random does
    assert mc256_mc16 > mc256, rates
