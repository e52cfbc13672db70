"""GPU: the tree-search player -- ``mnk_sample_search`` / ``SearchPolicy.act`` bit for bit against the numpy rule
(tests/search_rule.py) on the five built-in boards and two generic ones, finished games included, for every observation
dtype, with and without ``deterministic``, and with the largest budget; ``tournament.play_match`` and the strength
ladder.  What it shares with the Monte Carlo player: test_gpu_players.py."""
import numpy as np
import pytest
import torch

from player_cases import SEARCH, _score, hip, positions  # noqa: F401 (hip: the fixture)
from search_rule import search
from tactical_rule import completions

pytestmark = pytest.mark.gpu
OBS_DTYPES = (torch.float32, torch.bfloat16, torch.uint8)


def first_most_visited(stats):
    """the deterministic move from the stats: the first cell of maximal n, 0 when nothing was expanded"""
    v = stats[:, 0]
    return np.where(v.max(axis=1) > 0, v.argmax(axis=1), 0)


# ----------------------------------------------------------------------------- 1. bit for bit against the rule
@pytest.mark.parametrize("board,rows,runs", [
    ((3, 3, 3), 24, ((40, 8, 1.0), (128, 3, 0.5))),
    ((9, 9, 5), 8, ((96, 16, 1.0), (24, 64, 1.4))),
    ((13, 13, 5), 4, ((48, 8, 1.0),)),
    ((15, 15, 5), 4, ((40, 8, 1.0),)),
    ((19, 19, 5), 4, ((64, 8, 1.0),)),       # I < |L|: the root is never fully expanded
    ((7, 7, 4), 8, ((80, 16, 1.0),)),        # generic NW forms
    ((12, 12, 5), 4, ((48, 8, 0.7),)),
    ((17, 17, 5), 5, ((8, 4, 1.0),)),        # the forms of sixteen and of thirty-two words: ten and 21 words a plane
    ((25, 25, 5), 5, ((8, 4, 1.0),)),
])
def test_actions_and_stats_equal_the_rule(hip, board, rows, runs):
    """(3x3x3, 9x9x5, 13x13x5, 15x15x5, 19x19x5: built-in variants; 7x7x4, 12x12x5, 17x17x5, 25x25x5: the generic NW
    forms)"""
    m, n, k = board
    obs = positions(m, n, k, rows, m * 100 + n * 10 + k, max_fill=0.6 if m > 9 else 1.0)
    finished = [i for i in range(rows) if completions(obs[i:i + 1, 1], np.ones((1, m, n), bool), k).any()
                or completions(obs[i:i + 1, 0], np.ones((1, m, n), bool), k).any()]
    assert finished  # boards that already hold a run are in the comparison
    for I, B, c in runs:
        step, env_id0, seed = 3, 17, 1000 + I
        want_r, want_stats = search(obs, k, I, B, c, seed, step, env_id0)
        want_d = first_most_visited(want_stats)
        for dtype in OBS_DTYPES:
            for det, want in ((False, want_r), (True, want_d)):
                got, stats = SEARCH.act(hip, obs, k, (I, B, c), seed, step, env_id0, dtype, det)
                assert np.array_equal(stats, want_stats), (I, B, dtype, det)
                assert np.array_equal(got, want), (I, B, dtype, det)
        if board == (19, 19, 5):
            legal = ((obs[:, 0] == 0) & (obs[:, 1] == 0)).reshape(rows, -1)
            assert ((want_stats[:, 0] > 0).sum(1) < legal.sum(1))[2:].all()


def test_largest_budget_matches_the_rule_on_one_row(hip):
    """I = 2048, B = 4 on one 3x3x3 row (the tree fills its whole LDS budget of I + 1 nodes or runs into terminals)"""
    obs = np.zeros((1, 2, 3, 3), np.float32)
    obs[0, 1, 1, 1] = 1
    want_a, want_s = search(obs, 3, 2048, 4, 1.0, seed=5)
    got, stats = SEARCH.act(hip, obs, 3, (2048, 4, 1.0), seed=5)
    assert np.array_equal(stats, want_s) and np.array_equal(got, want_a)
    assert stats[0, 0].sum() == 2048 * 4


# ----------------------------------------------------------------------------- 2. the strength ladder
@pytest.mark.parametrize("board", [(9, 9, 5), (3, 3, 3)])
def test_strength_ordering(hip, board):
    """play_match scores of player 1 over 1024 games (half as black) with these seeds and the default c, as measured on
    the MI355X (tools/exp_search.py):
        9x9x5:  Search(256) vs Random 1.0000;  vs Tactical 0.9990 (Random vs Tactical 0.0068);  Search(256) vs Search(16)
                0.9990
        3x3x3:  Search(128) vs Random 0.9785;  vs Tactical 0.6416 (Random vs Tactical 0.1147);  Search(128) vs Search(4)
                0.9565
    A score over 1024 games has a standard error of at most 0.016 (5 SE: 0.08), a difference of two at most 0.022 (5 SE:
    0.11); every threshold in LADDER lies at least 5 SE below the measured rate."""
    m, n, k = board
    pol = hip.policy
    small, large = {(9, 9, 5): (16, 256), (3, 3, 3): (4, 128)}[board]
    s_random = _score(hip, pol.SearchPolicy(k, large, 32, seed=1), pol.RandomPolicy(m * n, seed=2), board)
    s_tactical = _score(hip, pol.SearchPolicy(k, large, 32, seed=3), pol.TacticalPolicy(k, seed=4), board)
    random_tactical = _score(hip, pol.RandomPolicy(m * n, seed=5), pol.TacticalPolicy(k, seed=6), board)
    large_small = _score(hip, pol.SearchPolicy(k, large, 32, seed=7), pol.SearchPolicy(k, small, 32, seed=8), board)
    rates = (s_random, s_tactical, random_tactical, large_small)
    print(board, "Search-Random %.4f Search-Tactical %.4f Random-Tactical %.4f Large-Small %.4f" % rates)
    vs_random, vs_tactical, gap = LADDER[board]
    assert s_random > vs_random, rates
    assert s_tactical > vs_tactical, rates
    assert s_tactical > random_tactical + 0.4, rates  # the search does far better against Tactical than Random does
    assert large_small > gap, rates


# thresholds per board: Search vs Random, Search vs Tactical, Search(large I) vs Search(small I)
LADDER = {(9, 9, 5): (0.9, 0.9, 0.9), (3, 3, 3): (0.88, 0.55, 0.85)}
