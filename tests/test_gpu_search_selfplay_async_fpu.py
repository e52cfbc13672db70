"""GPU: per-row search self-play with first-play urgency -- ``AsyncSearchSelfPlay(fpu=...)`` /
``mnk_search_selfplay_advance_opts_fpu`` and ``mnk_search_selfplay_advance_keep_fpu``.  With mixed budgets it is compared
launch for launch with the numpy rule (tests/puct_fpu_rule.py: ``AsyncKeepFpuRule``, which is ``AsyncOptsFpuRule`` without
``keep_tree``), with and without ``keep_tree``, the solver and root noise, on 3x3x3 from the empty board, on 9x9x5 from late
positions in the style of tests/golden/search_selfplay_async_starts.npz (a drawn board less a few stones: games end, fill
and are drawn inside the run) and on that fixture's own 7x9x5 rows, the sibling board of the 9x9x5 variant; and both
entry points on every other kind of board they are compiled for -- 12x13x5, 16x15x5 and 19x19x5 (the variants <6,13,5>,
<8,15,5> and <12,19,5>) and 12x12x5 (the generic form of five words) from the fixture's rows, 7x7x4 (the generic form of
two) from the empty board; the cases are tests/search_selfplay_async_fpu_cases.py's, where tests/test_puct_fpu_cpu.py shows
with the rule alone that each uses the options it turns on.  With every ply full it must leave, bit for bit, what the
lockstep ``SearchSelfPlay(fpu=..., same options)`` leaves (3x3x3, 9x9x5 and, for a few plies, 16x15x5 and 12x12x5) -- with
the solver the games are the lockstep solver's in no more launches, the exception the existing equalities state.

Everything is bit-exact except the noised priors of a root against numpy's, at the ``rtol=1e-6`` of
tests/test_gpu_puct_noise.py (``Beside`` of tests/test_gpu_search_selfplay_async_opts.py makes it); the rule then takes the
kernel's priors for those roots."""
import numpy as np
import pytest
import torch

from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from search_selfplay_async_fpu_cases import CASES, FPU, N, NOISE, new_rule
from test_gpu_search_selfplay_async import ENV_ID0, THRESHOLD, assert_same_state, exact_torch, new_async
from test_gpu_search_selfplay_async_keep import KeepBeside
from test_gpu_search_selfplay_async_opts import Beside, same_players

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("board,start,temp,rounds,seed,noise,solver,keep,tree_nodes", CASES)
def test_mixed_budgets_equal_the_rule_launch_for_launch(hip, board, start, temp, rounds, seed, noise, solver, keep,
                                                        tree_nodes):
    m, n, k = board
    rule, state = new_rule(board, start, temp, seed, noise, solver, keep, tree_nodes)
    assert rule.N % 4  # a partial workgroup
    sp = new_async(hip, board, rule.N, seed, temp_plies=temp, capacity=m * n, root_noise=noise, solver=solver,
                   keep_tree=keep, tree_nodes=tree_nodes, fpu=FPU)
    sp.sampler.env_id0 = ENV_ID0
    if state is not None:
        s = sp.state_dict()
        s["env"]["planes"] = torch.from_numpy(state[0].view(np.int64))
        s["env"]["meta"] = torch.from_numpy(state[1].astype(np.int64)).to(s["env"]["meta"].dtype)
        sp.load_state_dict(s)
    assert sp.fpu == FPU and sp.full_threshold == THRESHOLD
    (KeepBeside if keep else Beside)(sp, rule, rule.view()).advance(rounds)
    assert_same_state(sp, rule)
    assert sp.env._err.tolist() == [0, 0] and not rule.errors
    print(f"{board}: games {rule.stats[0]}, fast / full records {rule.fast_records} / {rule.full_records}, row plies "
          f"{rule.row_plies.tolist()}")
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0
    assert len(set(rule.row_plies.tolist())) > 1  # the rows are out of step


# ----------------------------------------------------------------------------- every ply full: the lockstep player
@pytest.mark.parametrize("noise", [None, NOISE])
@pytest.mark.parametrize("keep,tree_nodes", [(False, None), (True, 13), (True, 8)])
@pytest.mark.parametrize("board,plies,capacity", [((3, 3, 3), 2 * 9 + 5, None), ((9, 9, 5), 24, 81),
                                                  # a multi-word variant and the generic form of five words, a few plies
                                                  ((16, 15, 5), 6, None), ((12, 12, 5), 6, None),
                                                  ((17, 17, 5), 6, None)])  # (and the generic form of ten words)
def test_with_every_ply_full_it_is_the_lockstep_player(hip, board, plies, capacity, keep, tree_nodes, noise):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    I = 6
    lock = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(m * n), iterations=I, seed=13, temp_plies=3, capacity=capacity,
                          reuse=keep, tree_nodes=tree_nodes, root_noise=noise, fpu=FPU)
    lock.play(plies)
    kw = dict(full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity, root_noise=noise, keep_tree=keep,
              tree_nodes=tree_nodes)
    sp = new_async(hip, board, N, 13, fpu=FPU, **kw)
    sp.advance(plies * (I + 1))
    torch.cuda.synchronize()
    same_players(sp, lock)
    assert torch.equal(sp.leaf_obs, lock.obs) and torch.equal(sp.leaf_mask, lock.mask)  # the next roots
    assert sp.fresh.tolist() == [1] * N and sp.row_plies.tolist() == [plies] * N
    assert sp.buffer.plies.item() == plies and sp.env._err.tolist() == [0, 0]
    assert lock.buffer.visits.any()
    if board in ((16, 15, 5), (12, 12, 5), (17, 17, 5)):
        # (six plies of six iterations from the empty board: no game ends, and no unvisited cell's urgency decides a
        # selection -- the player without fpu records the same; the mixed cases above hold the urgency on these boards)
        assert lock.pop_game_stats() == sp.pop_game_stats()
    elif board == (9, 9, 5):
        assert lock.pop_game_stats() == sp.pop_game_stats()
        plain = new_async(hip, board, N, 13, **kw)
        plain.advance(plies * (I + 1))
        assert not torch.equal(sp.buffer.visits, plain.buffer.visits), "first-play urgency changed no search"
    else:
        assert lock.pop_game_stats() == sp.pop_game_stats() and lock.buffer.z.ne(hip.lib.Z_UNKNOWN).any()


def test_with_the_solver_the_games_are_the_lockstep_solvers_in_no_more_launches(hip):
    """(the exception the equalities above leave: a proven root plays at once, so the launches differ and the rows run out
    of step; the records of the first P plies of every row are the lockstep player's)"""
    from selfplay.search_selfplay import SearchSelfPlay

    board, seed, I, temp = (3, 3, 3), 13, 16, 3
    m, n, k = board
    C = m * n
    P, T = 2 * C, 8 * C
    lock = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=I, seed=seed, temp_plies=temp, capacity=T,
                          solver=True, fpu=FPU)
    lock.play(P)
    sp = new_async(hip, board, N, seed, full=I, fast=None, full_prob=1.0, temp_plies=temp, capacity=T, solver=True, fpu=FPU)
    rounds, block = 0, 8
    while sp.row_plies.min().item() < P:  # (the host looks between blocks)
        assert rounds <= P * (I + 1)
        sp.advance(block)
        rounds += block
    print(f"{board}: {rounds} launches for {P} plies of every row (lockstep: {P * (I + 1)}), row plies {sp.row_plies.tolist()}")
    assert sp.row_plies.max().item() <= T  # no slot below P was written twice
    a, b = sp.buffer, lock.buffer
    assert torch.equal(a.planes[:P], b.planes[:P]) and torch.equal(a.visits[:P], b.visits[:P])
    known = b.z[:P] != hip.lib.Z_UNKNOWN
    assert known.any() and torch.equal(a.z[:P][known], b.z[:P][known])
    assert b.visits[:P].any() and lock.pop_game_stats()["games"] > 0
    assert sp.env._err.tolist() == [0, 0]
