"""GPU: per-row search self-play with forced playouts and policy target pruning -- ``AsyncSearchSelfPlay(forced=k)`` /
``mnk_search_selfplay_advance_opts_forced``.  With mixed budgets it is compared launch for launch with the numpy rule
(tests/puct_forced_rule.py: ``AsyncOptsForcedRule``) on the cases of tests/puct_forced_cases.py -- five rows, or the three of
a stored start; the FULL / FAST budgets and round counts of the cases with first-play urgency; with and without root noise,
``noise_on_fast``, the solver and first-play urgency -- where tests/test_puct_forced_cpu.py shows with the rule alone that
each forces, prunes a full ply's record and leaves a ply that does not force as it was.  With every ply full it must leave,
bit for bit, what the lockstep ``SearchSelfPlay(forced=k)`` of the same seed leaves (3x3x3 and 9x9x5; six plies on 16x15x5,
12x12x5 and 17x17x5).

Everything is bit-exact except the noised priors of a root against numpy's, at the ``rtol=1e-6`` of
tests/test_gpu_puct_noise.py (``Beside`` of tests/test_gpu_search_selfplay_async_opts.py makes it); the rule then takes the
kernel's priors for those roots."""
import numpy as np
import pytest
import torch

import puct_forced_cases as cases
from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from puct_forced_cases import ASYNC_CASES, C_PUCT, ENV_ID0, FAST, FPU, FULL, K_FORCED, N, NOISE, THRESHOLD
from test_gpu_puct_forced import spike_torch
from test_gpu_search_selfplay_async import assert_same_state
from test_gpu_search_selfplay_async_opts import Beside, same_players

pytestmark = pytest.mark.gpu


def new_async(board, rows, seed, evaluator, full=FULL, fast=FAST, full_prob=0.75, **kw):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    m, n, k = board
    return AsyncSearchSelfPlay(m, n, k, rows, evaluator=evaluator, iterations=full, fast_iterations=fast,
                               full_prob=full_prob, c=C_PUCT, seed=seed, **kw)


class SpikeBeside(Beside):
    """``Beside`` with the case's own evaluator in the place of the dyadic one"""

    def __init__(self, sp, rule, view, evaluator):
        super().__init__(sp, rule, view)
        self.ev = evaluator


@pytest.mark.parametrize("case", range(len(ASYNC_CASES)))
def test_mixed_budgets_equal_the_rule_launch_for_launch(hip, case):
    board, start, temp, rounds, seed, noise, on_fast, solver, fpu = ASYNC_CASES[case]
    m, n, k = board
    rule, state, ev = cases.new_async_rule(case)
    assert rule.N % 4  # a partial workgroup
    sp = new_async(board, rule.N, seed, spike_torch(m * n, cases.free_spikes(board, state)), temp_plies=temp,
                   capacity=m * n, root_noise=noise, noise_on_fast=on_fast, solver=solver, fpu=fpu, forced=K_FORCED)
    sp.sampler.env_id0 = ENV_ID0
    if state is not None:
        s = sp.state_dict()
        s["env"]["planes"] = torch.from_numpy(state[0].view(np.int64))
        s["env"]["meta"] = torch.from_numpy(state[1].astype(np.int64)).to(s["env"]["meta"].dtype)
        sp.load_state_dict(s)
    assert sp.forced == K_FORCED and sp.fpu == fpu and sp.full_threshold == THRESHOLD
    SpikeBeside(sp, rule, rule.view(), ev).advance(rounds)
    assert_same_state(sp, rule)
    assert sp.env._err.tolist() == [0, 0] and not rule.errors
    pruned = sum(1 for _, _, full, forces, _, raw, counts, _ in rule.plies if full and forces and (raw != counts).any())
    print(f"{board}: games {rule.stats[0]}, fast / full records {rule.fast_records} / {rule.full_records}, row plies "
          f"{rule.row_plies.tolist()}, full plies with pruned counts {pruned}")
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0 and pruned > 0
    assert len(set(rule.row_plies.tolist())) > 1  # the rows are out of step


# ----------------------------------------------------------------------------- every ply full: the lockstep player
@pytest.mark.parametrize("noise,fpu", [(None, None), (NOISE, FPU)])
@pytest.mark.parametrize("board,plies,capacity", [((3, 3, 3), 2 * 9 + 5, None), ((9, 9, 5), 24, 81),
                                                  # a multi-word variant and the generic forms of five and of ten
                                                  # words, a few plies
                                                  ((16, 15, 5), 6, None), ((12, 12, 5), 6, None), ((17, 17, 5), 6, None)])
def test_with_every_ply_full_it_is_the_lockstep_player(hip, board, plies, capacity, noise, fpu):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    I, spikes = 6, cases.spikes_of(m, n, k)
    lock = SearchSelfPlay(m, n, k, N, evaluator=spike_torch(m * n, spikes), iterations=I, c=C_PUCT, seed=13, temp_plies=3,
                          capacity=capacity, root_noise=noise, fpu=fpu, forced=K_FORCED)
    lock.play(plies)
    kw = dict(full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity, root_noise=noise, fpu=fpu)
    sp = new_async(board, N, 13, spike_torch(m * n, spikes), forced=K_FORCED, **kw)
    sp.advance(plies * (I + 1))
    torch.cuda.synchronize()
    same_players(sp, lock)
    assert torch.equal(sp.leaf_obs, lock.obs) and torch.equal(sp.leaf_mask, lock.mask)  # the next roots
    assert sp.fresh.tolist() == [1] * N and sp.row_plies.tolist() == [plies] * N
    assert sp.buffer.plies.item() == plies and sp.env._err.tolist() == [0, 0]
    assert lock.buffer.visits.any() and lock.pop_game_stats() == sp.pop_game_stats()
    plain = new_async(board, N, 13, spike_torch(m * n, spikes), **kw)
    plain.advance(plies * (I + 1))
    assert not torch.equal(sp.buffer.visits, plain.buffer.visits), "forced playouts changed no record"
