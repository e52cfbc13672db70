"""GPU: per-row search self-play with several leaves per evaluator call -- ``AsyncSearchSelfPlay(leaves=L)`` /
``mnk_search_selfplay_advance_leaves``.  At one leaf the new entry point is ``mnk_search_selfplay_advance_opts`` launch for
launch; with every ply full it leaves, bit for bit, what the lockstep ``SearchSelfPlay(leaves=L, root_noise=...)`` leaves;
with the solver its games are the lockstep solver's, in fewer launches; with mixed budgets it is compared round by round
with the numpy rule (tests/search_selfplay_async_leaves_rule.py); a captured round replayed; a ``state_dict`` round trip;
the noise as a function of (seed, row id, ply).

Everything is bit-exact except one comparison: the noised priors of a root against numpy's, equal to ``rtol=1e-6`` on free
cells -- the bar and the reasoning of tests/test_gpu_puct_noise.py, taken over with ``Beside`` from
tests/test_gpu_search_selfplay_async_opts.py.  The rule then takes the kernel's priors for those roots."""
import numpy as np
import pytest
import torch

from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from search_selfplay_async_leaves_rule import AsyncLeavesRule
from test_gpu_search_selfplay_async import assert_same_state, exact_torch, load_start, new_async, start_state
from test_gpu_search_selfplay_async_keep import peaked_torch
from test_gpu_search_selfplay_async_opts import NOISE, Beside, same_players
from test_search_selfplay_async_leaves_cpu import (ENV_ID0, GPU_CASES, GPU_FAST, GPU_FULL, THRESHOLD,
                                                   assert_every_branch_was_reached, gpu_rule)

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}


def root_visits(sp):
    """n of node 0 of every row, read from the workspace (the layout: csrc/mnk_puct_tree.h, leaves = 1)"""
    al = lambda x, a: (x + a - 1) // a * a  # noqa: E731
    nwg = (sp.m * (sp.n + 1) + 31) // 32
    node = al(al(16 + 16 * nwg, 16) + 2 * (sp.iterations + 2), 16)
    rows = sp.workspace.reshape(sp.num_envs, -1)
    return rows[:, node:node + 4].contiguous().view(torch.int32)[:, 0]


# ----------------------------------------------------------------------------- 1. one leaf: the launch before
@pytest.mark.parametrize("board,N,rounds", [((3, 3, 3), 7, 130), ((9, 9, 5), 5, 600)])
def test_with_one_leaf_the_new_entry_point_is_the_old_launch(hip, board, N, rounds):
    lib = hip.lib
    m, n, k = board
    C = m * n

    def new():
        sp = new_async(hip, board, N, 6, full=GPU_FULL, fast=GPU_FAST, temp_plies=2, capacity=C, root_noise=NOISE,
                       solver=True)
        sp.workspace.zero_()
        sp._begin()
        return sp

    old, sp = new(), new()
    sims = torch.zeros(N, dtype=torch.int32, device=DEV)
    buf, env = sp.buffer, sp.env
    for r in range(rounds):
        old.advance(1)
        before = sims.clone()
        priors, pcode, values, vcode = sp.policy._evaluate(sp.leaf_obs, sp.leaf_mask, N, C)
        seed, seed_dev, _, _, env_id0, _ = sp.sampler.block()
        lib.call("mnk_search_selfplay_advance_leaves", lib.ptr(sp.workspace), lib.ptr(env._planes), lib.ptr(env._meta), N,
                 m, n, k, sp.iterations, sp.fast_iterations, 1, sp.full_threshold, lib.ptr(priors), pcode, lib.ptr(values),
                 vcode, sp.policy.c, sp.temp_plies, seed, seed_dev, env_id0, lib.ptr(sp.row_plies), buf.capacity,
                 lib.ptr(buf.planes), lib.ptr(buf.visits), lib.ptr(buf.z), lib.ptr(sp.leaf_obs), sp.policy._leaf_code,
                 lib.ptr(sp.leaf_mask), lib.ptr(sp.fresh), lib.ptr(buf.plies), lib.ptr(sp.stats), lib.ptr(env._err), 1,
                 NOISE[0], NOISE[1], 0, lib.ptr(sp.root_priors), lib.ptr(sims), lib.stream_ptr(DEV))
        what = f"round {r}"
        same_players(sp, old)
        assert torch.equal(sp.workspace, old.workspace), what
        assert torch.equal(sp.leaf_obs, old.leaf_obs) and torch.equal(sp.leaf_mask, old.leaf_mask), what
        assert torch.equal(sp.fresh, old.fresh) and torch.equal(sp.row_plies, old.row_plies), what
        assert torch.equal(sp.root_priors, old.root_priors), what
        # the counter the launch read is n_root - 1 of the tree it then backed up: on a row that searches on the tree still
        # stands so, and the counter is one more; a row that played starts at 0
        on = sp.fresh == 0
        assert torch.equal(before[on], root_visits(sp)[on] - 1) and torch.equal(sims[on], before[on] + 1), what
        assert not sims[~on].any(), what
    assert sp.env._err.tolist() == [0, 0] and len(set(old.row_plies.tolist())) > 1
    assert old.row_plies.min().item() > (C if C == 9 else 0) and old.pop_game_stats()["games"] > 0


# ----------------------------------------------------------------------------- 2. every ply full: the lockstep player
@pytest.mark.parametrize("board,N,plies,capacity,I,L", [((3, 3, 3), 6, 2 * 9 + 5, None, 8, 2), ((3, 3, 3), 6, 2 * 9 + 5, None, 8, 4),
                                                       ((9, 9, 5), 5, 81 + 5, 81, 8, 4), ((9, 9, 5), 5, 81 + 5, 81, 16, 16),
                                                       ((17, 17, 5), 5, 6, None, 8, 4)])  # (ten words, a few plies)
def test_with_every_ply_full_it_is_the_lockstep_player_with_leaves(hip, board, N, plies, capacity, I, L):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    # (on 289 cells eight iterations under the dyadic evaluator go to eight unvisited cells, one leaf at a time or four,
    # and the records would be those of one leaf: that board searches under the peaked evaluator)
    ev = peaked_torch if board == (17, 17, 5) else exact_torch
    lock = SearchSelfPlay(m, n, k, N, evaluator=ev(m * n), iterations=I, seed=13, temp_plies=3, capacity=capacity,
                          root_noise=NOISE, leaves=L)
    lock.play(plies)
    sp = new_async(hip, board, N, 13, full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity, root_noise=NOISE,
                   leaves=L, evaluator=ev(m * n))
    sp.advance(plies * (I // L + 1))
    torch.cuda.synchronize()
    same_players(sp, lock)
    assert sp.leaf_obs.shape[0] == N * L
    for j in range(L):  # the next roots: slot 0 pending, the others void and showing it
        assert torch.equal(sp.leaf_obs[j::L], lock.obs) and torch.equal(sp.leaf_mask[j::L], lock.mask), j
    assert sp.fresh.tolist() == [1] * N and sp.row_plies.tolist() == [plies] * N and sp.row_sims.tolist() == [0] * N
    assert sp.buffer.plies.item() == plies and sp.env._err.tolist() == [0, 0]
    one = new_async(hip, board, N, 13, full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity, root_noise=NOISE,
                    evaluator=ev(m * n))
    one.advance(plies * (I + 1))
    assert not torch.equal(sp.buffer.visits, one.buffer.visits), "the leaves changed no search"
    assert lock.pop_game_stats() == sp.pop_game_stats() and lock.buffer.visits.any()


# ----------------------------------------------------------------------------- 3. the solver with leaves
# The seeds are those of tests/test_search_selfplay_async_leaves_cpu.py (lockstep_runs), where the rule shows the
# conditions below.
SOLVER_I, SOLVER_L, SOLVER_TEMP = 16, 4, 3


@pytest.mark.parametrize("board,N,seed", [((3, 3, 3), 6, 13), ((4, 6, 3), 5, 13)])
def test_with_the_solver_and_leaves_the_games_are_the_lockstep_solvers_in_fewer_launches(hip, board, N, seed):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    C, I, L = m * n, SOLVER_I, SOLVER_L
    P, T = 2 * C, 8 * C
    lock = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=I, seed=seed, temp_plies=SOLVER_TEMP, capacity=T,
                          solver=True, leaves=L)
    lock.play(P)
    sp = new_async(hip, board, N, seed, full=I, fast=None, full_prob=1.0, temp_plies=SOLVER_TEMP, capacity=T, solver=True,
                   leaves=L)
    rounds = 0
    while sp.row_plies.min().item() < P:  # (the host looks after every launch: the count is exact)
        assert rounds < 3 * P * (I // L + 1)
        sp.advance(1)
        rounds += 1
    print(f"{board}: {rounds} launches for {P} plies of every row (lockstep: {P * (I // L + 1)}), row plies {sp.row_plies.tolist()}")
    assert rounds < P * (I // L + 1)
    assert sp.row_plies.max().item() <= T  # no slot below P was written twice
    a, b = sp.buffer, lock.buffer
    assert torch.equal(a.planes[:P], b.planes[:P]) and torch.equal(a.visits[:P], b.visits[:P])
    known = b.z[:P] != hip.lib.Z_UNKNOWN
    assert known.any() and torch.equal(a.z[:P][known], b.z[:P][known])
    assert b.visits[:P].any() and lock.pop_game_stats()["games"] > 0
    assert sp.env._err.tolist() == [0, 0]


# ----------------------------------------------------------------------------- 4. mixed budgets against the rule
class BesideLeaves(Beside):
    """``Beside`` for a player with L slots per row: the evaluator's batch has N * L rows, a row's root is its slot 0, and
    after every launch the counters, the ring and the error words are held against the rule's as well"""

    def advance(self, rounds, what=""):
        sp, rule, L = self.sp, self.rule, self.sp.leaves
        buf = sp.buffer
        for r in range(rounds):
            roots = sp.fresh.cpu().numpy().astype(bool)  # the rows whose slot 0 is their root, pending
            priors, values = self.ev(self.obs, self.mask)
            sp.advance(1)
            given = sp.root_priors.cpu().numpy() if self.held is not None else None
            self.obs, self.mask, fresh = rule.advance(priors, values, root_priors=given)
            if given is not None:
                self.check_root_priors(roots, priors[::L], f"{what}round {r}")
            assert np.array_equal(sp.leaf_obs.float().cpu().numpy(), self.obs), f"{what}leaves, round {r}"
            assert np.array_equal(sp.leaf_mask.cpu().numpy(), self.mask), f"{what}masks, round {r}"
            assert sp.fresh.tolist() == fresh.tolist(), f"{what}fresh, round {r}"
            assert sp.row_plies.tolist() == rule.row_plies.tolist(), f"{what}row_plies, round {r}"
            assert sp.row_sims.tolist() == rule.row_sims.tolist(), f"{what}row_sims, round {r}"
            assert np.array_equal(buf.planes.cpu().numpy().view(np.uint64), rule.ring_planes), f"{what}ring planes, round {r}"
            assert np.array_equal(buf.visits.cpu().numpy().view(np.uint16), rule.ring_visits), f"{what}ring visits, round {r}"
            assert np.array_equal(buf.z.cpu().numpy(), rule.ring_z), f"{what}ring z, round {r}"
            assert sp.env._err.tolist() == [0, 0] and not rule.errors, f"{what}err, round {r}"


def new_player(hip, case, seed=None, **kw):
    board, N, leaf, out, key_word, temp, _, _, case_seed, noise, on_fast, solver, L, c = GPU_CASES[case]
    seed = case_seed if seed is None else seed
    return new_async(hip, board, N, seed, full=GPU_FULL, fast=GPU_FAST, leaf_dtype=DTYPES[leaf], out_dtype=DTYPES[out],
                     temp_plies=temp, capacity=board[0] * board[1], root_noise=noise, noise_on_fast=on_fast, solver=solver,
                     leaves=L, c=c, **kw)


@pytest.mark.parametrize("case", list(GPU_CASES))
def test_mixed_budgets_equal_the_rule_round_by_round_with_leaves(hip, case):
    board, N, leaf, _, key_word, _, rounds, start, seed, _, _, _, L, _ = GPU_CASES[case]
    assert N % 4  # a partial workgroup
    rule = gpu_rule(case, start_state(board, start))
    sp = new_player(hip, case, seed + 100 if key_word else seed)
    sp.sampler.env_id0 = ENV_ID0
    if key_word:  # the device word replaces the host's key
        sp.sampler.seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    load_start(sp, board, start)
    assert sp.full_threshold == THRESHOLD and sp.leaf_obs.dtype == DTYPES[leaf] and sp.leaf_obs.shape[0] == N * L
    BesideLeaves(sp, rule, rule.view()).advance(rounds)  # (right after begin(): the roots)
    assert_same_state(sp, rule)
    assert_every_branch_was_reached(case, rule)
    assert len(set(rule.row_plies.tolist())) > 1  # the rows are out of step


# ----------------------------------------------------------------------------- 5. a captured round, and a state_dict
def test_a_captured_round_replayed_equals_eager_rounds_with_leaves(hip):
    R, board, N, seed = 60, (3, 3, 3), 6, 21

    def new():
        # (the workspace is compared whole below, and it is allocated uninitialised: both start from zeros and set their
        # roots up again)
        sp = new_async(hip, board, N, seed, full=GPU_FULL, fast=GPU_FAST, temp_plies=2, capacity=9, root_noise=NOISE,
                       solver=True, leaves=4)
        sp.workspace.zero_()
        sp._begin()
        return sp

    eager = new()
    eager.advance(1 + R)
    sp = new()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp.advance(1)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sp.advance(1)
    sp.buffer.plies_host -= 1  # (the capture itself ran nothing)
    for _ in range(R):
        graph.replay()
    sp.note_replayed(R)
    torch.cuda.synchronize()
    same_players(sp, eager)
    assert torch.equal(sp.row_plies, eager.row_plies) and torch.equal(sp.stats, eager.stats)
    assert torch.equal(sp.leaf_obs, eager.leaf_obs) and torch.equal(sp.leaf_mask, eager.leaf_mask)
    assert torch.equal(sp.fresh, eager.fresh) and torch.equal(sp.workspace, eager.workspace)
    assert torch.equal(sp.row_sims, eager.row_sims) and eager.row_sims.any()
    assert torch.equal(sp.root_priors, eager.root_priors) and sp.root_priors.any()
    assert sp.buffer.plies_host == eager.buffer.plies_host == 1 + R
    assert len(set(eager.row_plies.tolist())) > 1 and eager.pop_game_stats()["games"] > 0


def test_a_restored_state_continues_as_the_rule_does_with_leaves(hip):
    board, N, seed, temp, before, after = (3, 3, 3), 6, 9, 2, 31, 40
    kw = dict(full=GPU_FULL, fast=GPU_FAST, capacity=9, root_noise=NOISE, leaves=4)
    a = new_async(hip, board, N, seed, temp_plies=temp, **kw)
    a.advance(before)
    state = a.state_dict()
    searching = a.fresh.cpu().numpy() == 0  # rows in the middle of a search: root_priors holds their current root's
    assert searching.any() and len(set(a.row_plies.tolist())) > 1 and a.row_sims.any()
    b = new_async(hip, board, N, seed + 1, temp_plies=0, **kw)
    b.load_state_dict(state)
    assert b.fresh.tolist() == [1] * N and b.temp_plies == temp and b.sampler.seed == seed and not b.row_sims.any()
    rule = AsyncLeavesRule(3, 3, 3, N, 9, GPU_FULL, GPU_FAST, THRESHOLD, 1.25, temp, seed, root_noise=NOISE, leaves=4)
    rule.load(state["env"]["planes"].numpy().view(np.uint64), state["env"]["meta"].numpy())
    rule.ring_planes[:] = state["buffer"]["planes"].numpy().view(np.uint64)
    rule.ring_visits[:] = state["buffer"]["visits"].numpy().view(np.uint16)
    rule.ring_z[:] = state["buffer"]["z"].numpy()
    rule.row_plies[:] = state["row_plies"].numpy()
    rule.plies_max = int(state["buffer"]["plies"].item())
    rule.stats[:] = state["stats"].sum(dim=0)[:5].numpy()
    both = BesideLeaves(b, rule, rule.begin())
    both.advance(1)
    # the searches that were interrupted restart with the noise they had: bit for bit what the first player's roots held
    assert torch.equal(b.root_priors[searching], a.root_priors[searching])
    both.advance(after - 1, "after the first, ")
    assert_same_state(b, rule)
    assert b.pop_game_stats()["games"] > 0


# ----------------------------------------------------------------------------- 6. what the noise is a function of
def test_the_noise_is_a_function_of_seed_row_id_and_ply_alone_with_leaves(hip):
    board, rounds = (3, 3, 3), 30

    def play(N, id0, seed):
        sp = new_async(hip, board, N, seed, full=GPU_FULL, fast=GPU_FAST, temp_plies=2, capacity=9, root_noise=NOISE,
                       noise_on_fast=True, leaves=4)
        sp.sampler.env_id0 = id0
        first = None
        for r in range(rounds):
            sp.advance(1)
            if r == 0:
                first = sp.root_priors.clone()  # the roots of ply 0: the empty board's
        return sp, first

    small, small0 = play(4, 4, 5)  # rows of the global ids 4 .. 7
    large, large0 = play(8, 0, 5)  # ids 0 .. 7
    other, other0 = play(4, 4, 6)
    assert torch.equal(small0, large0[4:]) and torch.equal(small.root_priors, large.root_priors[4:])
    assert torch.equal(small.row_plies, large.row_plies[4:]) and small.row_plies.min().item() > 0
    assert torch.equal(small.buffer.visits, large.buffer.visits[:, 4:])
    assert torch.equal(small.leaf_obs, large.leaf_obs[16:]) and torch.equal(small.row_sims, large.row_sims[4:])
    plain = exact_torch(9)(torch.zeros(1, 2, 3, 3, device=DEV), torch.ones(1, 9, device=DEV))[0]  # the empty board's
    for i in range(4):  # every row its own draw, none the plain priors, and another seed gives others
        assert not torch.equal(small0[i], plain[0]) and not torch.equal(small0[i], other0[i])
        assert all(not torch.equal(large0[i], large0[j]) for j in range(8) if j != i)
    # the mix keeps the priors' sum (eta sums to 1 and the empty board's priors are mixed on every cell) up to rounding
    assert torch.allclose(small0.sum(dim=1), plain.sum() * 0.75 + 0.25, rtol=1e-5)
