"""GPU: per-row search self-play with root noise and the solver -- ``AsyncSearchSelfPlay(root_noise=..., solver=...)`` /
``mnk_search_selfplay_advance_opts``.  With every ply full and noise on it must leave, bit for bit, what the lockstep
``SearchSelfPlay(root_noise=...)`` leaves; with the solver its games are the lockstep solver's, in fewer launches; with mixed
budgets it is compared round by round with the numpy rule (tests/search_selfplay_async_opts_rule.py); a captured round
replayed; a ``state_dict`` round trip; the noise as a function of (seed, row id, ply); the options off against the old entry
point.

Everything is bit-exact except one comparison: the noised priors of a root against numpy's, which are equal to
``rtol=1e-6`` on free cells -- the bar of tests/test_gpu_puct_noise.py for the same arithmetic (the reasoning is in that
file's header: the device's f64 logarithms and numpy's may differ in the last place, which the f32 mix almost always rounds
away).  The rule then takes the kernel's priors for those roots, so that one ulp cannot send the two searches apart."""
import functools

import numpy as np
import pytest
import torch

from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_async_rule import exact_np
from test_gpu_search_selfplay_async import (ENV_ID0, FAST, FULL, THRESHOLD, assert_same_state, exact_torch, load_start,
                                            new_async, start_state)

pytestmark = pytest.mark.gpu
NOISE = (0.3, 0.25)


def same_players(a, b):
    for t in ("planes", "visits", "z", "plies"):
        assert torch.equal(getattr(a.buffer, t), getattr(b.buffer, t)), t
    assert torch.equal(a.env._planes, b.env._planes) and torch.equal(a.env._meta, b.env._meta)
    assert torch.equal(a.stats.sum(dim=0), b.stats.sum(dim=0))


# ----------------------------------------------------------------------------- 1. every ply full, noise: the lockstep player
@pytest.mark.parametrize("board,N,plies,capacity", [((3, 3, 3), 6, 2 * 9 + 5, None), ((9, 9, 5), 5, 81 + 5, 81),
                                                    ((25, 25, 5), 5, 6, None)])  # (21 words, a few plies)
def test_with_every_ply_full_and_noise_it_is_the_lockstep_player(hip, board, N, plies, capacity):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    I = 6
    lock = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(m * n), iterations=I, seed=13, temp_plies=3, capacity=capacity,
                          root_noise=NOISE)
    lock.play(plies)
    sp = new_async(hip, board, N, 13, full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity, root_noise=NOISE)
    sp.advance(plies * (I + 1))
    torch.cuda.synchronize()
    same_players(sp, lock)
    assert torch.equal(sp.leaf_obs, lock.obs) and torch.equal(sp.leaf_mask, lock.mask)  # the next roots
    assert sp.fresh.tolist() == [1] * N and sp.row_plies.tolist() == [plies] * N
    assert sp.buffer.plies.item() == plies
    plain = new_async(hip, board, N, 13, full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity)
    plain.advance(plies * (I + 1))
    assert not torch.equal(sp.buffer.visits, plain.buffer.visits), "the noise changed no search"
    assert lock.pop_game_stats() == sp.pop_game_stats() and lock.buffer.visits.any()


# ----------------------------------------------------------------------------- 2. the solver: proven roots play at once
# board, rows, seed.  The seeds were chosen on the CPU with the rule (tests/test_search_selfplay_async_opts_cpu.py,
# solver_runs) so that the three conditions below hold: on 3x3x3 the rule needs 288 launches for P = 18 plies of every
# row (the lockstep player 306) and its most advanced row has then played 20; on 4x6x3 779 (816) and 50.
SOLVER_I, SOLVER_TEMP = 16, 3


@pytest.mark.parametrize("board,N,seed", [((3, 3, 3), 6, 13), ((4, 6, 3), 5, 13)])
def test_with_the_solver_proven_roots_play_at_once_and_the_games_are_the_lockstep_players(hip, board, N, seed):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    C, I = m * n, SOLVER_I
    P, T = 2 * C, 8 * C
    lock = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=I, seed=seed, temp_plies=SOLVER_TEMP, capacity=T,
                          solver=True)
    lock.play(P)
    sp = new_async(hip, board, N, seed, full=I, fast=None, full_prob=1.0, temp_plies=SOLVER_TEMP, capacity=T, solver=True)
    rounds, block = 0, 8
    while sp.row_plies.min().item() < P:  # (the host looks between blocks)
        assert rounds < 3 * P * (I + 1)
        sp.advance(block)
        rounds += block
    print(f"{board}: {rounds} launches for {P} plies of every row (lockstep: {P * (I + 1)}), row plies {sp.row_plies.tolist()}")
    assert rounds < P * (I + 1)
    assert P < sp.row_plies.max().item() <= T  # a row ran ahead, and no slot below P was written twice
    a, b = sp.buffer, lock.buffer
    assert torch.equal(a.planes[:P], b.planes[:P]) and torch.equal(a.visits[:P], b.visits[:P])
    known = b.z[:P] != hip.lib.Z_UNKNOWN
    assert known.any() and torch.equal(a.z[:P][known], b.z[:P][known])
    assert b.visits[:P].any() and lock.pop_game_stats()["games"] > 0
    assert sp.env._err.tolist() == [0, 0]


# ----------------------------------------------------------------------------- 3. mixed budgets against the rule
# board, rows, leaf dtype, dtype of priors and values, device key word, temp_plies, rounds, start ("golden": a stored env
# state near the end of games), seed, root_noise, noise_on_fast, solver.  The seeds were chosen on the CPU with the rule so
# that the conditions at the end of the test hold in every case.
CASES = [
    ((3, 3, 3), 7, torch.float32, torch.float32, False, 2, 130, None, 6, NOISE, False, True),
    ((9, 9, 5), 5, torch.bfloat16, torch.float32, False, 6, 1150, None, 6, NOISE, True, False),
    ((7, 7, 4), 5, torch.uint8, torch.float32, True, 4, 700, None, 6, NOISE, False, True),
    ((8, 3, 3), 7, torch.uint8, torch.bfloat16, False, 2, 400, None, 6, None, False, True),
    ((19, 19, 5), 3, torch.float32, torch.float32, False, 4, 150, "golden", 6, (0.03, 0.25), False, True),
    ((16, 15, 5), 5, torch.float32, torch.bfloat16, False, 4, 150, "golden", 6, None, False, True),
    # the generic forms of sixteen and of thirty-two words, from a computed start ("late": no root has a single free cell)
    ((17, 17, 5), 5, torch.float32, torch.bfloat16, False, 4, 150, "late", 6, NOISE, False, True),
    ((25, 25, 5), 5, torch.uint8, torch.float32, False, 4, 150, "late", 6, (0.03, 0.25), False, True),
]
LARGE_CASES = CASES[-2:]


def new_rule(board, N, temp, seed, start, noise, on_fast, solver):
    m, n, k = board
    rule = AsyncOptsRule(m, n, k, N, m * n, FULL, FAST, THRESHOLD, 1.25, temp, seed, ENV_ID0, root_noise=noise,
                         noise_on_fast=on_fast, solver=solver)
    state = start_state(board, start)
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule


class Beside:
    """a player and the rule beside it: ``advance(rounds)`` launches both and compares them after every launch.  With
    noise, the rows of ``sp.root_priors`` that a launch wrote -- those whose pending leaf was their root -- are held
    against what the rule computes for them, every other row must be as it was, and the rule goes on with the kernel's."""

    def __init__(self, sp, rule, view):
        self.sp, self.rule, (self.obs, self.mask) = sp, rule, view
        self.ev = exact_np(rule.C)
        self.held = sp.root_priors.cpu().numpy() if sp.root_noise is not None else None

    def check_root_priors(self, roots, plain, what):
        rule, was, got = self.rule, self.held, self.sp.root_priors.cpu().numpy()
        assert sorted(rule.root_wanted) == np.flatnonzero(roots).tolist(), what
        assert np.array_equal(got[~roots], was[~roots]), what + ": a row that backed up no root was written"
        for i, (noised, want) in rule.root_wanted.items():
            free = plain[i] != 0  # (the evaluator's priors are positive on the free cells and zero on the others)
            assert np.array_equal(got[i][~free], want[~free]), f"{what}: row {i}, occupied cells"
            if noised:
                np.testing.assert_allclose(got[i][free], want[free], rtol=1e-6, atol=0, err_msg=f"{what}: row {i}")
                assert not np.array_equal(got[i][free], plain[i][free]), f"{what}: row {i} took no noise"
            else:
                assert np.array_equal(got[i], want), f"{what}: row {i}, a root without noise"
        self.held = got

    def advance(self, rounds, what=""):
        sp, rule = self.sp, self.rule
        for r in range(rounds):
            roots = sp.fresh.cpu().numpy().astype(bool)  # the rows whose pending leaf is their root
            priors, values = self.ev(self.obs, self.mask)
            sp.advance(1)
            given = sp.root_priors.cpu().numpy() if self.held is not None else None
            self.obs, self.mask, fresh = rule.advance(priors, values, root_priors=given)
            if given is not None:
                self.check_root_priors(roots, priors, f"{what}round {r}")
            assert np.array_equal(sp.leaf_obs.float().cpu().numpy(), self.obs), f"{what}leaves, round {r}"
            assert np.array_equal(sp.leaf_mask.cpu().numpy(), self.mask), f"{what}masks, round {r}"
            assert sp.fresh.tolist() == fresh.tolist(), f"{what}fresh, round {r}"


@pytest.mark.parametrize("board,N,leaf_dtype,out_dtype,key_word,temp,rounds,start,seed,noise,on_fast,solver", CASES)
def test_mixed_budgets_equal_the_rule_round_by_round_with_the_options_on(hip, board, N, leaf_dtype, out_dtype, key_word,
                                                                          temp, rounds, start, seed, noise, on_fast, solver):
    m, n, k = board
    assert N % 4  # a partial workgroup
    rule = new_rule(board, N, temp, seed, start, noise, on_fast, solver)
    sp = new_async(hip, board, N, seed + 100 if key_word else seed, leaf_dtype=leaf_dtype, out_dtype=out_dtype,
                   temp_plies=temp, capacity=m * n, root_noise=noise, noise_on_fast=on_fast, solver=solver)
    sp.sampler.env_id0 = ENV_ID0
    if key_word:  # the device word replaces the host's key
        sp.sampler.seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    load_start(sp, board, start)
    assert sp.full_threshold == THRESHOLD and sp.leaf_obs.dtype == leaf_dtype
    Beside(sp, rule, rule.view()).advance(rounds)  # (right after begin(): the roots)
    assert_same_state(sp, rule)
    assert sp.env._err.tolist() == [0, 0] and not rule.errors
    by_proof = sum(1 for rec in rule.proven_plies if rec[4])
    print(f"{board}: games {rule.stats[0]}, fast / full records {rule.fast_records} / {rule.full_records}, row plies "
          f"{rule.row_plies.tolist()}, plies ended by proof {by_proof}, noised / plain roots {rule.noised_roots} / "
          f"{rule.plain_roots}")
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0
    assert len(set(rule.row_plies.tolist())) > 1  # the rows are out of step
    if start is None and board == (3, 3, 3):
        assert rule.row_plies.min() > 2 * m * n  # more than two laps of the ring
    if solver:
        assert by_proof > 0
    if noise and not on_fast:
        assert rule.noised_roots > 0 and rule.plain_roots > 0
    if noise and on_fast:
        assert rule.noised_roots > 0 and rule.plain_roots == 0


# ----------------------------------------------------------------------------- 4. a captured round
def test_a_captured_round_replayed_equals_eager_rounds(hip):
    R, board, N, seed = 90, (3, 3, 3), 6, 21

    def new():
        # (the workspace is compared whole below, and it is allocated uninitialised: both start from zeros and set their
        # roots up again)
        sp = new_async(hip, board, N, seed, temp_plies=2, capacity=9, root_noise=NOISE, solver=True)
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
    assert torch.equal(sp.root_priors, eager.root_priors) and sp.root_priors.any()
    assert sp.buffer.plies_host == eager.buffer.plies_host == 1 + R
    assert len(set(eager.row_plies.tolist())) > 1 and eager.pop_game_stats()["games"] > 0


# ----------------------------------------------------------------------------- 5. state_dict
def test_a_restored_state_continues_as_the_rule_does_with_the_noise_it_had(hip):
    board, N, seed, temp, before, after = (3, 3, 3), 6, 9, 2, 47, 60
    a = new_async(hip, board, N, seed, temp_plies=temp, capacity=9, root_noise=NOISE)
    a.advance(before)
    state = a.state_dict()
    searching = a.fresh.cpu().numpy() == 0  # rows in the middle of a search: root_priors holds their current root's
    assert searching.any() and len(set(a.row_plies.tolist())) > 1
    b = new_async(hip, board, N, seed + 1, temp_plies=0, capacity=9, root_noise=NOISE)
    b.load_state_dict(state)
    assert b.fresh.tolist() == [1] * N and b.temp_plies == temp and b.sampler.seed == seed
    rule = AsyncOptsRule(3, 3, 3, N, 9, FULL, FAST, THRESHOLD, 1.25, temp, seed, root_noise=NOISE)
    rule.load(state["env"]["planes"].numpy().view(np.uint64), state["env"]["meta"].numpy())
    rule.ring_planes[:] = state["buffer"]["planes"].numpy().view(np.uint64)
    rule.ring_visits[:] = state["buffer"]["visits"].numpy().view(np.uint16)
    rule.ring_z[:] = state["buffer"]["z"].numpy()
    rule.row_plies[:] = state["row_plies"].numpy()
    rule.plies_max = int(state["buffer"]["plies"].item())
    rule.stats[:] = state["stats"].sum(dim=0)[:5].numpy()
    both = Beside(b, rule, rule.begin())
    both.advance(1)
    # the searches that were interrupted restart with the noise they had: bit for bit what the first player's roots held
    assert torch.equal(b.root_priors[searching], a.root_priors[searching])
    assert rule.noised_roots > 0 and rule.plain_roots > 0
    both.advance(after - 1, "after the first, ")
    assert_same_state(b, rule)
    assert b.pop_game_stats()["games"] > 0


# ----------------------------------------------------------------------------- 6. what the noise is a function of
def test_the_noise_is_a_function_of_seed_row_id_and_ply_alone(hip):
    board, rounds = (3, 3, 3), 40

    def play(N, id0, seed):
        sp = new_async(hip, board, N, seed, temp_plies=2, capacity=9, root_noise=NOISE, noise_on_fast=True)
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
    plain = exact_torch(9)(torch.zeros(1, 2, 3, 3, device=DEV), torch.ones(1, 9, device=DEV))[0]  # the empty board's
    for i in range(4):  # every row its own draw, none the plain priors, and another seed gives others
        assert not torch.equal(small0[i], plain[0]) and not torch.equal(small0[i], other0[i])
        assert all(not torch.equal(large0[i], large0[j]) for j in range(8) if j != i)
    # the mix keeps the priors' sum (eta sums to 1 and the empty board's priors are mixed on every cell) up to rounding
    assert torch.allclose(small0.sum(dim=1), plain.sum() * 0.75 + 0.25, rtol=1e-5)


# ----------------------------------------------------------------------------- 7. the options off
def test_with_the_options_off_the_new_entry_point_is_the_old_one(hip):
    lib = hip.lib
    board, N, rounds = (9, 9, 5), 5, 40

    def new():
        sp = new_async(hip, board, N, 6, leaf_dtype=torch.uint8, temp_plies=6, capacity=81)
        sp.workspace.zero_()
        sp._begin()
        return sp

    old, sp = new(), new()
    old.advance(rounds)
    buf, env = sp.buffer, sp.env
    for _ in range(rounds):
        priors, pcode, values, vcode = sp.policy._evaluate(sp.leaf_obs, sp.leaf_mask, N, 81)
        seed, seed_dev, _, _, env_id0, _ = sp.sampler.block()
        lib.call("mnk_search_selfplay_advance_opts", lib.ptr(sp.workspace), lib.ptr(env._planes), lib.ptr(env._meta), N, 9,
                 9, 5, sp.iterations, sp.fast_iterations, sp.full_threshold, lib.ptr(priors), pcode, lib.ptr(values), vcode,
                 sp.policy.c, sp.temp_plies, seed, seed_dev, env_id0, lib.ptr(sp.row_plies), buf.capacity,
                 lib.ptr(buf.planes), lib.ptr(buf.visits), lib.ptr(buf.z), lib.ptr(sp.leaf_obs), sp.policy._leaf_code,
                 lib.ptr(sp.leaf_mask), lib.ptr(sp.fresh), lib.ptr(buf.plies), lib.ptr(sp.stats), lib.ptr(env._err), 0, 0.0,
                 0.0, 0, None, lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    same_players(sp, old)
    assert torch.equal(sp.workspace, old.workspace) and torch.equal(sp.row_plies, old.row_plies)
    assert torch.equal(sp.leaf_obs, old.leaf_obs) and torch.equal(sp.leaf_mask, old.leaf_mask)
    assert torch.equal(sp.fresh, old.fresh) and len(set(old.row_plies.tolist())) > 1 and old.row_plies.min().item() > 0
