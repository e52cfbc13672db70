"""GPU: per-row search self-play with a Gumbel root -- ``AsyncSearchSelfPlay(gumbel=m)`` /
``mnk_search_selfplay_advance_gumbel``.  With every ply full it must leave, bit for bit, what the lockstep
``SearchSelfPlay(gumbel=m)`` of the same seed leaves; with mixed budgets it is compared round by round with the numpy rule
(tests/search_selfplay_async_gumbel_rule.py), which is handed the kernel's ``gscore`` of the rows that backed up a root so
that one ulp in a logarithm cannot send the two searches different ways -- and that ``gscore`` is compared with the rule's
own; the draw as a function of (seed, row id, ply); a captured round replayed; a ``state_dict`` round trip; the row without
a legal cell; the example's loop.

Ring visits on full plies are compared within ONE count: the policy is the f32 of f64 values that agree with numpy's to a
few ulps, rtol 1e-6 * 65 535 is 0.07 of a count, so a difference can arise only next to a rounding boundary of rint (the
bar of tests/test_gpu_puct_gumbel.py).  On fast plies they are exactly zero.  The seeds and shapes are those of
tests/test_search_selfplay_async_gumbel_cpu.py, which shows on the CPU that they reach every branch.

The boards: with mixed budgets 3x3x3, 4x6x3 and 9x9x5 from the empty board, 12x13x5, 16x15x5 and 19x19x5 (the variants
<6,13,5>, <8,15,5> and <12,19,5>) and 12x12x5 (the generic form of five words) from the stored late positions of
tests/golden/search_selfplay_async_starts.npz, and 7x7x4 (the generic form of two words) from the empty board for more
than a lap of its ring; uint8 and bfloat16 leaves, bfloat16 priors and values and the device key word are spread over
them.  With every ply full 3x3x3, 9x9x5, 7x9x5 and, for a few plies, the same four large boards."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from puct_gumbel_rule import gumbel_scores  # noqa: F401 (the reference of gscore, through the rule)
from search_selfplay_async_gumbel_rule import AsyncGumbelRule
from search_selfplay_async_rule import exact_np
from test_gpu_search_selfplay_async import exact_torch, load_start, new_async  # noqa: F401
from test_gpu_search_selfplay_async_opts import same_players
from test_search_selfplay_async_gumbel_cpu import (CONSIDERED, ENV_ID0, FAST, FULL, MIXED_HOW, MIXED_RUNS, THRESHOLD,
                                                   new_rule)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ring(sp):
    buf = sp.buffer
    return (buf.planes.cpu().numpy().view(np.uint64), buf.visits.cpu().numpy().view(np.uint16), buf.z.cpu().numpy())


# ----------------------------------------------------------------------------- 1. every ply full: the lockstep player
@pytest.mark.parametrize("board,N,I,cons,plies,capacity", [((3, 3, 3), 6, 8, 4, 2 * 9 + 5, None),
                                                           ((9, 9, 5), 5, 16, 8, 81 + 5, 81),
                                                           ((7, 9, 5), 5, 8, 8, 20, None),
                                                           # the multi-word variants and the generic form of five words,
                                                           # from the empty board: no game ends in so few plies (the
                                                           # mixed cases below carry the game ends)
                                                           ((12, 13, 5), 5, 4, 4, 6, None),
                                                           ((16, 15, 5), 5, 4, 4, 6, None),
                                                           ((19, 19, 5), 3, 4, 4, 6, None),
                                                           ((12, 12, 5), 3, 4, 4, 6, None),
                                                           # and those of ten and of 21 words
                                                           ((25, 25, 5), 3, 4, 4, 6, None),
                                                           ((17, 17, 5), 5, 4, 4, 6, None)])
def test_with_every_ply_full_it_is_the_lockstep_gumbel_player(hip, board, N, I, cons, plies, capacity):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    lock = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(m * n), iterations=I, seed=13, capacity=capacity, gumbel=cons)
    lock.play(plies)
    sp = new_async(hip, board, N, 13, full=I, fast=None, full_prob=1.0, capacity=capacity, gumbel=cons)
    sp.advance(plies * (I + 1))
    torch.cuda.synchronize()
    same_players(sp, lock)
    assert torch.equal(sp.leaf_obs, lock.obs) and torch.equal(sp.leaf_mask, lock.mask)  # the next roots
    assert sp.fresh.tolist() == [1] * N and sp.row_plies.tolist() == [plies] * N
    assert sp.buffer.plies.item() == plies == lock.buffer.plies.item()
    assert sp.env._err.tolist() == [0, 0] and lock.env._err.tolist() == [0, 0]
    assert lock.buffer.visits.any()
    # and the option did something: the PUCT player of the same seed records other targets
    puct = new_async(hip, board, N, 13, full=I, fast=None, full_prob=1.0, capacity=capacity)
    puct.advance(plies * (I + 1))
    assert not torch.equal(puct.buffer.visits, sp.buffer.visits)
    assert lock.pop_game_stats() == sp.pop_game_stats()


# ----------------------------------------------------------------------------- 2 / 3. mixed budgets against the rule
def follow(sp, rule, rounds, obs, mask, what=""):
    """``rounds`` launches of the player beside the rule, which searches with the kernel's gscore: leaves, masks and
    fresh are compared exactly in every round, gscore of the rows that backed a root up with the rule's own (rtol 1e-6 on
    free cells, -inf elsewhere; every other row's is untouched, bit for bit), every ply's ring record as it is written
    (visits: zero on a fast ply, within one count and summing to 65 535 within half the free cells on a full one).
    Returns the counts of (full, fast) records compared and the largest difference of a count."""
    ev = exact_np(rule.C)
    N, C = rule.N, rule.C
    full_seen = fast_seen = worst = 0
    for r in range(rounds):
        roots = sp.fresh.cpu().numpy().astype(bool)  # the rows whose pending leaf is the root of a fresh tree
        before = sp.gscore.cpu().numpy().view(np.uint32).copy()
        logged = len(rule.log)
        sp.advance(1)
        got = sp.gscore.cpu().numpy()
        out = rule.advance(*ev(obs, mask), gscore=got)
        obs, mask, fresh = out
        assert np.array_equal(sp.leaf_obs.float().cpu().numpy(), obs), f"{what}leaves, round {r}"
        assert np.array_equal(sp.leaf_mask.cpu().numpy(), mask), f"{what}masks, round {r}"
        assert sp.fresh.tolist() == fresh.tolist(), f"{what}fresh, round {r}"
        assert sorted(rule.gscore_wanted) == np.flatnonzero(roots).tolist(), f"{what}rows that backed up a root, round {r}"
        for i in range(N):
            if roots[i]:
                want = rule.gscore_wanted[i]
                free = np.isfinite(want)
                assert np.array_equal(np.isneginf(got[i]), ~free), f"{what}-inf cells, round {r}, row {i}"
                assert np.allclose(got[i][free], want[free], rtol=1e-6, atol=0), f"{what}gscore, round {r}, row {i}"
            else:
                assert np.array_equal(got[i].view(np.uint32), before[i]), f"{what}gscore touched, round {r}, row {i}"
        if len(rule.log) > logged:
            visits = sp.buffer.visits.cpu().numpy().view(np.uint16)
            for e in rule.log[logged:]:
                mine = visits[e["slot"], e["row"]].astype(np.int64)
                want = rule.ring_visits[e["slot"], e["row"]].astype(np.int64)
                if e["full"]:
                    full_seen += 1
                    worst = max(worst, int(np.abs(mine - want).max()))
                    assert np.abs(mine - want).max() <= 1, f"{what}visits, round {r}, row {e['row']}"
                    assert abs(int(mine.sum()) - 65535) <= e["free"] / 2, f"{what}sum, round {r}, row {e['row']}"
                else:
                    fast_seen += 1
                    assert not mine.any() and not want.any(), f"{what}a fast ply's visits, round {r}, row {e['row']}"
    return full_seen, fast_seen, worst, obs, mask


def assert_same_state(sp, rule, what=""):
    """ring planes and z, env, ply counts, statistics and the device's count of written plies against the rule; the ring's
    visits within one count, zero where the rule's are"""
    planes, visits, z = ring(sp)
    assert np.array_equal(planes, rule.ring_planes), what + " ring planes"
    assert np.array_equal(z, rule.ring_z), what + " ring z"
    diff = np.abs(visits.astype(np.int64) - rule.ring_visits.astype(np.int64))
    assert diff.max() <= 1, what + " ring visits"
    zero = ~rule.ring_visits.any(axis=2)
    assert not visits[zero].any(), what + " records without a policy target"
    assert np.array_equal(sp.env._planes.cpu().numpy().view(np.uint64), rule.planes()), what + " env planes"
    assert np.array_equal(sp.env._meta.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, rule.meta()), what + " env meta"
    assert sp.row_plies.tolist() == rule.row_plies.tolist(), what + " row_plies"
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist(), what + " stats"
    assert sp.buffer.plies.item() == rule.plies_max, what + " plies_max"


@pytest.mark.parametrize("board,N,rounds,seed", MIXED_RUNS)
def test_mixed_budgets_equal_the_rule_round_by_round(hip, board, N, rounds, seed):
    m, n, k = board
    assert N % 4  # a partial workgroup
    start, leaf_dtype, out_dtype, key_word = MIXED_HOW[board, N, rounds, seed]
    leaf_dtype, out_dtype = getattr(torch, leaf_dtype), getattr(torch, out_dtype)
    rule = new_rule(board, N, seed, start)
    sp = new_async(hip, board, N, seed + 100 if key_word else seed, full=FULL, fast=FAST, full_prob=0.5,
                   leaf_dtype=leaf_dtype, out_dtype=out_dtype, capacity=m * n, gumbel=CONSIDERED)
    sp.sampler.env_id0 = ENV_ID0
    if key_word:  # the device word replaces the host's key
        sp.sampler.seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    load_start(sp, board, start)
    assert sp.full_threshold == THRESHOLD and sp.gscore.shape == (N, m * n) and sp.vroot.shape == (N,)
    assert sp.leaf_obs.dtype == leaf_dtype
    obs, mask = rule.view()
    full_seen, fast_seen, worst, _, _ = follow(sp, rule, rounds, obs, mask)
    print(f"{board}: {full_seen} full and {fast_seen} fast records, largest difference of a count {worst}")
    assert_same_state(sp, rule)
    assert sp.env._err.tolist() == [0, 0] and not rule.errors
    assert full_seen == rule.full_records > 0 and fast_seen == rule.fast_records > 0
    assert len(set(rule.row_plies.tolist())) > 1  # the rows are out of step
    assert sp.buffer.plies_host == rounds >= sp.buffer.plies.item()


# ----------------------------------------------------------------------------- 4. the draw: (seed, row id, ply)
def test_two_halves_with_their_row_ids_play_the_games_of_the_whole(hip):
    board, seed, rounds = (3, 3, 3), 6, 130
    kw = dict(full=FULL, fast=FAST, full_prob=0.5, capacity=9, gumbel=CONSIDERED)
    whole = new_async(hip, board, 6, seed, **kw)
    whole.advance(rounds)
    halves = []
    for id0 in (0, 3):
        sp = new_async(hip, board, 3, seed, **kw)
        sp.sampler.env_id0 = id0
        sp.advance(rounds)
        halves.append(sp)
    torch.cuda.synchronize()
    for id0, sp in zip((0, 3), halves):
        rows = slice(id0, id0 + 3)
        assert torch.equal(sp.buffer.planes, whole.buffer.planes[..., rows]), f"ring planes of rows {id0}.."
        assert torch.equal(sp.buffer.visits, whole.buffer.visits[:, rows]), f"ring visits of rows {id0}.."
        assert torch.equal(sp.buffer.z, whole.buffer.z[:, rows]), f"ring z of rows {id0}.."
        assert torch.equal(sp.row_plies, whole.row_plies[rows]) and torch.equal(sp.env._meta, whole.env._meta[rows])
        assert torch.equal(sp.env._planes, whole.env._planes[..., rows])
        assert torch.equal(sp.gscore, whole.gscore[rows]) and torch.equal(sp.vroot, whole.vroot[rows])
    assert len(set(whole.row_plies.tolist())) > 1 and whole.buffer.visits.any()
    assert not torch.equal(halves[0].buffer.visits, halves[1].buffer.visits)  # (the row id matters)


# ----------------------------------------------------------------------------- 5. a captured round; a restored state
def test_a_captured_round_replayed_equals_eager_rounds(hip):
    R, board, N, seed = 90, (3, 3, 3), 6, 21

    def new():
        # (the workspace is compared whole below, and it is allocated uninitialised: both start from zeros and set
        # their roots up again)
        sp = new_async(hip, board, N, seed, full=FULL, fast=FAST, full_prob=0.5, capacity=9, gumbel=CONSIDERED)
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
    assert torch.equal(sp.gscore, eager.gscore) and torch.equal(sp.vroot, eager.vroot)
    assert sp.buffer.plies_host == eager.buffer.plies_host == 1 + R
    assert len(set(eager.row_plies.tolist())) > 1 and eager.pop_game_stats()["games"] > 0
    assert eager.buffer.visits.any()


def test_a_restored_state_continues_as_the_rule_does(hip):
    board, N, seed, before, after = (3, 3, 3), 6, 9, 47, 60
    kw = dict(full=FULL, fast=FAST, full_prob=0.5, capacity=9, gumbel=CONSIDERED)
    a = new_async(hip, board, N, seed, **kw)
    a.advance(before)
    state = a.state_dict()
    b = new_async(hip, board, N, seed + 1, **kw)
    b.load_state_dict(state)
    assert b.fresh.tolist() == [1] * N and b.sampler.seed == seed
    # the rule, loaded from the same state: SelfPlayRule.load, the ring, the ply counts, then fresh trees
    rule = AsyncGumbelRule(3, 3, 3, N, 9, FULL, FAST, THRESHOLD, 1.25, seed, CONSIDERED)
    rule.load(state["env"]["planes"].numpy().view(np.uint64), state["env"]["meta"].numpy())
    rule.ring_planes[:] = state["buffer"]["planes"].numpy().view(np.uint64)
    rule.ring_visits[:] = state["buffer"]["visits"].numpy().view(np.uint16)
    rule.ring_z[:] = state["buffer"]["z"].numpy()
    rule.row_plies[:] = state["row_plies"].numpy()
    rule.plies_max = int(state["buffer"]["plies"].item())
    rule.stats[:] = state["stats"].sum(dim=0)[:5].numpy()
    assert len(set(rule.row_plies.tolist())) > 1  # saved in the middle of searches that were out of step
    obs, mask = rule.begin()
    full_seen, fast_seen, _, _, _ = follow(b, rule, after, obs, mask)
    assert_same_state(b, rule)
    assert full_seen > 0 and fast_seen > 0 and b.pop_game_stats()["games"] > 0


# ----------------------------------------------------------------------------- 6. a row without a legal cell
def test_a_root_without_a_legal_cell_is_reported_and_left_alone(hip):
    lib = hip.lib
    N = 5
    sp = new_async(hip, (3, 3, 3), N, 4, full=FULL, fast=FAST, full_prob=0.5, capacity=9, gumbel=CONSIDERED)
    s = sp.state_dict()
    # row 2 holds a full board without a run (x o x / x o o / o x x), handed in by state
    black, white = [0, 2, 3, 7, 8], [1, 4, 5, 6]
    bits = lambda cells: sum(1 << (a + a // 3) for a in cells)  # noqa: E731
    s["env"]["planes"][0, 0, 2], s["env"]["planes"][1, 0, 2] = bits(black), bits(white)
    s["env"]["meta"][2] = (9 << 1) | 1
    sp.load_state_dict(s)
    sp.gscore[2] = 123.0  # a sentinel: the row's scores and value are never written
    sp.vroot[2] = -7.0
    sp.advance(40)
    torch.cuda.synchronize()
    assert sp.env._err.tolist() == [lib.ERR_VISITS, 2]
    assert sp.row_plies[2].item() == 0 and sp.fresh[2].item() == 0 and (sp.row_plies > 0).sum().item() == N - 1
    assert sp.env._meta[2].item() == (9 << 1) | 1
    assert sp.env._planes[:, 0, 2].tolist() == [bits(black), bits(white)]
    assert (sp.buffer.z[:, 2] == lib.Z_UNKNOWN).all() and not sp.buffer.visits[:, 2].any()
    assert sp.leaf_mask[2].sum().item() == 0 and sp.leaf_obs[2].sum().item() == 9  # its root, shown again
    assert (sp.gscore[2] == 123.0).all() and sp.vroot[2].item() == -7.0
    assert sp.buffer.visits.any() and (sp.gscore[[0, 1, 3, 4]] != 123.0).all()  # the other rows play on
    sp.env._err.zero_()


# ----------------------------------------------------------------------------- 7. the example
def test_the_examples_loop_runs_with_a_gumbel_root_and_per_ply_budgets(hip):
    path = os.path.join(ROOT, "examples", "alphazero_selfplay.py")
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    lines = []
    net = ex.train(3, 3, 3, envs=64, iterations=16, rounds=2, updates=10, seed=0, search="gumbel", fast_iterations=4,
                   full_prob=0.5, log=lines.append)
    assert net is not None and len(lines) == 2
    loss = float(lines[-1].rsplit("loss", 1)[1])
    assert math.isfinite(loss)
