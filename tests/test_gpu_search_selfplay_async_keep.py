"""GPU: per-row search self-play that keeps the played move's subtree -- ``AsyncSearchSelfPlay(keep_tree=True)`` /
``mnk_search_selfplay_advance_keep``.  With every ply full it must leave, bit for bit, what the lockstep
``SearchSelfPlay(reuse=True, tree_nodes=K)`` leaves, ``carried`` included; with mixed budgets it is compared round by round
with the numpy rule (tests/search_selfplay_async_keep_rule.py), ``carried`` included; a row that keeps more than a chunk of
64 nodes; a captured round replayed; a ``state_dict`` round trip; ``reset_trees()``; and ``keep_tree=False`` against the
player without the keyword.  The cases and their seeds: tests/search_selfplay_async_keep_cases.py, chosen and checked on
the CPU (tests/test_search_selfplay_async_keep_cpu.py).

Everything is bit-exact except one comparison: the noised priors of a root against numpy's, at the ``rtol=1e-6`` of
tests/test_gpu_puct_noise.py (``Beside`` of tests/test_gpu_search_selfplay_async_opts.py makes it); the rule then takes the
kernel's priors for those roots."""
import numpy as np
import pytest
import torch

import search_selfplay_async_keep_cases as cases
from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from search_selfplay_async_keep_rule import AsyncKeepRule
from test_gpu_search_selfplay_async import assert_same_state, exact_torch, load_start, new_async
from test_gpu_search_selfplay_async_opts import Beside, same_players

pytestmark = pytest.mark.gpu
NOISE, ENV_ID0 = cases.NOISE, cases.ENV_ID0
FULL, FAST, THRESHOLD = cases.FULL, cases.FAST, cases.THRESHOLD


def peaked_torch(C, out_dtype=torch.float32):
    """``cases.peaked_np`` in plain torch ops"""
    table = torch.from_numpy(cases.peaked_table(C)).to(DEV)

    def evaluate(leaf_obs, leaf_mask):
        cnt = leaf_obs.float().reshape(len(leaf_obs), 2, -1).sum(dim=2)
        priors, values = leaf_mask.float() * table, (torch.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5) - 2) / 4
        return priors.to(out_dtype), values.to(out_dtype)

    return evaluate


class KeepBeside(Beside):
    """``Beside`` with ``carried`` compared after every launch as well"""

    def advance(self, rounds, what=""):
        for r in range(rounds):
            super().advance(1, f"{what}launch {r}: ")
            assert np.array_equal(self.sp.carried.cpu().numpy(), self.rule.carried), f"{what}carried, launch {r}"


# ----------------------------------------------------------------------------- 1. every ply full: the lockstep player
@pytest.mark.parametrize("noise", [None, NOISE])
@pytest.mark.parametrize("tree_nodes", [13, 8])  # (8: keep_nodes = 2, children are dropped on every carried ply)
@pytest.mark.parametrize("board,N,plies,capacity", [((3, 3, 3), 6, 2 * 9 + 5, None), ((9, 9, 5), 5, 81 + 5, 81),
                                                    ((25, 25, 5), 5, 6, None)])  # (21 words, a few plies)
def test_with_every_ply_full_it_is_the_lockstep_player_that_keeps_its_trees(hip, board, N, plies, capacity, tree_nodes,
                                                                            noise):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    I = 6
    # (on 625 cells six iterations under the dyadic evaluator never visit a child twice, every ply would carry the child
    # alone and the records would be those of the player that keeps nothing: that board searches under the peaked one)
    ev = peaked_torch if board == (25, 25, 5) else exact_torch
    lock = SearchSelfPlay(m, n, k, N, evaluator=ev(m * n), iterations=I, seed=13, temp_plies=3, capacity=capacity,
                          reuse=True, tree_nodes=tree_nodes, root_noise=noise)
    lock.play(plies)
    kw = dict(full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity, root_noise=noise, evaluator=ev(m * n))
    sp = new_async(hip, board, N, 13, keep_tree=True, tree_nodes=tree_nodes, **kw)
    sp.advance(plies * (I + 1))
    torch.cuda.synchronize()
    same_players(sp, lock)
    assert torch.equal(sp.leaf_obs, lock.obs) and torch.equal(sp.leaf_mask, lock.mask)  # the next roots
    assert sp.fresh.tolist() == [1] * N and sp.row_plies.tolist() == [plies] * N
    assert sp.buffer.plies.item() == plies
    plain = new_async(hip, board, N, 13, **kw)
    plain.advance(plies * (I + 1))
    assert not torch.equal(sp.buffer.visits, plain.buffer.visits), "the carried trees changed no search"
    assert lock.pop_game_stats() == sp.pop_game_stats() and lock.buffer.visits.any()
    # what the player carried at the end of its last ply is what the lockstep search finds at the start of its next
    lock.play(1)
    assert torch.equal(sp.carried, lock.carried)
    kept = sp.carried[:, 0]
    assert kept.max().item() <= tree_nodes - I and sp.carried.any()
    assert sp.env._err.tolist() == [0, 0]


# ----------------------------------------------------------------------------- 2. mixed budgets against the rule
@pytest.mark.parametrize("case", range(len(cases.MIXED)))
def test_mixed_budgets_equal_the_rule_round_by_round(hip, case):
    board, N, leaf, out, key_word, temp, rounds, start, seed, noise, on_fast, solver, tree_nodes, evaluator = cases.MIXED[case]
    m, n, k = board
    leaf_dtype, out_dtype = getattr(torch, leaf), getattr(torch, out)
    assert N % 4  # a partial workgroup
    rule = cases.new_rule(board, N, temp, seed, start, noise, on_fast, solver, tree_nodes)
    ev = {"exact": exact_torch, "peaked": peaked_torch}[evaluator](m * n, out_dtype)
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    sp = AsyncSearchSelfPlay(m, n, k, N, evaluator=ev, iterations=FULL, fast_iterations=FAST, full_prob=0.75,
                             seed=seed + 100 if key_word else seed, leaf_dtype=leaf_dtype, temp_plies=temp, capacity=m * n,
                             root_noise=noise, noise_on_fast=on_fast, solver=solver, keep_tree=True, tree_nodes=tree_nodes)
    sp.sampler.env_id0 = ENV_ID0
    if key_word:  # the device word replaces the host's key
        sp.sampler.seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    load_start(sp, board, start)
    assert sp.full_threshold == THRESHOLD and sp.leaf_obs.dtype == leaf_dtype and not sp.carried.any()
    both = KeepBeside(sp, rule, rule.view())  # (right after begin(): the roots)
    both.ev = cases.EVALUATORS[evaluator](rule.C)
    both.advance(rounds)
    assert_same_state(sp, rule)
    assert sp.env._err.tolist() == [0, 0] and not rule.errors
    many, fresh_after_end, truncated, proven = cases.conditions(rule)
    print(f"{board}: games {rule.stats[0]}, fast / full records {rule.fast_records} / {rule.full_records}, row plies "
          f"{rule.row_plies.tolist()}, kept counts {sorted({t[3] for t in rule.trace})}, truncated {truncated}, proven when "
          f"carried {proven}")
    assert many, "no carried ply kept more than one node"
    assert fresh_after_end, "no ply started fresh after a game ended"
    assert rule.fast_records > 0 and rule.full_records > 0 and len(set(rule.row_plies.tolist())) > 1
    if tree_nodes == 8:
        assert truncated, "no ply kept keep_nodes nodes"
    if solver and board in ((3, 3, 3), (16, 15, 5)):
        assert proven, "no carried root kept the proof it had when carried"
    if solver and tree_nodes == 8:
        assert cases.dropped_proofs(rule) > 0, "no proof was dropped with the child that justified it"
    if noise:
        assert rule.noised_roots > 0


# ----------------------------------------------------------------------------- 3. the marking's chunk boundary
def test_a_row_that_keeps_more_than_a_chunk_of_nodes(hip):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    (m, n, k), N, I = cases.CHUNK_BOARD, cases.CHUNK_N, cases.CHUNK_I
    rule, trace = cases.chunk_run()
    kept = [t[3] for t in rule.trace]
    assert any(x > 64 and x % 8 for x in kept), kept
    sp = AsyncSearchSelfPlay(m, n, k, N, evaluator=peaked_torch(m * n), iterations=I, seed=cases.CHUNK_SEED,
                             temp_plies=cases.CHUNK_TEMP, capacity=m * n, keep_tree=True, tree_nodes=cases.CHUNK_NODES)
    sp.sampler.env_id0 = ENV_ID0
    for r, (obs, mask, fresh, carried) in enumerate(trace):
        sp.advance(1)
        assert np.array_equal(sp.leaf_obs.cpu().numpy(), obs), f"leaves, launch {r}"
        assert np.array_equal(sp.leaf_mask.cpu().numpy(), mask), f"masks, launch {r}"
        assert sp.fresh.tolist() == fresh.tolist(), f"fresh, launch {r}"
        assert np.array_equal(sp.carried.cpu().numpy(), carried), f"carried, launch {r}"
    assert_same_state(sp, rule)
    assert sp.row_plies.tolist() == [cases.CHUNK_PLIES] * N and sp.env._err.tolist() == [0, 0]
    print("kept", kept)


# ----------------------------------------------------------------------------- 4. a captured round
def test_a_captured_round_replayed_equals_eager_rounds(hip):
    R, board, N, seed = 90, (3, 3, 3), 6, 21

    def new():
        # (the workspace is compared whole below, and it is allocated uninitialised: both start from zeros and set their
        # roots up again)
        sp = new_async(hip, board, N, seed, temp_plies=2, capacity=9, root_noise=NOISE, solver=True, keep_tree=True)
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
    assert torch.equal(sp.carried, eager.carried) and eager.carried.any()
    assert torch.equal(sp.root_priors, eager.root_priors) and sp.root_priors.any()
    assert sp.buffer.plies_host == eager.buffer.plies_host == 1 + R
    assert len(set(eager.row_plies.tolist())) > 1 and eager.pop_game_stats()["games"] > 0
    assert sp.env._err.tolist() == [0, 0]


# ----------------------------------------------------------------------------- 5. state_dict
def rule_from_state(state, N, temp, seed, **kw):
    rule = AsyncKeepRule(3, 3, 3, N, 9, FULL, FAST, THRESHOLD, 1.25, temp, seed, keep_tree=True, **kw)
    rule.load(state["env"]["planes"].numpy().view(np.uint64), state["env"]["meta"].numpy())
    rule.ring_planes[:] = state["buffer"]["planes"].numpy().view(np.uint64)
    rule.ring_visits[:] = state["buffer"]["visits"].numpy().view(np.uint16)
    rule.ring_z[:] = state["buffer"]["z"].numpy()
    rule.row_plies[:] = state["row_plies"].numpy()
    rule.plies_max = int(state["buffer"]["plies"].item())
    rule.stats[:] = state["stats"].sum(dim=0)[:5].numpy()
    return rule


def test_a_restored_state_starts_every_row_fresh_and_continues_as_the_rule_does(hip):
    board, N, seed, temp, before, after = (3, 3, 3), 6, 9, 2, 47, 60
    a = new_async(hip, board, N, seed, temp_plies=temp, capacity=9, keep_tree=True)
    a.advance(before)
    state = a.state_dict()
    assert "carried" not in state and a.carried.any() and len(set(a.row_plies.tolist())) > 1
    b = new_async(hip, board, N, seed + 1, temp_plies=0, capacity=9, keep_tree=True)
    b.advance(5)
    b.load_state_dict(state)
    assert b.fresh.tolist() == [1] * N and not b.carried.any() and b.temp_plies == temp and b.sampler.seed == seed
    rule = rule_from_state(state, N, temp, seed)
    both = KeepBeside(b, rule, rule.begin())
    both.advance(after)
    assert_same_state(b, rule)
    assert b.pop_game_stats()["games"] > 0 and b.carried.any() and b.env._err.tolist() == [0, 0]


# ----------------------------------------------------------------------------- 6. reset_trees
def test_reset_trees_starts_every_rows_search_afresh(hip):
    board, N, seed, temp = (3, 3, 3), 6, 9, 2
    sp = new_async(hip, board, N, seed, temp_plies=temp, capacity=9, keep_tree=True)
    sp.advance(47)
    assert sp.carried.any() and (sp.fresh == 0).any()
    state = sp.state_dict()  # (what the rule beside it starts from: reset_trees changes none of it)
    sp.reset_trees()
    assert not sp.carried.any() and sp.fresh.tolist() == [1] * N
    plies = sp.row_plies.clone()
    rule = rule_from_state(state, N, temp, seed)
    both = KeepBeside(sp, rule, rule.begin())
    for r in range(40):
        both.advance(1, f"after the reset, {r}: ")
        still = (sp.row_plies == plies).cpu().numpy()  # rows whose next ply has not ended: their search began afresh
        assert not sp.carried.cpu().numpy()[still].any(), f"launch {r}"
    assert (sp.row_plies > plies).all() and sp.carried.any()
    assert_same_state(sp, rule)
    assert sp.env._err.tolist() == [0, 0]


# ----------------------------------------------------------------------------- 7. off is off
def test_without_keep_tree_the_player_is_what_it_was(hip):
    board, N, rounds = (9, 9, 5), 5, 40

    def new(**kw):
        sp = new_async(hip, board, N, 6, leaf_dtype=torch.uint8, temp_plies=6, capacity=81, root_noise=NOISE, solver=True,
                       **kw)
        sp.workspace.zero_()
        sp._begin()
        return sp

    old, sp = new(), new(keep_tree=False)
    assert sp.carried is None and sp.tree_nodes == sp.iterations + 1 and sp.workspace.shape == old.workspace.shape
    old.advance(rounds)
    sp.advance(rounds)
    torch.cuda.synchronize()
    same_players(sp, old)
    assert torch.equal(sp.workspace, old.workspace) and torch.equal(sp.row_plies, old.row_plies)
    assert torch.equal(sp.leaf_obs, old.leaf_obs) and torch.equal(sp.leaf_mask, old.leaf_mask)
    assert torch.equal(sp.fresh, old.fresh) and torch.equal(sp.root_priors, old.root_priors)
    assert len(set(old.row_plies.tolist())) > 1 and old.row_plies.min().item() > 0
    assert sp.env._err.tolist() == [0, 0]
