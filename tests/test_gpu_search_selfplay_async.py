"""GPU: search self-play with per-row budgets -- ``AsyncSearchSelfPlay`` / ``mnk_search_selfplay_advance``.  With every ply
full it must leave, bit for bit, what the lockstep ``SearchSelfPlay`` of the same seed leaves; with mixed budgets it is
compared round by round with the numpy rule (tests/search_selfplay_async_rule.py) on built-in and generic boards, every
leaf dtype, bf16 priors and values and a device key word, the large boards from states near the end of games; a captured
round replayed; a ``state_dict`` round trip; the refusals of the host and the row without a legal cell."""
import functools
import os

import numpy as np
import pytest
import torch

import search_selfplay_async_keep_cases as keep_cases
from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from search_selfplay_async_rule import AsyncSelfPlayRule, exact_np

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_selfplay_async_starts.npz")
FULL, FAST, THRESHOLD = 6, 2, 3 * 2 ** 30  # the mixed budgets: a ply is full with probability 3/4


def exact_torch(C, out_dtype=torch.float32):
    """a capturable evaluator of plain torch ops: dyadic per-cell priors on the legal cells, a value from stone counts
    (every number a multiple of 1/16 below 2: exact in bfloat16 too)"""
    table = (((torch.arange(C) * 37) % 16 + 1).float() / 16).to(DEV)

    def evaluate(leaf_obs, leaf_mask):
        cnt = leaf_obs.float().reshape(len(leaf_obs), 2, -1).sum(dim=2)
        priors, values = leaf_mask.float() * table, (torch.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5) - 2) / 4
        return priors.to(out_dtype), values.to(out_dtype)

    return evaluate


def new_async(hip, board, N, seed, full=FULL, fast=FAST, full_prob=0.75, leaf_dtype=torch.float32,
              out_dtype=torch.float32, evaluator=None, **kw):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    m, n, k = board
    return AsyncSearchSelfPlay(m, n, k, N, evaluator=evaluator or exact_torch(m * n, out_dtype), iterations=full,
                               fast_iterations=fast,
                               full_prob=full_prob, seed=seed, leaf_dtype=leaf_dtype, **kw)


def assert_same_state(sp, rule, what=""):
    """ring, env, ply counts, statistics and the device's count of written plies against the rule"""
    buf = sp.buffer
    assert np.array_equal(buf.planes.cpu().numpy().view(np.uint64), rule.ring_planes), what + " ring planes"
    assert np.array_equal(buf.visits.cpu().numpy().view(np.uint16), rule.ring_visits), what + " ring visits"
    assert np.array_equal(buf.z.cpu().numpy(), rule.ring_z), what + " ring z"
    assert np.array_equal(sp.env._planes.cpu().numpy().view(np.uint64), rule.planes()), what + " env planes"
    assert np.array_equal(sp.env._meta.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, rule.meta()), what + " env meta"
    assert sp.row_plies.tolist() == rule.row_plies.tolist(), what + " row_plies"
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist(), what + " stats"
    assert buf.plies.item() == rule.plies_max, what + " plies_max"


# ----------------------------------------------------------------------------- 1. every ply full: the lockstep player
@pytest.mark.parametrize("board,N,plies,capacity", [((3, 3, 3), 6, 2 * 9 + 5, None), ((9, 9, 5), 5, 81 + 5, 81),
                                                    ((17, 17, 5), 5, 6, None)])  # (ten words, a few plies)
def test_with_every_ply_full_it_is_the_lockstep_player(hip, board, N, plies, capacity):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    I = 6
    lock = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(m * n), iterations=I, seed=13, temp_plies=3, capacity=capacity)
    lock.play(plies)
    sp = new_async(hip, board, N, 13, full=I, fast=None, full_prob=1.0, temp_plies=3, capacity=capacity)
    sp.advance(plies * (I + 1))
    torch.cuda.synchronize()
    for t in ("planes", "visits", "z", "plies"):
        assert torch.equal(getattr(sp.buffer, t), getattr(lock.buffer, t)), t
    assert torch.equal(sp.env._planes, lock.env._planes) and torch.equal(sp.env._meta, lock.env._meta)
    assert torch.equal(sp.stats.sum(dim=0), lock.stats.sum(dim=0))
    assert torch.equal(sp.leaf_obs, lock.obs) and torch.equal(sp.leaf_mask, lock.mask)  # the next roots
    assert sp.fresh.tolist() == [1] * N and sp.row_plies.tolist() == [plies] * N
    assert sp.buffer.plies.item() == plies
    assert lock.pop_game_stats() == sp.pop_game_stats() and lock.buffer.visits.any()


# ----------------------------------------------------------------------------- 2. mixed budgets against the rule
# board, rows, leaf dtype, dtype of priors and values, device key word, temp_plies, rounds, start ("golden": a stored env
# state near the end of games), seed.  The seeds were chosen on the CPU with the rule so that in every case a game ends
# and fast and full plies are recorded; the small boards run more than two laps of their T = C ring.
CASES = [
    ((3, 3, 3), 7, torch.float32, torch.float32, False, 2, 130, None, 6),
    ((9, 9, 5), 5, torch.bfloat16, torch.float32, False, 6, 1150, None, 6),
    ((7, 7, 4), 5, torch.uint8, torch.float32, True, 4, 700, None, 6),
    ((12, 12, 5), 3, torch.float32, torch.bfloat16, False, 4, 150, "golden", 6),
    ((19, 19, 5), 3, torch.float32, torch.float32, False, 4, 150, "golden", 6),
    # boards that share a built-in variant with a board of another row count (tests/test_gpu_variant_siblings.py), from
    # the empty board.  The rule gives 46 games, 122 fast and 345 full records, row plies 65..69 on 8x3x3 and 14 games,
    # 193 fast and 559 full records, row plies 148..156 on 7x9x5
    ((8, 3, 3), 7, torch.uint8, torch.bfloat16, True, 2, 400, None, 6),
    ((7, 9, 5), 5, torch.bfloat16, torch.float32, False, 6, 900, None, 6),
    # and from stored states: three rows after 30 / 70 / 120 / 150 plies of random play and two rows two stones short of a
    # drawn board, which fill and are drawn at m * n stones (make_golden_search_selfplay_async.py) -- where a rule with the
    # variant's own cell count goes another way (tests/test_search_selfplay_async_cpu.py)
    ((7, 9, 5), 5, torch.float32, torch.float32, False, 4, 150, "golden", 6),
    ((12, 13, 5), 5, torch.uint8, torch.float32, False, 4, 150, "golden", 6),
    ((16, 15, 5), 5, torch.float32, torch.bfloat16, True, 4, 150, "golden", 6),
    ((18, 19, 5), 5, torch.bfloat16, torch.float32, False, 4, 150, "golden", 6),
    # the generic forms of sixteen and of thirty-two words: ten and 21 words a plane (an odd count: a ring row of planes
    # is no whole number of 64-bit words a plane), 289- and 625-byte leaf rows, from a computed start ("late": five rows
    # three to eight stones short of a drawn board)
    ((17, 17, 5), 5, torch.uint8, torch.float32, False, 4, 150, "late", 6),
    ((25, 25, 5), 5, torch.bfloat16, torch.float32, True, 4, 150, "late", 6),
]
LARGE_CASES = CASES[-2:]
SIBLING_BOARDS = ((8, 3, 3), (7, 9, 5), (12, 13, 5), (16, 15, 5), (18, 19, 5))
SIBLING_CASES = [case for case in CASES if case[0] in SIBLING_BOARDS]
ENV_ID0 = 3


def start_state(board, start):
    return keep_cases.start_state(board, start)  # (None, "golden", or "late": computed, five rows)


def new_rule(board, N, temp, seed, start, T=None):
    m, n, k = board
    rule = AsyncSelfPlayRule(m, n, k, N, T or m * n, FULL, FAST, THRESHOLD, 1.25, temp, seed, ENV_ID0)
    state = start_state(board, start)
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule


@functools.lru_cache(maxsize=None)
def rule_trace(board, N, temp, rounds, start, seed):
    """the rule's run of a case, computed once: (rule at the end, [(leaf_obs, leaf_mask, fresh) of every round])"""
    rule = new_rule(board, N, temp, seed, start)
    ev = exact_np(rule.C)
    obs, mask = rule.view()
    trace = []
    for _ in range(rounds):
        obs, mask, fresh = rule.advance(*ev(obs, mask))
        trace.append((obs, mask, fresh))
    return rule, trace


def load_start(sp, board, start):
    state = start_state(board, start)
    if state is not None:
        s = sp.state_dict()
        s["env"]["planes"] = torch.from_numpy(state[0].view(np.int64))
        s["env"]["meta"] = torch.from_numpy(state[1].astype(np.int64)).to(s["env"]["meta"].dtype)
        sp.load_state_dict(s)


@pytest.mark.parametrize("board,N,leaf_dtype,out_dtype,key_word,temp,rounds,start,seed", CASES)
def test_mixed_budgets_equal_the_rule_round_by_round(hip, board, N, leaf_dtype, out_dtype, key_word, temp, rounds, start,
                                                     seed):
    m, n, k = board
    assert N % 4  # a partial workgroup
    rule, trace = rule_trace(board, N, temp, rounds, start, seed)
    sp = new_async(hip, board, N, seed + 100 if key_word else seed, leaf_dtype=leaf_dtype, out_dtype=out_dtype,
                   temp_plies=temp, capacity=m * n)
    sp.sampler.env_id0 = ENV_ID0
    if key_word:  # the device word replaces the host's key
        sp.sampler.seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    load_start(sp, board, start)
    assert sp.full_threshold == THRESHOLD
    for r, (obs, mask, fresh) in enumerate(trace):
        sp.advance(1)
        assert sp.leaf_obs.dtype == leaf_dtype
        assert np.array_equal(sp.leaf_obs.float().cpu().numpy(), obs), f"leaves, round {r}"
        assert np.array_equal(sp.leaf_mask.cpu().numpy(), mask), f"masks, round {r}"
        assert sp.fresh.tolist() == fresh.tolist(), f"fresh, round {r}"
    assert_same_state(sp, rule)
    assert sp.env._err.tolist() == [0, 0] and not rule.errors
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0
    assert len(set(rule.row_plies.tolist())) > 1  # the rows are out of step
    if start is None:
        assert rule.row_plies.min() > 2 * m * n  # more than two laps of the ring
    assert sp.buffer.plies_host == rounds >= sp.buffer.plies.item()  # the host's count is an upper bound


# ----------------------------------------------------------------------------- 3. a captured round
def test_a_captured_round_replayed_equals_eager_rounds(hip):
    R, board, N, seed = 90, (3, 3, 3), 6, 21
    def new():
        # (the workspace is compared whole below, and it is allocated uninitialised: the bytes no kernel writes are
        # what an earlier tensor left there, so both start from zeros and set their roots up again)
        sp = new_async(hip, board, N, seed, temp_plies=2, capacity=9)
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
    for t in ("planes", "visits", "z", "plies"):
        assert torch.equal(getattr(sp.buffer, t), getattr(eager.buffer, t)), t
    assert torch.equal(sp.env._planes, eager.env._planes) and torch.equal(sp.env._meta, eager.env._meta)
    assert torch.equal(sp.row_plies, eager.row_plies) and torch.equal(sp.stats, eager.stats)
    assert torch.equal(sp.leaf_obs, eager.leaf_obs) and torch.equal(sp.leaf_mask, eager.leaf_mask)
    assert torch.equal(sp.fresh, eager.fresh) and torch.equal(sp.workspace, eager.workspace)
    assert sp.buffer.plies_host == eager.buffer.plies_host == 1 + R
    assert len(set(eager.row_plies.tolist())) > 1 and eager.pop_game_stats()["games"] > 0


# ----------------------------------------------------------------------------- 4. state_dict
def test_a_restored_state_continues_as_the_rule_does(hip):
    board, N, seed, temp, before, after = (3, 3, 3), 6, 9, 2, 47, 60
    a = new_async(hip, board, N, seed, temp_plies=temp, capacity=9)
    a.advance(before)
    state = a.state_dict()
    b = new_async(hip, board, N, seed + 1, temp_plies=0, capacity=9)
    b.load_state_dict(state)
    assert b.fresh.tolist() == [1] * N and b.temp_plies == temp and b.sampler.seed == seed
    # the rule, loaded from the same state: SelfPlayRule.load, the ring, the ply counts, then fresh trees
    rule = AsyncSelfPlayRule(3, 3, 3, N, 9, FULL, FAST, THRESHOLD, 1.25, temp, seed)
    rule.load(state["env"]["planes"].numpy().view(np.uint64), state["env"]["meta"].numpy())
    rule.ring_planes[:] = state["buffer"]["planes"].numpy().view(np.uint64)
    rule.ring_visits[:] = state["buffer"]["visits"].numpy().view(np.uint16)
    rule.ring_z[:] = state["buffer"]["z"].numpy()
    rule.row_plies[:] = state["row_plies"].numpy()
    rule.plies_max = int(state["buffer"]["plies"].item())
    rule.stats[:] = state["stats"].sum(dim=0)[:5].numpy()
    assert len(set(rule.row_plies.tolist())) > 1  # saved in the middle of searches that were out of step
    obs, mask = rule.begin()
    ev = exact_np(9)
    for r in range(after):
        obs, mask, fresh = rule.advance(*ev(obs, mask))
        b.advance(1)
        assert np.array_equal(b.leaf_obs.cpu().numpy(), obs) and b.fresh.tolist() == fresh.tolist(), f"round {r}"
    assert_same_state(b, rule)
    assert b.pop_game_stats()["games"] > 0


# ----------------------------------------------------------------------------- 5. refusals
# entry point: (the player's options, the argument index of `leaves` or None, has temp_plies, {its own arguments after
# `err`, by offset: (what the player passes there -- checked, so that a moved argument fails here --, one bad value)})
KEEP_NODES = lambda sp: sp.tree_nodes - sp.iterations  # noqa: E731
ENTRY_POINTS = {
    "mnk_search_selfplay_advance": ({}, None, True, {}),
    "mnk_search_selfplay_advance_opts": ({"solver": True}, None, True, {0: (1, 2)}),                      # solver
    "mnk_search_selfplay_advance_opts_fpu": ({"solver": True, "fpu": 0.25}, None, True, {0: (1, 2), 5: (0.25, -1.0)}),  # fpu
    "mnk_search_selfplay_advance_keep": ({"keep_tree": True}, None, True, {6: (KEEP_NODES, 0)}),          # keep_nodes
    "mnk_search_selfplay_advance_keep_fpu": ({"keep_tree": True, "fpu": 0.25}, None, True,
                                             {6: (KEEP_NODES, 0), 8: (0.25, -1.0)}),
    "mnk_search_selfplay_advance_leaves": ({"leaves": 2}, 9, True, {0: (0, 2)}),                          # solver; leaves below
    "mnk_search_selfplay_advance_gumbel": ({"gumbel": 4}, None, False, {0: (4, 0)}),                      # considered
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_the_host_refuses_bad_budgets_before_anything_is_enqueued(hip, name):
    lib = hip.lib
    options, at_leaves, has_temp, own = ENTRY_POINTS[name]
    sp = new_async(hip, (3, 3, 3), 5, 1, capacity=9, **options)
    # the argument list of the player's own call of the entry point
    seen, inner = [], lib.call
    lib.call = lambda fn, *a: (seen.append((fn, a)), inner(fn, *a))[1]
    try:
        sp.advance(3)
    finally:
        lib.call = inner
    assert {fn for fn, _ in seen if fn.startswith("mnk_search_selfplay_advance")} == {name}
    good = list([a for fn, a in seen if fn == name][-1])
    torch.cuda.synchronize()
    before = [t.clone() for t in (sp.workspace, sp.row_plies, sp.leaf_obs, sp.buffer.z, sp.env._meta)]
    priors, values = exact_torch(9)(sp.leaf_obs, sp.leaf_mask)
    priors, values = priors.contiguous(), values.contiguous()
    # where the arguments stand: iterations, fast_iterations, [leaves,] full_threshold, priors, .., values, ..,
    # [temp_plies,] .., T, .., err, then the entry point's own
    shift = 0 if at_leaves is None else 1
    FULL_AT, FAST_AT, THRESHOLD_AT, PRIORS_AT, VALUES_AT = 7, 8, 9 + shift, 10 + shift, 12 + shift
    T_AT = 19 + shift + (1 if has_temp else 0)
    OWN_AT = T_AT + 11
    good[PRIORS_AT], good[VALUES_AT] = lib.ptr(priors), lib.ptr(values)
    assert good[FULL_AT] == FULL and good[FAST_AT] == FAST and good[THRESHOLD_AT] == THRESHOLD and good[T_AT] == 9

    def adv(changed=()):
        args = list(good)
        for at, value in dict(changed).items():
            args[at] = value
        return getattr(lib.load(), name)(*args)

    EINVAL = -1
    assert adv({T_AT: 8}) == EINVAL and adv({FAST_AT: FULL + 1}) == EINVAL and adv({FAST_AT: 0}) == EINVAL
    assert adv({THRESHOLD_AT: 2 ** 32 + 1}) == EINVAL
    for offset, (passed, bad) in own.items():
        assert good[OWN_AT + offset] == (passed(sp) if callable(passed) else passed), (name, offset)
        assert adv({OWN_AT + offset: bad}) == EINVAL, (name, offset)
    if at_leaves is not None:
        assert good[at_leaves] == 2 and adv({at_leaves: 4}) == EINVAL  # (4 does not divide 6 iterations)
    torch.cuda.synchronize()
    for was, now in zip(before, (sp.workspace, sp.row_plies, sp.leaf_obs, sp.buffer.z, sp.env._meta)):
        assert torch.equal(was, now)
    assert adv() == 0 and adv({THRESHOLD_AT: 2 ** 32}) == 0 and adv({THRESHOLD_AT: 0, FAST_AT: 1}) == 0


def test_a_root_without_a_legal_cell_is_reported_and_left_alone(hip):
    lib = hip.lib
    N = 5
    sp = new_async(hip, (3, 3, 3), N, 4, capacity=9)
    s = sp.state_dict()
    # row 2 holds a full board without a run (x o x / x o o / o x x), handed in by state
    black, white = [0, 2, 3, 7, 8], [1, 4, 5, 6]
    bits = lambda cells: sum(1 << (a + a // 3) for a in cells)  # noqa: E731
    s["env"]["planes"][0, 0, 2], s["env"]["planes"][1, 0, 2] = bits(black), bits(white)
    s["env"]["meta"][2] = (9 << 1) | 1
    sp.load_state_dict(s)
    sp.advance(25)
    torch.cuda.synchronize()
    assert sp.env._err.tolist() == [lib.ERR_VISITS, 2]
    assert sp.row_plies[2].item() == 0 and sp.fresh[2].item() == 0 and (sp.row_plies > 0).sum().item() == N - 1
    assert sp.env._meta[2].item() == (9 << 1) | 1
    assert sp.env._planes[:, 0, 2].tolist() == [bits(black), bits(white)]
    assert (sp.buffer.z[:, 2] == lib.Z_UNKNOWN).all() and not sp.buffer.visits[:, 2].any()
    assert sp.leaf_mask[2].sum().item() == 0 and sp.leaf_obs[2].sum().item() == 9  # its root, shown again
    sp.env._err.zero_()


@pytest.mark.parametrize("options", [{"root_noise": (0.3, 0.25), "solver": True}, {"keep_tree": True}, {"leaves": 2}],
                         ids=["opts", "keep", "leaves"])
def test_every_form_reports_a_root_without_a_legal_cell_and_leaves_it_alone(hip, options):
    """the same row in the kernels with the options, with kept trees and with two leaves per row: the error row is one
    piece of code, and every form must go through it"""
    lib = hip.lib
    N, L = 5, options.get("leaves", 1)
    sp = new_async(hip, (3, 3, 3), N, 4, capacity=9, **options)
    s = sp.state_dict()
    # row 2 holds a full board without a run (x o x / x o o / o x x), handed in by state
    black, white = [0, 2, 3, 7, 8], [1, 4, 5, 6]
    bits = lambda cells: sum(1 << (a + a // 3) for a in cells)  # noqa: E731
    s["env"]["planes"][0, 0, 2], s["env"]["planes"][1, 0, 2] = bits(black), bits(white)
    s["env"]["meta"][2] = (9 << 1) | 1
    sp.load_state_dict(s)
    if L > 1:
        sp.row_sims[2] = 5  # (a count that no ply of this run leaves behind)
    sp.advance(25)
    torch.cuda.synchronize()
    assert sp.env._err.tolist() == [lib.ERR_VISITS, 2]
    assert sp.row_plies[2].item() == 0 and sp.fresh[2].item() == 0 and (sp.row_plies > 0).sum().item() == N - 1
    assert sp.env._meta[2].item() == (9 << 1) | 1
    assert sp.env._planes[:, 0, 2].tolist() == [bits(black), bits(white)]
    assert (sp.buffer.z[:, 2] == lib.Z_UNKNOWN).all() and not sp.buffer.visits[:, 2].any()
    for b in range(2 * L, 2 * L + L):  # its root, shown again in every batch row of the row
        assert sp.leaf_mask[b].sum().item() == 0 and sp.leaf_obs[b].sum().item() == 9
    if L > 1:
        assert sp.row_sims[2].item() == 5
    sp.env._err.zero_()
