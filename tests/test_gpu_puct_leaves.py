"""GPU: the PUCT player with several leaves per row and evaluation -- ``mnk_puct_begin_leaves`` / ``mnk_puct_rebase_leaves``
/ ``mnk_puct_step_leaves`` through ``PUCTSearchPolicy(leaves=L).act`` bit for bit against the numpy rule
(tests/puct_leaves_rule.py): actions, root visits, root values and every evaluation's leaf rows, void slots included, on
built-in and generic boards, every L, a single round and the largest budget; one leaf through the new entry points
against the old ones; a kept tree over sequences of plies; a captured act; narrow dtypes; ``SearchSelfPlay(leaves=4)``;
and a guard on the strength of the player under virtual loss.  (That the cases reach void slots, repeated terminals and
shared prefixes is checked on the CPU, tests/test_puct_leaves_cpu.py.)"""
import numpy as np
import pytest
import torch

from player_cases import DEV, _score, hip  # noqa: F401 (hip: the fixture)
from puct_leaves_cases import C_PUCT, CASES, ENV_ID0, LARGE, PARAMS, SEED, positions, reference
from puct_leaves_rule import LeavesPuct
from search_selfplay_rule import SelfPlayRule
from test_gpu_puct_reuse import advance, exact_np, exact_torch, gpu_act, same, same_leaves, start

pytestmark = pytest.mark.gpu


def policy(hip, k, I, C, L, record=None, leaf_dtype=torch.float32, out_dtype=torch.float32, refresh=False, step=0, **kw):
    ev = exact_torch(C, out_dtype, record, I // L if refresh else None)
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=ev, iterations=I, c=C_PUCT, leaf_dtype=leaf_dtype, seed=SEED, leaves=L,
                                      **kw)
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, step
    return pol


# ----------------------------------------------------------------------------- 1. every board, budget and L
@pytest.mark.parametrize("name,L", PARAMS)
def test_an_act_equals_the_rule(hip, name, L):
    (m, n, k), rows, I, _ = CASES[name]
    obs, want, leaves, trace = reference(name, L)
    rec = []
    pol = policy(hip, k, I, m * n, L, rec, step=2)
    assert pol.evaluations_per_act == I // L + 1
    got = gpu_act(pol, obs)
    assert len(rec) == I // L + 1 and rec[0][0].shape == (rows * L, 2, m, n)
    same_leaves(rec, leaves, (name, L))
    same(got, want + (np.zeros((rows, 2), np.int32),), (name, L))
    for i, tr in enumerate(trace):
        assert got[1][i].sum() == (I - tr["void"] if tr["live"] else 0), (name, L, i)


# ----------------------------------------------------------------------------- 2. one leaf: the new entry points and the old
def act_through_the_leaves_entry_points(hip, obs_np, k, I, L, temperature, step):
    """one act driven through the C ABI (PUCTSearchPolicy stays on the old entry points at one leaf)"""
    lib = hip.lib
    b, _, m, n = obs_np.shape
    C = m * n
    rec = []
    ev = exact_torch(C, torch.float32, rec)
    obs = torch.from_numpy(obs_np).to(DEV)
    ws = torch.empty(lib.puct_workspace_bytes(b, m, n, I, L), dtype=torch.uint8, device=DEV)
    leaf_obs = torch.empty((b * L, 2, m, n), device=DEV)
    leaf_mask = torch.empty((b * L, C), dtype=torch.bool, device=DEV)
    actions = torch.empty(b, dtype=torch.long, device=DEV)
    visits = torch.full((b, C), -7, dtype=torch.int32, device=DEV)
    value = torch.full((b,), -7.0, device=DEV)
    stream = lib.stream_ptr(DEV)
    lib.call("mnk_puct_begin_leaves", lib.ptr(obs), lib.OBS_F32, b, m, n, k, I, L, lib.ptr(ws), lib.ptr(leaf_obs),
             lib.OBS_F32, lib.ptr(leaf_mask), stream)
    for it in range(I // L + 1):
        priors, values = ev(leaf_obs, leaf_mask)
        priors, values = priors.contiguous(), values.contiguous()
        last = it == I // L
        lib.call("mnk_puct_step_leaves", lib.ptr(ws), b, m, n, k, I, L, lib.ptr(priors), lib.LOGITS_F32, lib.ptr(values),
                 lib.LOGITS_F32, C_PUCT, int(last), temperature, SEED, None, step, None, ENV_ID0, 0, lib.ptr(leaf_obs),
                 lib.OBS_F32, lib.ptr(leaf_mask), lib.ptr(actions) if last else None, lib.ptr(visits) if last else None,
                 lib.ptr(value) if last else None, stream)
    torch.cuda.synchronize()
    return (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), np.zeros((b, 2), np.int32)), rec


@pytest.mark.parametrize("temperature", [0, 1])
@pytest.mark.parametrize("name", ["3x3x3", "4x6x3", "9x9x5", "19x19x5"])
def test_one_leaf_through_the_new_entry_points_equals_the_old(hip, name, temperature):
    (m, n, k), rows, I, _ = CASES[name]
    obs = positions(name)
    rec = []
    old = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(m * n, torch.float32, rec), iterations=I, c=C_PUCT,
                                      seed=SEED, temperature=temperature)
    old._sampler.env_id0, old._sampler.calls = ENV_ID0, 4
    want = gpu_act(old, obs)
    got, rec1 = act_through_the_leaves_entry_points(hip, obs, k, I, 1, temperature, 4)
    same_leaves(rec1, rec, (name, temperature))
    same(got, want, (name, temperature))


# ----------------------------------------------------------------------------- 3. a kept tree
@pytest.mark.parametrize("distance", [1, 2])
@pytest.mark.parametrize("board,rows,I", [((3, 3, 3), 6, 12), ((4, 6, 3), 5, 12), ((9, 9, 5), 6, 16)])
def test_a_sequence_of_plies_with_a_kept_tree_equals_the_rule(hip, board, rows, I, distance):
    """``reuse=True, leaves=4``: the next root one ply on (self-play) and two plies on (a wrapper's opponent), games that
    end and rows that are cleared inside the sequence.  One ply on, the evaluator answers the roots' call with other priors
    (on a carried root evaluation 0 renews the priors and nothing else); two plies on it answers alike every time, so
    that the second mover's lowest free cell is a child the search had tried and trees are carried on every board"""
    m, n, k = board
    C, L, plies = m * n, 4, 10
    rec, leaves = [], []
    refresh = distance == 1
    pol = policy(hip, k, I, C, L, rec, refresh=refresh, reuse=True)
    rule = LeavesPuct(k, I, C_PUCT, exact_np(C, I // L if refresh else None), L, reuse=True, seed=SEED, env_id0=ENV_ID0,
                      leaves=leaves)
    assert pol.tree_nodes == rule.tree_nodes == 2 * I + 1
    obs = start(m, n, k, rows, m * 100 + n * 10 + k + distance)
    resets, kept, fresh = np.zeros(rows, np.int64), 0, 0
    for ply in range(plies):
        del rec[:], leaves[:]
        want = rule.act(obs, step=ply)
        got = gpu_act(pol, obs)
        same_leaves(rec, leaves, (board, distance, ply))
        same(got, want, (board, distance, ply))
        kept += int((want[3][:, 0] > 1).sum())
        fresh += int(ply > 0 and (want[3][:, 0] == 0).sum())
        obs = advance(obs, want[0], k, distance, resets)
        if ply == plies // 2 and board != (3, 3, 3):
            obs[1::2] = 0
    assert kept and fresh, (kept, fresh)


# ----------------------------------------------------------------------------- 4. capture
def test_a_captured_act_replayed_equals_eager(hip):
    (m, n, k), rows, I, _ = CASES["9x9x5"]
    C, L = m * n, 4
    obs_np, want, _, _ = reference("9x9x5", L)
    pol = policy(hip, k, I, C, L)
    pol._sampler.step_dev = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    obs = torch.zeros((rows, 2, m, n), device=DEV)
    visits = torch.zeros((rows, C), dtype=torch.int32, device=DEV)
    value = torch.zeros(rows, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act({"observation": obs})  # eager, on empty boards: the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        actions = pol.act({"observation": obs}, visits=visits, root_value=value)
    obs.copy_(torch.from_numpy(obs_np))
    graph.replay()
    torch.cuda.synchronize()
    got = (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), np.zeros((rows, 2), np.int32))
    same(got, want + (np.zeros((rows, 2), np.int32),), "replay")


# ----------------------------------------------------------------------------- 5. dtypes
@pytest.mark.parametrize("dtype,leaf_dtype,out_dtype,L", [
    (torch.float32, torch.uint8, torch.bfloat16, 8), (torch.uint8, torch.bfloat16, torch.bfloat16, 2)])
def test_narrow_dtypes_on_one_board(hip, dtype, leaf_dtype, out_dtype, L, name="9x9x5"):
    """(the evaluator's priors are powers of two and its values eighths: exact in bfloat16)"""
    narrow_act_equals_the_rule(hip, name, dtype, leaf_dtype, out_dtype, L)


def narrow_act_equals_the_rule(hip, name, dtype, leaf_dtype, out_dtype, L):
    (m, n, k), rows, I, _ = CASES[name]
    obs, want, leaves, _ = reference(name, L)
    rec = []
    pol = policy(hip, k, I, m * n, L, rec, leaf_dtype, out_dtype, step=2)
    got = gpu_act(pol, obs, dtype)
    same_leaves(rec, leaves, (dtype, L))
    same(got, want + (np.zeros((rows, 2), np.int32),), (dtype, L))


@pytest.mark.parametrize("name", list(LARGE))
def test_narrow_leaves_on_the_large_generic_boards(hip, name):
    """``uint8`` leaf rows of 289 bytes and ``bfloat16`` ones of 625 elements: rows at odd offsets"""
    leaf_dtype = getattr(torch, LARGE[name])
    narrow_act_equals_the_rule(hip, name, torch.uint8 if leaf_dtype is torch.bfloat16 else torch.float32, leaf_dtype,
                               torch.bfloat16, 4)


# ----------------------------------------------------------------------------- 6. search self-play
@pytest.mark.parametrize("reuse", [False, True])
def test_search_selfplay_with_leaves_equals_the_rule(hip, reuse):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k, N, I, L, plies = 3, 3, 3, 6, 12, 4, 14
    C, T, temp_plies, seed = m * n, m * n, 2, 13
    sp = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=I, c=C_PUCT, temp_plies=temp_plies, capacity=T,
                        seed=seed, device=DEV, reuse=reuse, leaves=L)
    assert sp.policy.leaves == L and sp.policy.evaluations_per_act == I // L + 1
    sp.play(plies)
    rule, search = SelfPlayRule(m, n, k, N, T), LeavesPuct(k, I, C_PUCT, exact_np(C), L, reuse=reuse, seed=seed)
    obs, mask = rule.view()
    for p in range(plies):
        _, visits, _, _ = search.act(obs, step=p)
        obs, mask = rule.step(visits, temp_plies, seed, p)
    assert not rule.errors
    assert np.array_equal(sp.buffer.planes.cpu().numpy().view(np.uint64), rule.ring_planes)
    assert np.array_equal(sp.buffer.visits.cpu().numpy().view(np.uint16), rule.ring_visits)
    assert np.array_equal(sp.buffer.z.cpu().numpy(), rule.ring_z)
    assert np.array_equal(sp.obs.cpu().numpy(), obs) and np.array_equal(sp.mask.cpu().numpy(), mask)
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist() and rule.stats[0] >= N


# ----------------------------------------------------------------------------- 7. strength
LEAVES_MIN = 0.60


def test_virtual_loss_does_not_break_the_player_on_9x9x5(hip):
    """PUCT(256, leaves=8) against PUCT(256, leaves=1), both on the heuristic evaluator of tests/test_gpu_puct.py, 256
    games (half as black).  Measured on the MI355X: 0.7578 (189 W / 10 D / 57 L); the threshold lies 5 standard errors
    (0.031 each at 256 games) below that.  A guard against a broken virtual loss, not a claim about strength at equal
    budget"""
    from test_gpu_puct import heuristic_evaluator

    pol = hip.policy
    wide = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=14, leaves=8)
    one = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=15)
    score = _score(hip, wide, one, (9, 9, 5), 256)
    print("PUCT(256, leaves=8)-PUCT(256) %.4f" % score)
    assert score > LEAVES_MIN, score
