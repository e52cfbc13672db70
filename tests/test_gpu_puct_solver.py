"""GPU: the PUCT player that proves wins, draws and losses -- ``mnk_puct_step_solver`` through
``PUCTSearchPolicy(solver=True).act`` bit for bit against the numpy rule (tests/puct_solver_rule.py): actions, adjusted
visits, root values, proofs and every evaluation's leaf rows, on the single-word, sibling, generic, two-trip and multi-word
boards, one leaf and four, both temperatures, narrow priors; the misled search put right; a kept tree that arrives at
roots its proofs decide; a captured act; ``SearchSelfPlay(solver=True)``; the solver off against the old entry points;
and a guard on the strength of the player.  (What the positions hold is checked on the CPU,
tests/test_puct_solver_cpu.py.)"""
import numpy as np
import pytest
import torch

from player_cases import DEV, _score, hip  # noqa: F401 (hip: the fixture)
from puct_solver_cases import (C_PUCT, CASES, ENV_ID0, LEAVES, MISLED_BOARD, MISLED_FAR, MISLED_I, MISLED_OBS, MISLED_WIN,
                               REUSE_CASES, SEED, misled_reference, misled_tables, positions, reference, reuse_reference)
from puct_solver_rule import PROOF_UNKNOWN, SolverPuct
from search_selfplay_rule import SelfPlayRule
from test_gpu_puct_reuse import exact_np, exact_torch, same, same_leaves

pytestmark = pytest.mark.gpu


def policy(hip, k, I, C, L, record=None, out_dtype=torch.float32, step=0, solver=True, **kw):
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(C, out_dtype, record), iterations=I, c=C_PUCT, seed=SEED,
                                      leaves=L, solver=solver, **kw)
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, step
    return pol


def gpu_act(pol, obs_np, **kw):
    """(actions, visits, root_value, carried, proof) of one act"""
    b, _, m, n = obs_np.shape
    visits = torch.full((b, m * n), -7, dtype=torch.int32, device=DEV)
    value = torch.full((b,), -7.0, device=DEV)
    carried = torch.full((b, 2), -7, dtype=torch.int32, device=DEV) if pol.reuse else None
    proof = torch.full((b,), -7, dtype=torch.int8, device=DEV) if pol.solver else None
    a = pol.act({"observation": torch.from_numpy(obs_np).to(DEV)}, visits=visits, root_value=value,
                **({"carried": carried} if pol.reuse else {}), **({"proof": proof} if pol.solver else {}), **kw)
    return (a.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(),
            carried.cpu().numpy() if pol.reuse else np.zeros((b, 2), np.int32),
            proof.cpu().numpy() if pol.solver else np.full(b, PROOF_UNKNOWN, np.int8))


def same_act(got, want, what):
    same(got, want, what)
    assert np.array_equal(got[4], want[4]), (what, "proof", got[4], want[4])


# ----------------------------------------------------------------------------- 1. an act
@pytest.mark.parametrize("temperature", [0, 1])
@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", list(CASES))
def test_an_act_equals_the_rule(hip, name, L, temperature):
    (m, n, k), rows, I = CASES[name]
    obs, want, leaves = reference(name, L, temperature)
    rec = []
    pol = policy(hip, k, I, m * n, L, rec, step=2, temperature=temperature)
    got = gpu_act(pol, obs)
    same_leaves(rec, leaves, (name, L))
    same_act(got, want, (name, L, temperature))
    assert set(np.unique(got[4])) <= {-1, 0, 1, PROOF_UNKNOWN}


@pytest.mark.parametrize("L", LEAVES)
def test_bfloat16_priors_and_values_on_one_board(hip, L):
    """(the evaluator's priors are powers of two and its values eighths: exact in bfloat16)"""
    (m, n, k), rows, I = CASES["9x9x5"]
    obs, want, leaves = reference("9x9x5", L)
    rec = []
    got = gpu_act(policy(hip, k, I, m * n, L, rec, torch.bfloat16, step=2), obs)
    same_leaves(rec, leaves, L)
    same_act(got, want, L)


# ----------------------------------------------------------------------------- 2. the misled search
def misled_torch(leaf_obs, leaf_mask):
    table = torch.from_numpy(misled_tables()).to(DEV)
    return leaf_mask.float() * table, torch.ones(len(leaf_mask), device=DEV)


@pytest.mark.parametrize("solver", [True, False])
def test_proofs_put_a_misled_search_right(hip, solver):
    pol = hip.policy.PUCTSearchPolicy(MISLED_BOARD[2], evaluator=misled_torch, iterations=MISLED_I, c=C_PUCT, seed=SEED,
                                      solver=solver)
    got = gpu_act(pol, MISLED_OBS, deterministic=True)
    same_act(got, misled_reference(solver), solver)
    if solver:
        assert got[0][0] == MISLED_WIN and got[4][0] == 1 and got[2][0] == 1.0
    else:
        assert got[0][0] == MISLED_FAR


# ----------------------------------------------------------------------------- 3. a kept tree
@pytest.mark.parametrize("distance", [1, 2])
@pytest.mark.parametrize("case", range(len(REUSE_CASES)))
def test_a_kept_tree_equals_the_rule(hip, case, distance):
    (m, n, k), rows, I, L = REUSE_CASES[case]
    plies, decided = reuse_reference(case, distance)
    assert decided >= 1  # a row arrived at a carried root that the proofs of the search before decide
    rec = []
    pol = policy(hip, k, I, m * n, L, rec, reuse=True)
    for ply, (obs, want, leaves) in enumerate(plies):
        del rec[:]
        got = gpu_act(pol, obs)
        same_leaves(rec, leaves, (case, distance, ply))
        same_act(got, want, (case, distance, ply))


# ----------------------------------------------------------------------------- 4. capture
def test_a_captured_act_replayed_equals_eager(hip):
    (m, n, k), rows, I = CASES["9x9x5"]
    C, L = m * n, 4
    obs_np, want, _ = reference("9x9x5", L)
    pol = policy(hip, k, I, C, L)
    pol._sampler.step_dev = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    obs = torch.zeros((rows, 2, m, n), device=DEV)
    visits = torch.zeros((rows, C), dtype=torch.int32, device=DEV)
    value = torch.zeros(rows, device=DEV)
    proof = torch.zeros(rows, dtype=torch.int8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act({"observation": obs})  # eager, on empty boards: the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        actions = pol.act({"observation": obs}, visits=visits, root_value=value, proof=proof)
    obs.copy_(torch.from_numpy(obs_np))
    graph.replay()
    torch.cuda.synchronize()
    got = (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), np.zeros((rows, 2), np.int32),
           proof.cpu().numpy())
    same_act(got, want, "replay")


# ----------------------------------------------------------------------------- 5. search self-play
@pytest.mark.parametrize("reuse", [False, True])
def test_search_selfplay_with_the_solver_equals_the_rule(hip, reuse):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k, N, I, L, plies = 3, 3, 3, 6, 12, 2, 12
    C, T, temp_plies, seed = m * n, m * n, 2, 13
    sp = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=I, c=C_PUCT, temp_plies=temp_plies, capacity=T,
                        seed=seed, device=DEV, reuse=reuse, leaves=L, solver=True)
    assert sp.policy.solver
    sp.play(plies)
    rule, search = SelfPlayRule(m, n, k, N, T), SolverPuct(k, I, C_PUCT, exact_np(C), L, reuse=reuse, seed=seed)
    obs, mask = rule.view()
    proven = 0
    for p in range(plies):
        _, visits, _, _, proof = search.act(obs, step=p)
        proven += int((proof != PROOF_UNKNOWN).sum())
        obs, mask = rule.step(visits, temp_plies, seed, p)
    assert not rule.errors and proven
    assert np.array_equal(sp.buffer.planes.cpu().numpy().view(np.uint64), rule.ring_planes)
    assert np.array_equal(sp.buffer.visits.cpu().numpy().view(np.uint16), rule.ring_visits)
    assert np.array_equal(sp.buffer.z.cpu().numpy(), rule.ring_z)
    assert np.array_equal(sp.obs.cpu().numpy(), obs) and np.array_equal(sp.mask.cpu().numpy(), mask)
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist() and rule.stats[0] >= 1


# ----------------------------------------------------------------------------- 6. the solver off
def act_through_the_old_entry_points(hip, obs_np, k, I, L, step):
    """one act driven through the C ABI as it was before the solver: mnk_puct_begin[_leaves], mnk_puct_step[_leaves]"""
    lib = hip.lib
    b, _, m, n = obs_np.shape
    C = m * n
    ev = exact_torch(C)
    sfx, lv = ("_leaves", (L,)) if L > 1 else ("", ())
    obs = torch.from_numpy(obs_np).to(DEV)
    ws = torch.empty(lib.puct_workspace_bytes(b, m, n, I, L), dtype=torch.uint8, device=DEV)
    leaf_obs = torch.empty((b * L, 2, m, n), device=DEV)
    leaf_mask = torch.empty((b * L, C), dtype=torch.bool, device=DEV)
    actions = torch.empty(b, dtype=torch.long, device=DEV)
    visits = torch.full((b, C), -7, dtype=torch.int32, device=DEV)
    value = torch.full((b,), -7.0, device=DEV)
    stream = lib.stream_ptr(DEV)
    lib.call("mnk_puct_begin" + sfx, lib.ptr(obs), lib.OBS_F32, b, m, n, k, I, *lv, lib.ptr(ws), lib.ptr(leaf_obs),
             lib.OBS_F32, lib.ptr(leaf_mask), stream)
    for it in range(I // L + 1):
        priors, values = ev(leaf_obs, leaf_mask)
        priors, values = priors.contiguous(), values.contiguous()
        last = it == I // L
        lib.call("mnk_puct_step" + sfx, lib.ptr(ws), b, m, n, k, I, *lv, lib.ptr(priors), lib.LOGITS_F32, lib.ptr(values),
                 lib.LOGITS_F32, C_PUCT, int(last), 0, SEED, None, step, None, ENV_ID0, 0, lib.ptr(leaf_obs), lib.OBS_F32,
                 lib.ptr(leaf_mask), lib.ptr(actions) if last else None, lib.ptr(visits) if last else None,
                 lib.ptr(value) if last else None, stream)
    torch.cuda.synchronize()
    return (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), np.zeros((b, 2), np.int32),
            np.full(b, PROOF_UNKNOWN, np.int8))


@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", ["3x3x3", "9x9x5"])
def test_with_the_solver_off_an_act_is_the_old_entry_points(hip, name, L, monkeypatch):
    (m, n, k), rows, I = CASES[name]
    obs = positions(name)
    want = act_through_the_old_entry_points(hip, obs, k, I, L, 2)
    called = []
    call = hip.lib.call
    monkeypatch.setattr(hip.lib, "call", lambda entry, *args: (called.append(entry), call(entry, *args))[1])
    pol = policy(hip, k, I, m * n, L, step=2, solver=False)
    got = gpu_act(pol, obs)
    same_act(got, want, (name, L))
    sfx = "_leaves" if L > 1 else ""
    assert called == ["mnk_puct_begin" + sfx] + ["mnk_puct_step" + sfx] * (I // L + 1), called
    with pytest.raises(ValueError, match="solver=True"):
        pol.act({"observation": torch.from_numpy(obs).to(DEV)}, proof=torch.zeros(rows, dtype=torch.int8, device=DEV))
    # and the search with proofs is another search on these rows
    assert not np.array_equal(reference(name, L)[1][1], want[1])


# ----------------------------------------------------------------------------- 7. strength
SOLVER_MIN = 0.5 - 5 * 0.03125


def test_the_solver_does_not_weaken_the_player_on_9x9x5(hip):
    """PUCT(256, solver=True) against PUCT(256), both on the heuristic evaluator of tests/test_gpu_puct.py, 256 games
    (half as black).  The standard error is at most 0.5 / sqrt(256) = 0.03125 and the threshold lies 5 of them below
    one half: a guard against a solver that weakens the player, not a claim of strength.  Measured on the MI355X: 0.5391
    (133 W / 10 D / 113 L), 1.3 standard errors above one half"""
    from test_gpu_puct import heuristic_evaluator

    pol = hip.policy
    solver = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=14, solver=True)
    plain = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=15)
    res = hip.tournament.play_match(solver, plain, (9, 9, 5), 256, device=DEV)
    print("PUCT(256, solver)-PUCT(256) %.4f (%d W / %d D / %d L)" % (res["score"], res["wins"], res["draws"], res["losses"]))
    assert res["wins"] + res["losses"] + res["draws"] == 256
    assert res["score"] > SOLVER_MIN, res
