"""GPU: the PUCT player with forced playouts and policy target pruning -- ``mnk_puct_step_forced`` through
``PUCTSearchPolicy(forced=k).act`` bit for bit against the numpy rule (tests/puct_forced_rule.py): actions, ``visits`` (the
pruned counts), ``raw_visits``, root values, ``carried``, proofs and every evaluation's leaf rows, five rows (a partial
workgroup), on the single-word, two-trip, sibling, generic and multi-word boards, one leaf and four, the solver on and off,
with and without first-play urgency, both temperatures; a kept tree over three acts; root noise; bf16 priors and values; a
prior above 1 and a prior of 0 on a visited cell; a captured act replayed twice; and ``forced=None`` against the policy as it
was.  The cases are tests/puct_forced_cases.py's, where tests/test_puct_forced_cpu.py shows with the rule alone that each
forces and prunes."""
import numpy as np
import pytest
import torch

import puct_forced_cases as cases
from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from puct_forced_cases import BOARDS, C_PUCT, ENV_ID0, FPU, K_FORCED, OPTIONS, ROWS, SEED
from puct_noise_rule import root_noise
from puct_solver_rule import PROOF_UNKNOWN
from test_gpu_puct_reuse import same, same_leaves

pytestmark = pytest.mark.gpu


def spike_torch(C, spikes, spike=0.25, bad=1.0, zero=None, above=None, lost=False, out_dtype=torch.float32, record=None):
    """``puct_forced_cases.spike_np`` on the GPU, in plain torch ops (capturable when it does not record)"""
    table, mark = (torch.from_numpy(t).to(DEV) for t in cases.tables(C, spikes, spike, zero, above))

    def evaluate(leaf_obs, leaf_mask):
        if record is not None:
            record.append((leaf_obs.float().cpu().numpy(), leaf_mask.cpu().numpy()))
        o = leaf_obs.float().reshape(len(leaf_obs), 2, -1)
        own, opp = (o[:, 0] * mark).sum(dim=1), (o[:, 1] * mark).sum(dim=1)
        cnt = o.sum(dim=2)
        small = torch.full_like(own, 0.5) if lost else (2 - torch.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5)) / 16
        value = torch.where(opp > own, torch.full_like(own, bad), torch.where(own > opp, torch.full_like(own, -bad), small))
        return (leaf_mask.float() * table).to(out_dtype), value.to(out_dtype)

    return evaluate


def evaluator_of(name, **kw):
    (m, n, k), _, spike, bad = BOARDS[name]
    return spike_torch(m * n, cases.spikes_of(m, n, k)[:cases.SPIKES.get(name, 3)], spike, bad, **kw)


def policy(hip, name, L, solver, fpu, evaluator, step=2, forced=K_FORCED, **kw):
    (m, n, k), I, _, _ = BOARDS[name]
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=evaluator, iterations=I, c=C_PUCT, seed=SEED, leaves=L, solver=solver,
                                      fpu=fpu, forced=forced, **kw)
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, step
    return pol


def gpu_act(pol, obs_np):
    """((actions, visits, root_value, carried, proof), raw_visits) of one act"""
    b, _, m, n = obs_np.shape
    visits = torch.full((b, m * n), -7, dtype=torch.int32, device=DEV)
    raw = torch.full((b, m * n), -7, dtype=torch.int32, device=DEV) if pol.forced is not None else None
    value = torch.full((b,), -7.0, device=DEV)
    carried = torch.full((b, 2), -7, dtype=torch.int32, device=DEV) if pol.reuse else None
    proof = torch.full((b,), -7, dtype=torch.int8, device=DEV) if pol.solver else None
    a = pol.act({"observation": torch.from_numpy(obs_np).to(DEV)}, visits=visits, root_value=value,
                **({"carried": carried} if pol.reuse else {}), **({"proof": proof} if pol.solver else {}),
                **({"raw_visits": raw} if raw is not None else {}))
    return ((a.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(),
             carried.cpu().numpy() if pol.reuse else np.zeros((b, 2), np.int32),
             proof.cpu().numpy() if pol.solver else np.full(b, PROOF_UNKNOWN, np.int8)),
            raw.cpu().numpy() if raw is not None else None)


def same_act(got, want, raw, what):
    got, got_raw = got
    if raw is not None:
        assert np.array_equal(got_raw, raw), (what, "raw_visits", got_raw, raw)
    same(got, want, what)
    assert np.array_equal(got[4], want[4]), (what, "proof", got[4], want[4])


# ----------------------------------------------------------------------------- 1. an act
@pytest.mark.parametrize("L,solver,fpu,temperature", OPTIONS)
@pytest.mark.parametrize("name", list(BOARDS))
def test_an_act_equals_the_rule(hip, name, L, solver, fpu, temperature):
    obs, want, leaves, rule = cases.reference(name, L, solver, fpu, temperature)
    rec = []
    pol = policy(hip, name, L, solver, fpu, evaluator_of(name, record=rec), temperature=temperature)
    assert pol.forced == K_FORCED and pol.fpu == fpu
    got = gpu_act(pol, obs)
    same_leaves(rec, leaves, (name, L, solver, fpu))
    same_act(got, want, rule.raw_visits, (name, L, solver, fpu, temperature))
    assert not np.array_equal(got[0][1], got[1])  # (the CPU test's condition 2, on the device's own outputs)


# ----------------------------------------------------------------------------- 2. one board each
@pytest.mark.parametrize("L,solver", cases.REUSE)
def test_a_kept_tree_over_three_acts_equals_the_rule(hip, L, solver):
    """``tree_nodes`` lets a ply carry five nodes over, so a carried root's n_0 - 1 exceeds the sum of its kept children:
    t_a is made of the root's own count"""
    rec = []
    pol = policy(hip, cases.REUSE_NAME, L, solver, FPU, evaluator_of(cases.REUSE_NAME, record=rec), step=0, reuse=True,
                 tree_nodes=cases.REUSE_NODES)
    for ply, (obs, want, leaves, raw, _) in enumerate(cases.reuse_reference(L, solver)):
        del rec[:]
        got = gpu_act(pol, obs)
        same_leaves(rec, leaves, (L, ply))
        same_act(got, want, raw, (L, ply))


def test_root_noise_equals_the_rule_on_the_kernels_priors(hip):
    """forcing acts on the noised priors.  They are taken from the policy's own buffer (their comparison with numpy, to
    one part in 10^6, is tests/test_gpu_puct_noise.py's); the search on them is the rule's, bit for bit"""
    name, L, noise = "9x9x5", 4, (0.3, 0.25)
    obs, rec = cases.rows_of(name), []
    pol = policy(hip, name, L, True, FPU, evaluator_of(name, record=rec), root_noise=noise)
    got = gpu_act(pol, obs)
    noised = pol._bufs[4].cpu().numpy()
    base, calls, seen = cases.evaluator_of(name), [0], []

    def evaluator(leaf_obs, leaf_mask):
        priors, values = base(leaf_obs, leaf_mask)
        if calls[0] == 0:
            wanted = root_noise(priors[::L], leaf_mask[::L], *noise, SEED, 2, ENV_ID0)
            free = leaf_mask[::L]
            np.testing.assert_allclose(noised[::L][free], wanted[free], rtol=1e-6, atol=0)
            priors = priors.astype(np.float32).copy()
            priors[::L] = noised[::L]
        calls[0] += 1
        return priors, values

    rule = cases.new_rule(name, L, True, FPU, seen=seen, evaluator=evaluator)
    want = rule.act(obs, step=2)
    same_leaves(rec, seen, "noise")
    same_act(got, want, rule.raw_visits, "noise")
    assert any(taken != plain for taken, plain in rule.picks) and (rule.raw_visits != want[1]).any()
    assert not np.array_equal(want[1], cases.reference(name, L, True, FPU)[1][1])  # the noise changed the search


@pytest.mark.parametrize("L", [1, 4])
def test_bfloat16_priors_and_values(hip, L):
    """(the evaluator's priors are dyadic with at most two significant bits and its values sixteenths: exact in bfloat16)"""
    name = "9x9x5"
    obs, want, leaves, rule = cases.reference(name, L, True, FPU)
    rec = []
    got = gpu_act(policy(hip, name, L, True, FPU, evaluator_of(name, out_dtype=torch.bfloat16, record=rec)), obs)
    same_leaves(rec, leaves, L)
    same_act(got, want, rule.raw_visits, L)


@pytest.mark.parametrize("L,fpu", cases.LOSS_OPTIONS)
def test_a_proven_loss_short_of_its_floor_is_not_forced(hip, L, fpu):
    """the solver's clause of the forced test: rows whose root has children proven LOSS with n'^2 < k * P * S' at most of
    its selections (tests/test_puct_forced_cpu.py shows that, and that a selection without the clause searches another
    tree)"""
    obs, want, leaves, rule = cases.loss_reference(L, fpu)
    assert rule.shunned
    (m, n, k), _, spike, bad = BOARDS[cases.LOSS_NAME]
    rec = []
    got = gpu_act(policy(hip, cases.LOSS_NAME, L, True, fpu, spike_torch(m * n, cases.LOSS_SPIKES, spike, bad, record=rec)), obs)
    same_leaves(rec, leaves, ("loss", L, fpu))
    same_act(got, want, rule.raw_visits, ("loss", L, fpu))


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("which", list(cases.EDGES))
def test_a_prior_above_one_and_a_prior_of_zero_on_a_visited_cell(hip, which, L):
    obs, want, leaves, rule = cases.edge_reference(which, L)
    rec = []
    got = gpu_act(policy(hip, cases.EDGE_NAME, L, False, None, evaluator_of(cases.EDGE_NAME, record=rec, **cases.EDGES[which])),
                  obs)
    same_leaves(rec, leaves, (which, L))
    same_act(got, want, rule.raw_visits, (which, L))


@pytest.mark.parametrize("name", cases.FLOOR_NAMES)
def test_cells_pruned_to_a_floor_of_two_visits_or_more_below_their_count(hip, name):
    """the large generic boards under the evaluator for which every move looks bad: the pruned counts depend on
    t = k P (n_0 - 1) exactly (tests/test_puct_forced_cpu.py plants n_0)"""
    (m, n, k), _, _, _ = BOARDS[name]
    obs, want, leaves, rule = cases.floor_reference(name)
    rec = []
    ev = spike_torch(m * n, cases.spikes_of(m, n, k), cases.FLOOR_SPIKE, 1.0, lost=True, record=rec)
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=ev, iterations=cases.FLOOR_I, c=C_PUCT, seed=SEED, leaves=cases.FLOOR_L,
                                      fpu=FPU, forced=K_FORCED)
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, 2
    got = gpu_act(pol, obs)
    same_leaves(rec, leaves, name)
    same_act(got, want, rule.raw_visits, name)


def test_a_captured_act_replayed_twice_equals_eager(hip):
    name, L = "9x9x5", 4
    (m, n, k), _, _, _ = BOARDS[name]
    C = m * n
    obs_np, want, _, rule = cases.reference(name, L, True, FPU)
    pol = policy(hip, name, L, True, FPU, evaluator_of(name))
    pol._sampler.calls = 0
    pol._sampler.step_dev = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    obs = torch.zeros((ROWS, 2, m, n), device=DEV)
    visits = torch.zeros((ROWS, C), dtype=torch.int32, device=DEV)
    raw = torch.zeros((ROWS, C), dtype=torch.int32, device=DEV)
    value = torch.zeros(ROWS, device=DEV)
    proof = torch.zeros(ROWS, dtype=torch.int8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act({"observation": obs})  # eager, on empty boards: the buffers
    torch.cuda.current_stream().wait_stream(side)
    pol._sampler.calls = 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        actions = pol.act({"observation": obs}, visits=visits, root_value=value, proof=proof, raw_visits=raw)
    obs.copy_(torch.from_numpy(obs_np))
    for replay in range(2):
        visits.fill_(-7)
        raw.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), np.zeros((ROWS, 2), np.int32),
               proof.cpu().numpy())
        same_act((got, raw.cpu().numpy()), want, rule.raw_visits, ("replay", replay))


@pytest.mark.parametrize("L,solver,fpu", [(1, False, None), (4, False, None), (4, True, None), (4, True, FPU)])
def test_without_forced_an_act_is_the_policy_as_it_was(hip, L, solver, fpu, monkeypatch):
    """the same entry points, launch for launch, and the same bits as the rule without forced playouts"""
    name = "9x9x5"
    I = BOARDS[name][1]
    obs, want, leaves, _ = cases.reference(name, L, solver, fpu, 0, None)
    called = []
    call = hip.lib.call
    monkeypatch.setattr(hip.lib, "call", lambda entry, *args: (called.append(entry), call(entry, *args))[1])
    rec = []
    pol = policy(hip, name, L, solver, fpu, evaluator_of(name, record=rec), forced=None)
    assert pol.forced is None
    got = gpu_act(pol, obs)
    same_leaves(rec, leaves, (L, solver))
    same_act(got, want, None, (L, solver))
    sfx = "_leaves" if L > 1 or solver or fpu is not None else ""
    step = "mnk_puct_step_fpu" if fpu is not None else ("mnk_puct_step_solver" if solver else "mnk_puct_step" + sfx)
    assert called == ["mnk_puct_begin" + sfx] + [step] * (I // L + 1), called
    del called[:]
    gpu_act(policy(hip, name, L, solver, fpu, evaluator_of(name)), obs)
    assert called == ["mnk_puct_begin_leaves"] + ["mnk_puct_step_forced"] * (I // L + 1), called
    with pytest.raises(ValueError, match="raw_visits"):
        pol.act({"observation": torch.from_numpy(obs).to(DEV)}, raw_visits=torch.zeros((ROWS, 81), dtype=torch.int32, device=DEV))


# ----------------------------------------------------------------------------- 3. search self-play
@pytest.mark.parametrize("name,plies", [("3x3x3", 12), ("9x9x5", 4)])
def test_search_selfplay_with_forced_equals_the_rule(hip, name, plies):
    """``SearchSelfPlay(forced=k)``: the step kernel plays from, and records, the pruned counts"""
    from search_selfplay_rule import SelfPlayRule
    from selfplay.search_selfplay import SearchSelfPlay

    (m, n, k), I, _, _ = BOARDS[name]
    C, T, temp_plies, seed = m * n, m * n, 2, 13
    sp = SearchSelfPlay(m, n, k, ROWS, evaluator=evaluator_of(name), iterations=I, c=C_PUCT, temp_plies=temp_plies, capacity=T,
                        seed=seed, device=DEV, forced=K_FORCED, fpu=FPU)
    assert sp.policy.forced == K_FORCED
    sp.play(plies)
    rule = SelfPlayRule(m, n, k, ROWS, T)
    search = cases.ForcedPuct(k, I, C_PUCT, cases.evaluator_of(name), 1, seed=seed, fpu=FPU, forced=K_FORCED)
    obs, mask = rule.view()
    pruned = 0
    for p in range(plies):
        _, visits, _, _, _ = search.act(obs, step=p)
        pruned += int((visits != search.raw_visits).any(axis=1).sum())
        obs, mask = rule.step(visits, temp_plies, seed, p)
    assert pruned and not rule.errors
    assert np.array_equal(sp.buffer.planes.cpu().numpy().view(np.uint64), rule.ring_planes)
    assert np.array_equal(sp.buffer.visits.cpu().numpy().view(np.uint16), rule.ring_visits)
    assert np.array_equal(sp.buffer.z.cpu().numpy(), rule.ring_z)
    assert np.array_equal(sp.obs.cpu().numpy(), obs) and np.array_equal(sp.mask.cpu().numpy(), mask)
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist()
