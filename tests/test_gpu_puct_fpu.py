"""GPU: the PUCT player with first-play urgency -- ``mnk_puct_step_fpu`` through ``PUCTSearchPolicy(fpu=...).act`` bit for
bit against the numpy rule (tests/puct_fpu_rule.py): actions, visits, root values, ``carried``, proofs and every
evaluation's leaf rows, on the single-word, two-trip, sibling, generic and multi-word boards, five rows (a partial
workgroup), one leaf and four, the solver on and off, both temperatures, ``fpu != fpu_root``; an evaluator under which
untried moves decide the search; a kept tree over three acts; root noise; bf16 priors and values; priors above 1; a captured
act; and ``fpu=None`` against the policy as it was."""
import functools

import numpy as np
import pytest
import torch

from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from puct_fpu_rule import FpuPuct
from puct_noise_rule import root_noise
from puct_solver_cases import C_PUCT, CASES, ENV_ID0, SEED, positions
from puct_solver_rule import PROOF_UNKNOWN
from test_gpu_puct_reuse import advance, exact_np, exact_torch, same, same_leaves, start

pytestmark = pytest.mark.gpu
ROWS = 5  # not a multiple of the four rows per workgroup
FPU = (0.25, 0.5)  # (fpu, fpu_root): dyadic, and not the same
#          name      I: 8 .. 24, a multiple of 4
BOARDS = {"3x3x3": 12,    # one pass per lane
          "9x9x5": 24,    # C = 81: the mass spans two passes and the lanes
          "7x9x5": 16,    # a sibling of the 9x9x5 variant
          "5x5x4": 20,    # the generic form
          "19x19x5": 8,   # the multi-word form
          "12x13x5": 32,  # <6,13,5>: 156 cells for the variant's 169
          "16x15x5": 32,  # <8,15,5>: 240 cells for 225
          "12x12x5": 8,   # generic, five words: the eight-word instantiation
          "7x9x7": 8,     # generic, three words: the four-word instantiation
          "17x17x5": 16,  # generic, ten words: the sixteen-word instantiation; the mass spans five passes
          "25x25x5": 8}   # generic, 21 words: the 32-word instantiation; ten passes
SEVEN = ("12x13x5", "16x15x5", "17x17x5", "25x25x5")  # boards that take all seven rows of ``sibling_positions``
GENERIC = {"12x12x5": (12, 12, 5), "7x9x7": (7, 9, 7)}  # boards tests/puct_solver_cases.py has no rows of: ``start`` positions
LEAVES = (1, 4)


def board_of(name):
    return GENERIC[name] if name in GENERIC else CASES[name][0]


def rows_of(name, early=False):
    """five rows of the board: those of tests/puct_solver_cases.py (late positions, wins at once, full boards; 19x19x5
    has four and takes an empty board as its fifth; the boards of SEVEN take all seven), or with ``early``, and on the
    boards of GENERIC, an empty board and four a few stones in"""
    m, n, k = board_of(name)
    if early or name in GENERIC:
        return start(m, n, k, ROWS, 7)
    if name in SEVEN:
        return positions(name)
    obs = positions(name)[:ROWS]
    return obs if len(obs) == ROWS else np.concatenate([obs, np.zeros((ROWS - len(obs), 2, m, n), np.float32)])


def losing_np(C):
    """dyadic priors that fall with the cell and the value +1/2 for every position: every move looks bad to the one who
    made it, so the score of the untried moves decides where the search goes"""
    table = (2.0 ** -(np.arange(C) % 5 + 4)).astype(np.float32)
    return lambda leaf_obs, leaf_mask: (leaf_mask * table, np.full(len(leaf_mask), 0.5, np.float32))


def losing_torch(C, record=None, scale=1.0):
    table = torch.from_numpy((2.0 ** -(np.arange(C) % 5 + 4)).astype(np.float32) * np.float32(scale)).to(DEV)

    def evaluate(leaf_obs, leaf_mask):
        if record is not None:
            record.append((leaf_obs.float().cpu().numpy(), leaf_mask.cpu().numpy()))
        return leaf_mask.float() * table, torch.full((len(leaf_mask),), 0.5, device=DEV)

    return evaluate


@functools.lru_cache(maxsize=None)
def reference(name, L, solver, temperature=0, fpu=FPU, losing=False):
    """(obs, (actions, visits, root_value, carried, proof), every evaluation's (leaf_obs, leaf_mask)) of the rule"""
    m, n, k = board_of(name)
    obs, seen = rows_of(name, losing), []
    ev = losing_np(m * n) if losing else exact_np(m * n)
    rule = FpuPuct(k, BOARDS[name], C_PUCT, ev, L, seed=SEED, env_id0=ENV_ID0, temperature=temperature, leaves=seen,
                   solver=solver, fpu=fpu)
    return obs, rule.act(obs, step=2), seen


def policy(hip, name, L, solver, evaluator, step=2, fpu=FPU, **kw):
    m, n, k = board_of(name)
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=evaluator, iterations=BOARDS[name], c=C_PUCT, seed=SEED, leaves=L,
                                      solver=solver, fpu=fpu, **kw)
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, step
    return pol


def gpu_act(pol, obs_np):
    """(actions, visits, root_value, carried, proof) of one act"""
    b, _, m, n = obs_np.shape
    visits = torch.full((b, m * n), -7, dtype=torch.int32, device=DEV)
    value = torch.full((b,), -7.0, device=DEV)
    carried = torch.full((b, 2), -7, dtype=torch.int32, device=DEV) if pol.reuse else None
    proof = torch.full((b,), -7, dtype=torch.int8, device=DEV) if pol.solver else None
    a = pol.act({"observation": torch.from_numpy(obs_np).to(DEV)}, visits=visits, root_value=value,
                **({"carried": carried} if pol.reuse else {}), **({"proof": proof} if pol.solver else {}))
    return (a.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(),
            carried.cpu().numpy() if pol.reuse else np.zeros((b, 2), np.int32),
            proof.cpu().numpy() if pol.solver else np.full(b, PROOF_UNKNOWN, np.int8))


def same_act(got, want, what):
    same(got, want, what)
    assert np.array_equal(got[4], want[4]), (what, "proof", got[4], want[4])


# ----------------------------------------------------------------------------- 1. an act
@pytest.mark.parametrize("temperature", [0, 1])
@pytest.mark.parametrize("solver", [False, True])
@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", list(BOARDS))
def test_an_act_equals_the_rule(hip, name, L, solver, temperature):
    m, n, k = board_of(name)
    obs, want, leaves = reference(name, L, solver, temperature)
    rec = []
    pol = policy(hip, name, L, solver, exact_torch(m * n, record=rec), temperature=temperature)
    assert pol.fpu == FPU
    got = gpu_act(pol, obs)
    same_leaves(rec, leaves, (name, L, solver))
    same_act(got, want, (name, L, solver, temperature))
    # and it is another search than the one without first-play urgency
    if temperature == 0 and name != "3x3x3" and not solver:
        plain = reference(name, L, solver, 0, None)[1]
        assert not np.array_equal(plain[1], want[1]), (name, L, solver)


@pytest.mark.parametrize("solver", [False, True])
@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", ["9x9x5", "19x19x5"])
def test_an_act_where_untried_moves_decide_equals_the_rule(hip, name, L, solver):
    """the value +1/2 everywhere, from an empty board and positions a few stones in: without first-play urgency a root
    visits as many children as it has iterations, once each; with it, fewer"""
    (m, n, k), _, _ = CASES[name]
    obs, want, leaves = reference(name, L, solver, 0, FPU, True)
    rec = []
    got = gpu_act(policy(hip, name, L, solver, losing_torch(m * n, rec)), obs)
    same_leaves(rec, leaves, (name, L, solver))
    same_act(got, want, (name, L, solver))
    plain = reference(name, L, solver, 0, None, True)[1]
    assert ((plain[1] > 0).sum(axis=1) == BOARDS[name]).all()
    assert ((want[1] > 0).sum(axis=1) < BOARDS[name]).all()


# ----------------------------------------------------------------------------- 2. one board each
@pytest.mark.parametrize("L", LEAVES)
def test_bfloat16_priors_and_values(hip, L):
    """(the evaluator's priors are powers of two and its values eighths: exact in bfloat16)"""
    name = "9x9x5"
    obs, want, leaves = reference(name, L, True)
    rec = []
    got = gpu_act(policy(hip, name, L, True, exact_torch(81, torch.bfloat16, rec)), obs)
    same_leaves(rec, leaves, L)
    same_act(got, want, L)


@pytest.mark.parametrize("L", LEAVES)
def test_priors_above_one_are_clipped_term_by_term(hip, L):
    """priors of 4, 2, 1, 1/2, 1/4 by cell: each term of the mass is clipped to 1 before the sum, and the mass itself
    exceeds 1 once two cells are visited"""
    name, scale = "9x9x5", 64.0
    (m, n, k), _, I = CASES[name]
    obs, seen = rows_of(name), []
    base = losing_np(m * n)
    rule = FpuPuct(k, BOARDS[name], C_PUCT, lambda o, msk: (base(o, msk)[0] * np.float32(scale), base(o, msk)[1]), L,
                   seed=SEED, env_id0=ENV_ID0, leaves=seen, fpu=FPU)
    want = rule.act(obs, step=2)
    rec = []
    got = gpu_act(policy(hip, name, L, False, losing_torch(m * n, rec, scale)), obs)
    same_leaves(rec, seen, L)
    same_act(got, want, L)
    roots = [t.prior[0][[a for a, ch in t.kids[0].items() if t.n[ch]]] for t in rule.trees]
    assert any((p > 1).any() and np.minimum(p, 1).sum() > 1 for p in roots)


@pytest.mark.parametrize("L,solver", [(1, False), (4, True)])
def test_a_kept_tree_over_three_acts_equals_the_rule(hip, L, solver):
    name = "9x9x5"
    (m, n, k), _, _ = CASES[name]
    seen, rec = [], []
    rule = FpuPuct(k, BOARDS[name], C_PUCT, exact_np(m * n), L, reuse=True, seed=SEED, env_id0=ENV_ID0, leaves=seen,
                   solver=solver, fpu=FPU)
    pol = policy(hip, name, L, solver, exact_torch(m * n, record=rec), step=0, reuse=True)
    obs, resets, kept = rows_of(name), np.zeros(ROWS, np.int64), 0
    for ply in range(3):
        del seen[:], rec[:]
        want = rule.act(obs, step=ply)
        got = gpu_act(pol, obs)
        same_leaves(rec, seen, (L, ply))
        same_act(got, want, (L, ply))
        kept += int((want[3][:, 0] > 1).sum())
        obs = advance(obs, want[0], k, 1, resets)
    assert kept  # a row carried a subtree over


def test_root_noise_equals_the_rule_on_the_kernels_priors(hip):
    """the noised priors of the roots are taken from the policy's own buffer (their comparison with numpy, to one part in
    10^6, is tests/test_gpu_puct_noise.py's); the search on them is the rule's, bit for bit"""
    name, L, noise = "9x9x5", 4, (0.3, 0.25)
    (m, n, k), _, _ = CASES[name]
    obs, rec = rows_of(name), []
    pol = policy(hip, name, L, True, exact_torch(m * n, record=rec), root_noise=noise)
    got = gpu_act(pol, obs)
    noised = pol._bufs[4].cpu().numpy()
    base, calls, seen = exact_np(m * n), [0], []

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

    rule = FpuPuct(k, BOARDS[name], C_PUCT, evaluator, L, seed=SEED, env_id0=ENV_ID0, leaves=seen, solver=True, fpu=FPU)
    want = rule.act(obs, step=2)
    same_leaves(rec, seen, "noise")
    same_act(got, want, "noise")


def test_a_captured_act_replayed_equals_eager(hip):
    name, L = "9x9x5", 4
    (m, n, k), _, _ = CASES[name]
    C = m * n
    obs_np, want, _ = reference(name, L, True)
    pol = policy(hip, name, L, True, exact_torch(C))
    pol._sampler.calls = 0
    pol._sampler.step_dev = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    obs = torch.zeros((ROWS, 2, m, n), device=DEV)
    visits = torch.zeros((ROWS, C), dtype=torch.int32, device=DEV)
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
        actions = pol.act({"observation": obs}, visits=visits, root_value=value, proof=proof)
    obs.copy_(torch.from_numpy(obs_np))
    graph.replay()
    torch.cuda.synchronize()
    got = (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), np.zeros((ROWS, 2), np.int32),
           proof.cpu().numpy())
    same_act(got, want, "replay")


@pytest.mark.parametrize("L,solver", [(1, False), (4, False), (4, True)])
def test_without_fpu_an_act_is_the_policy_as_it_was(hip, L, solver, monkeypatch):
    """the same entry points, launch for launch, and the same bits as the rule without first-play urgency"""
    name = "9x9x5"
    (m, n, k), _, I = CASES[name]
    obs, want, leaves = reference(name, L, solver, 0, None)
    called = []
    call = hip.lib.call
    monkeypatch.setattr(hip.lib, "call", lambda entry, *args: (called.append(entry), call(entry, *args))[1])
    rec = []
    pol = policy(hip, name, L, solver, exact_torch(m * n, record=rec), fpu=None)
    assert pol.fpu is None
    got = gpu_act(pol, obs)
    same_leaves(rec, leaves, (L, solver))
    same_act(got, want, (L, solver))
    sfx = "_leaves" if L > 1 or solver else ""
    step = "mnk_puct_step_solver" if solver else "mnk_puct_step" + sfx
    assert called == ["mnk_puct_begin" + sfx] + [step] * (BOARDS[name] // L + 1), called
    del called[:]
    gpu_act(policy(hip, name, L, solver, exact_torch(m * n)), obs)
    assert called == ["mnk_puct_begin_leaves"] + ["mnk_puct_step_fpu"] * (BOARDS[name] // L + 1), called


# ----------------------------------------------------------------------------- strength
FPU_MIN = 0.666 - 5 * 0.0293


def test_first_play_urgency_strengthens_the_player_at_64_iterations_on_9x9x5(hip):
    """PUCT(64, fpu=0.2) against PUCT(64), both on the heuristic evaluator of tests/test_gpu_puct.py, 256 games (half as
    black).  Measured on the MI355X: 0.6660 (169 W / 3 D / 84 L), standard error 0.0293, 5.7 standard errors above one
    half; the threshold lies 5 standard errors below the measured score.  At I = 256 the same match scored 0.4844 (118 W /
    12 D / 126 L), half a standard error below one half: nothing is claimed, or asserted, there"""
    from test_gpu_puct import heuristic_evaluator

    pol = hip.policy
    fpu = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=64, seed=14, fpu=0.2)
    plain = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=64, seed=15)
    res = hip.tournament.play_match(fpu, plain, (9, 9, 5), 256, device=DEV)
    print("PUCT(64, fpu=0.2)-PUCT(64) %.4f (%d W / %d D / %d L)" % (res["score"], res["wins"], res["draws"], res["losses"]))
    assert res["wins"] + res["losses"] + res["draws"] == 256
    assert res["score"] > FPU_MIN, res
