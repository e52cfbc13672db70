"""GPU: every PUCT form against its numpy rule on near-tie evaluator outputs (tests/near_tie_evaluator.py): priors within a
few ulps of 1 / C, values within a few ulps of four levels, c = 1.1, fpu = (0.3, 0.45), forced = 1.7 -- no dyadic number
anywhere, sibling scores an ulp or two apart all the way down the tree, so that a kernel that rounds one operation
otherwise than include/mnk_hip.h says searches another tree within a few iterations.  tests/test_near_tie_cpu.py shows
with the rules alone which planted rounding defects each case of tests/near_tie_cases.py notices, and that the dyadic
inputs of the older tests notice none.

Lockstep: ``PUCTSearchPolicy.act`` plain, with leaves, the solver, first-play urgency, forced playouts, all of those and root
noise at once, a kept tree over three plies one and two plies on, and a Gumbel root, on 3x3x3, 4x6x3, 9x9x5 and 19x19x5; the
bfloat16 tables on 9x9x5.  Per row: one case per ``mnk_search_selfplay_advance*`` kernel on 3x3x3 and 9x9x5, launch for
launch.  Lockstep self-play with a Gumbel root on 3x3x3.

Everything is compared bit for bit -- actions, visits, root_value as uint32, carried, proof, raw_visits, every evaluation's
leaf rows, rings and env states -- with the exceptions the older files make for numbers that come out of float64
logarithms and exponentials, whose last place the device's and numpy's libraries need not share: the noised priors of a
root and the Gumbel scores against numpy's (rtol 1e-6, the reasoning of tests/test_gpu_puct_noise.py), after which the rule
searches on the kernel's; the improved policy of a Gumbel root (rtol 1e-6, tests/test_gpu_puct_gumbel.py) and its ring
record (one count of 65 535)."""
import numpy as np
import pytest
import torch

import near_tie_cases as cases
from near_tie_cases import ASYNC_FAST, ASYNC_FULL, ASYNC_SEED, ASYNC_TEMP, ASYNC_THRESHOLD, BOARDS, C_PUCT, CONSIDERED, ENV_ID0
from near_tie_cases import FPU, K_FORCED, NOISE, SEED, STEP
from near_tie_evaluator import near_np, near_torch
from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from puct_gumbel_rule import GumbelSelfPlayRule, gumbel_puct
from puct_noise_rule import root_noise
from puct_solver_rule import PROOF_UNKNOWN
from test_gpu_puct_reuse import same, same_leaves
from test_gpu_search_selfplay_async import assert_same_state, load_start
from test_gpu_search_selfplay_async_gumbel import assert_same_state as assert_same_gumbel_state
from test_gpu_search_selfplay_async_opts import Beside

pytestmark = pytest.mark.gpu
OPTIONS = {"plain": {}, "solver": dict(solver=True), "fpu": dict(fpu=FPU), "forced": dict(forced=K_FORCED),
           "all": dict(solver=True, fpu=FPU, forced=K_FORCED, root_noise=NOISE), "reuse1": dict(reuse=True),
           "reuse2": dict(reuse=True), "gumbel": dict(gumbel=CONSIDERED), "leaves": {}}


def policy(hip, name, form, record, L=None, out_dtype=torch.float32, bf16=False, table=None):
    (m, n, k), _, I, _, _ = BOARDS[name]
    ev = near_torch(m * n, *(table or cases.choice(name, form)), out_dtype, record, DEV, bf16)
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=ev, iterations=I, c=C_PUCT, seed=SEED,
                                      leaves=L or cases.leaves_of(name, form), **OPTIONS[form])
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, 0 if pol.reuse else STEP
    return pol


def gpu_act(pol, obs_np):
    """one act as an entry of ``near_tie_cases.run``: dict(out = (actions, visits, root_value, carried, proof), raw, policy)"""
    b, _, m, n = obs_np.shape
    C = m * n
    out = dict(visits=torch.full((b, C), -7, dtype=torch.int32, device=DEV), root_value=torch.full((b,), -7.0, device=DEV))
    if pol.reuse:
        out["carried"] = torch.full((b, 2), -7, dtype=torch.int32, device=DEV)
    if pol.solver:
        out["proof"] = torch.full((b,), -7, dtype=torch.int8, device=DEV)
    if pol.forced is not None:
        out["raw_visits"] = torch.full((b, C), -7, dtype=torch.int32, device=DEV)
    if pol.gumbel is not None:
        out["policy"] = torch.full((b, C), -7.0, device=DEV)
    a = pol.act({"observation": torch.from_numpy(obs_np).to(DEV)}, **out)
    torch.cuda.synchronize()
    got = {key: t.cpu().numpy() for key, t in out.items()}
    return dict(out=(a.cpu().numpy(), got["visits"], got["root_value"], got.get("carried", np.zeros((b, 2), np.int32)),
                     got.get("proof", np.full(b, PROOF_UNKNOWN, np.int8))), raw=got.get("raw_visits"), policy=got.get("policy"))


def same_act(got, want, rec, what):
    same_leaves(rec, want["leaves"], what)
    same(got["out"], want["out"], what)
    assert np.array_equal(got["out"][4], want["out"][4]), (what, "proof", got["out"][4], want["out"][4])
    if want["raw"] is not None:
        assert np.array_equal(got["raw"], want["raw"]), (what, "raw_visits", got["raw"], want["raw"])


# ----------------------------------------------------------------------------- 1. lockstep
@pytest.mark.parametrize("form", ["plain", "leaves", "solver", "fpu", "forced"])
@pytest.mark.parametrize("name", list(BOARDS))
def test_an_act_equals_the_rule(hip, name, form):
    (want,), rec = cases.reference(name, form), []
    got = gpu_act(policy(hip, name, form, rec), want["obs"])
    same_act(got, want, rec, (name, form))


@pytest.mark.parametrize("name,table", [(name, table) for name in BOARDS for table in cases.tables_of(name, "all")])
def test_every_option_of_the_forced_step_at_once_equals_the_rule(hip, name, table):
    """four leaves, the solver, first-play urgency, forced playouts and root noise.  The noised priors are the policy's own
    buffer, held against numpy's to one part in 10^6; the search on them is the rule's, bit for bit"""
    obs, rec = cases.rows_of(name), []
    pol = policy(hip, name, "all", rec, table=table)
    got = gpu_act(pol, obs)
    noised = pol._bufs[4].cpu().numpy()
    L, C = pol.leaves, obs.shape[2] * obs.shape[3]
    free = (obs.reshape(len(obs), 2, C) == 0).all(axis=1)
    plain = near_np(C, *table)(obs, free)[0]
    wanted = root_noise(plain, free, *NOISE, SEED, STEP, ENV_ID0)
    np.testing.assert_allclose(noised[::L][free], wanted[free], rtol=1e-6, atol=0)
    (want,) = cases.run(name, "all", noise=noised, table=table)
    same_act(got, want, rec, (name, "all"))
    assert not np.array_equal(noised[::L][free], plain[free])


@pytest.mark.parametrize("distance", [1, 2])
@pytest.mark.parametrize("name", list(BOARDS))
def test_a_kept_tree_over_three_plies_equals_the_rule(hip, name, distance):
    form, rec = f"reuse{distance}", []
    acts = cases.reference(name, form)
    pol = policy(hip, name, form, rec)
    for ply, want in enumerate(acts):
        del rec[:]
        same_act(gpu_act(pol, want["obs"]), want, rec, (name, form, ply))
    assert any((want["out"][3][:, 0] > 1).any() for want in acts[1:])  # trees were carried


@pytest.mark.parametrize("name", list(BOARDS))
def test_a_gumbel_root_equals_the_rule_fed_with_the_kernels_gscore(hip, name):
    obs, rec = cases.rows_of(name), []
    pol = policy(hip, name, "gumbel", rec)
    got = gpu_act(pol, obs)
    gscore = pol._gumbel_bufs[2].cpu().numpy()
    (want,) = cases.run(name, "gumbel", gscore=gscore)
    same_act(got, want, rec, (name, "gumbel"))
    err = np.abs(got["policy"] - want["policy"])[want["policy"] > 0] / want["policy"][want["policy"] > 0]
    print(name, "policy: largest relative deviation %.3g" % err.max())
    np.testing.assert_allclose(got["policy"], want["policy"], rtol=1e-6, atol=0)
    own = cases.reference(name, "gumbel")[0]["gscore"]  # the rule's own scores are the kernel's to 1e-6
    free = np.isfinite(own)
    assert np.array_equal(np.isneginf(gscore), ~free)
    np.testing.assert_allclose(gscore[free], own[free], rtol=1e-6, atol=0)


@pytest.mark.parametrize("form,L", [("plain", 1), ("leaves", 4)])
def test_the_bfloat16_tables_on_9x9x5(hip, form, L):
    """priors and values as bfloat16 tensors: the perturbations count bfloat16 ulps, so the rule reads the same numbers"""
    name, rec = "9x9x5", []
    (want,) = cases.run(name, form, evaluator=near_np(81, *cases.choice(name, form), bf16=True), L=L)
    got = gpu_act(policy(hip, name, form, rec, L, torch.bfloat16, True), want["obs"])
    same_act(got, want, rec, (name, form, "bf16"))


# ----------------------------------------------------------------------------- 2. per row
class NearBeside(Beside):
    """``Beside`` (a player and its rule, compared after every launch) under the case's evaluator, with ``carried``
    compared as well where trees are kept"""

    def __init__(self, sp, rule, view, evaluator):
        super().__init__(sp, rule, view)
        self.ev = evaluator

    def advance(self, rounds, what=""):
        for r in range(rounds):
            super().advance(1, f"{what}launch {r}: ")
            if self.sp.keep_tree:
                assert np.array_equal(self.sp.carried.cpu().numpy(), self.rule.carried), f"{what}carried, launch {r}"


def follow_gumbel(sp, rule, ev, rounds):
    """the launches of a player with a Gumbel root beside its rule, which searches on the kernel's gscore (held against
    the rule's own to 1e-6 for the rows that backed a root up)"""
    obs, mask = rule.view()
    for r in range(rounds):
        roots = sp.fresh.cpu().numpy().astype(bool)
        sp.advance(1)
        got = sp.gscore.cpu().numpy()
        obs, mask, fresh = rule.advance(*ev(obs, mask), gscore=got)
        assert np.array_equal(sp.leaf_obs.float().cpu().numpy(), obs), f"leaves, launch {r}"
        assert np.array_equal(sp.leaf_mask.cpu().numpy(), mask), f"masks, launch {r}"
        assert sp.fresh.tolist() == fresh.tolist(), f"fresh, launch {r}"
        assert sorted(rule.gscore_wanted) == np.flatnonzero(roots).tolist(), f"rows that backed up a root, launch {r}"
        for i, want in rule.gscore_wanted.items():
            free = np.isfinite(want)
            assert np.array_equal(np.isneginf(got[i]), ~free), f"-inf cells, launch {r}, row {i}"
            np.testing.assert_allclose(got[i][free], want[free], rtol=1e-6, atol=0, err_msg=f"gscore, launch {r}, row {i}")


@pytest.mark.parametrize("name,form", cases.ASYNC)
def test_a_per_row_kernel_equals_its_rule_launch_for_launch(hip, name, form, monkeypatch):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    (m, n, k), _, _, ulps, table_seed = BOARDS[name]
    rule = cases.new_async_rule(name, form)
    sp = AsyncSearchSelfPlay(m, n, k, rule.N, evaluator=near_torch(m * n, ulps, table_seed, device=DEV),
                             iterations=ASYNC_FULL, fast_iterations=ASYNC_FAST, full_prob=0.75, c=C_PUCT, seed=ASYNC_SEED,
                             capacity=m * n, **({} if form == "gumbel" else {"temp_plies": ASYNC_TEMP}),
                             **cases.ASYNC_FORMS[form])
    sp.sampler.env_id0 = ENV_ID0
    load_start(sp, (m, n, k), None if cases.async_start(name) is None else "late")
    assert sp.full_threshold == ASYNC_THRESHOLD and rule.N % 4
    called = []
    call = hip.lib.call
    monkeypatch.setattr(hip.lib, "call", lambda entry, *args: (called.append(entry), call(entry, *args))[1])
    ev, rounds = cases.async_evaluator(name, form), cases.async_rounds(name, form)
    if form == "advance":  # (the rule without options takes no root priors)
        plain = rule.advance
        rule.advance = lambda priors, values, root_priors=None: plain(priors, values)
    if form == "gumbel":
        follow_gumbel(sp, rule, ev, rounds)
        assert_same_gumbel_state(sp, rule)
    else:
        NearBeside(sp, rule, rule.view(), ev).advance(rounds)
        assert_same_state(sp, rule)
    kernel = "mnk_search_selfplay_advance" + ("" if form == "advance" else "_" + form)
    assert {c for c in called if c.startswith("mnk_search_selfplay_advance")} == {kernel}, set(called)
    assert sp.env._err.tolist() == [0, 0] and not rule.errors
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0


# ----------------------------------------------------------------------------- 3. lockstep self-play
def test_lockstep_selfplay_with_a_gumbel_root_equals_its_rule(hip):
    """the ring holds rint(p * 65535) of a float policy: within one count, as tests/test_gpu_puct_gumbel.py holds it;
    planes, outcomes, statistics and the next roots exactly"""
    from selfplay.search_selfplay import SearchSelfPlay

    (m, n, k), _, _, ulps, table_seed = BOARDS["3x3x3"]
    C, N, I, plies, seed = m * n, 5, 8, 12, 13
    sp = SearchSelfPlay(m, n, k, N, evaluator=near_torch(C, ulps, table_seed, device=DEV), iterations=I, c=C_PUCT, capacity=C,
                        seed=seed, device=DEV, gumbel=CONSIDERED)
    sp.play(plies)
    torch.cuda.synchronize()
    rule, ev = GumbelSelfPlayRule(m, n, k, N, C), near_np(C, ulps, table_seed)
    obs, mask = rule.view()
    for p in range(plies):
        actions, _, _, target, _ = gumbel_puct(obs, k, I, C_PUCT, ev, CONSIDERED, seed=seed, step=p)
        obs, mask = rule.step_moves(target, actions, p)
    assert not rule.errors and rule.stats[0] >= 1
    assert np.array_equal(sp.buffer.planes.cpu().numpy().view(np.uint64), rule.ring_planes)
    assert np.array_equal(sp.buffer.z.cpu().numpy(), rule.ring_z)
    assert np.array_equal(sp.obs.cpu().numpy(), obs) and np.array_equal(sp.mask.cpu().numpy(), mask)
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist()
    got = sp.buffer.visits.cpu().numpy().view(np.uint16).astype(np.int64)
    assert np.abs(got - rule.ring_visits.astype(np.int64)).max() <= 1
    sp.env.check_errors()
