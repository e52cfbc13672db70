"""CPU: first-play urgency in the PUCT player -- the C ABI of ``mnk_puct_step_fpu``, ``mnk_search_selfplay_advance_opts_fpu``
and ``mnk_search_selfplay_advance_keep_fpu`` (header, binding, host checks that reject before anything is enqueued), the
argument checks of ``PUCTSearchPolicy(fpu=...)``, ``SearchSelfPlay`` and ``AsyncSearchSelfPlay`` before the GPU is touched,
and the numpy restatement (tests/puct_fpu_rule.py) on its own: that it is ``SolverPuct`` with ``fpu=None``, what the rule
is for, that ``fpu=0`` is not ``fpu=None``, and the clamp at -1; and the cases of
tests/test_gpu_search_selfplay_async_fpu.py (tests/search_selfplay_async_fpu_cases.py) under the rule alone: each shows what
it is there for."""
import re

import numpy as np
import pytest

import search_selfplay_async_fpu_cases as async_cases
from oracle.packing import record_words
from player_cases import HEADER, check_header_and_binding, lib  # noqa: F401 (lib: the fixture)
from puct_fpu_rule import FpuPuct, as_pair, mass_of, untried_q
from puct_rule import _Tree
from puct_solver_cases import C_PUCT, CASES, ENV_ID0, SEED, positions, reference

STEP, OPTS, KEEP = "mnk_puct_step_fpu", "mnk_search_selfplay_advance_opts_fpu", "mnk_search_selfplay_advance_keep_fpu"
NAN, INF = float("nan"), float("inf")


def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl, name
    return [" ".join(a.split()) for a in decl.group(1).split(",") if a.strip()]


# ----------------------------------------------------------------------------- the C ABI
def test_the_header_declares_the_entry_points_and_the_binding_has_them(lib):
    sig = lib.SIGNATURES
    for name in (STEP, OPTS, KEEP):
        check_header_and_binding(lib, name)
    old = _params("mnk_puct_step_solver")
    assert _params(STEP) == old[:-1] + ["int solver", "float fpu", "float fpu_root", "void* stream"]
    assert sig[STEP][:-4] == sig["mnk_puct_step_solver"][:-1] and len(sig[STEP]) == len(sig["mnk_puct_step_solver"]) + 3
    for name in (OPTS, KEEP):
        old = _params(name[:-4])
        assert _params(name) == old[:-1] + ["float fpu", "float fpu_root", "void* stream"]
        assert sig[name][:-3] == sig[name[:-4]][:-1] and len(sig[name]) == len(sig[name[:-4]]) + 2
    assert lib.ABI_VERSION == 6  # additive, like every entry point since version 6


def test_the_step_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000  # a non-NULL pointer that must never be touched

    def step(ws=p, N=8, m=9, n=9, k=5, I=256, L=4, pr=p, pdt=0, va=p, vdt=0, c=1.25, last=0, temp=0, lo=p, ldt=0, lm=p,
             acts=p, proof=None, solver=0, fpu=0.25, root=0.5):
        return lib.call(STEP, ws, N, m, n, k, I, L, pr, pdt, va, vdt, c, last, temp, 1, None, 0, None, 0, 0, lo, ldt, lm,
                        acts, None, None, proof, solver, fpu, root, None)

    for bad in (dict(fpu=-0.5), dict(fpu=NAN), dict(fpu=INF), dict(fpu=-INF), dict(root=-0.5), dict(root=NAN),
                dict(root=INF), dict(root=-INF), dict(solver=2), dict(solver=-1),
                # and every check of mnk_puct_step_solver
                dict(ws=None), dict(pr=None), dict(va=None), dict(N=-1), dict(pdt=2), dict(vdt=-1), dict(I=0),
                dict(I=2052), dict(c=-0.5), dict(c=NAN), dict(temp=2), dict(last=2), dict(lo=None), dict(lm=None),
                dict(ldt=3), dict(last=1, acts=None), dict(k=10), dict(m=40, n=40), dict(L=0), dict(L=-1), dict(L=17),
                dict(L=3), dict(I=250, L=4), dict(I=8, L=16)):
        for N in (8, 0):  # (the checks come before the empty batch's early return)
            with pytest.raises(lib.MnkHipError, match=STEP):
                step(**dict(bad, N=bad.get("N", N)))
    assert step(N=0) == 0 and step(N=0, last=1, lo=None, lm=None, ldt=9, proof=p, solver=1) == 0
    assert step(N=0, L=1) == 0 and step(N=0, I=16, L=16) == 0 and step(N=0, solver=1) == 0  # (proof may be NULL)
    assert step(N=0, fpu=0.0, root=0.0) == 0 and step(N=0, fpu=3.0e38, root=3.0e38) == 0


@pytest.mark.parametrize("name", [OPTS, KEEP])
def test_the_per_row_launches_reject_bad_arguments_and_enqueue_nothing(lib, name):
    p = 0x1000
    keep = name == KEEP

    def adv(ws=p, pl=p, me=p, N=8, m=9, n=9, k=5, I=8, fast=3, thr=2 ** 31, pri=p, pdt=0, val=p, vdt=0, c=1.25, temp=0,
            rows=p, T=81, rp=p, rv=p, rz=p, lo=p, ldt=0, lm=p, solver=1, alpha=0.3, eps=0.25, nfast=0, roots=None, TI=16,
            kn=9, carried=p, fpu=0.25, root=0.5):
        tail = (TI, kn, carried) if keep else ()
        return lib.call(name, ws, pl, me, N, m, n, k, I, fast, thr, pri, pdt, val, vdt, c, temp, 1, None, 0, rows, T, rp, rv,
                        rz, lo, ldt, lm, None, None, None, None, solver, alpha, eps, nfast, roots, *tail, fpu, root, None)

    cases = [dict(fpu=-0.5), dict(fpu=NAN), dict(fpu=INF), dict(fpu=-INF), dict(root=-1e-3), dict(root=NAN), dict(root=INF),
             # and every check of the sibling
             dict(ws=None), dict(pl=None), dict(me=None), dict(pri=None), dict(val=None), dict(rows=None), dict(rp=None),
             dict(rv=None), dict(rz=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(T=80), dict(fast=9), dict(fast=0),
             dict(I=0, fast=0), dict(I=2052, fast=1), dict(thr=2 ** 32 + 1), dict(pdt=2), dict(vdt=-1), dict(ldt=3),
             dict(c=-1.0), dict(c=NAN), dict(temp=-1), dict(k=10), dict(m=40, n=40), dict(solver=2), dict(solver=-1),
             dict(alpha=-0.3), dict(alpha=NAN), dict(alpha=INF), dict(eps=-0.1), dict(eps=1.5), dict(eps=NAN),
             dict(nfast=2), dict(nfast=-1)]
    if keep:
        cases += [dict(carried=None), dict(TI=7), dict(TI=2049), dict(kn=0), dict(kn=10), dict(TI=8, kn=2)]
    for bad in cases:
        for N in (8, 0):
            with pytest.raises(lib.MnkHipError, match=name):
                adv(**dict(bad, N=bad.get("N", N)))
    assert adv(N=0) == 0 and adv(N=0, fpu=0.0, root=0.0) == 0 and adv(N=0, fpu=3.0e38, root=3.0e38, solver=0) == 0
    assert adv(N=0, solver=0, alpha=0.0, eps=0.0) == 0 and adv(N=0, alpha=0.0, eps=1.0, nfast=1, roots=p) == 0


# ----------------------------------------------------------------------------- the classes
def test_the_classes_check_fpu_before_touching_the_gpu(lib):
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from selfplay.search_selfplay import AsyncSearchSelfPlay, SearchSelfPlay

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731 (never called)
    assert PUCTSearchPolicy(5, evaluator=ev).fpu is None
    assert PUCTSearchPolicy(5, evaluator=ev, fpu=0.25).fpu == (0.25, 0.25)
    assert PUCTSearchPolicy(5, evaluator=ev, fpu=0).fpu == (0.0, 0.0)
    pol = PUCTSearchPolicy(5, evaluator=ev, iterations=48, leaves=16, reuse=True, root_noise=(0.3, 0.25), solver=True,
                           fpu=(0.5, 0.125))
    assert pol.fpu == (0.5, 0.125) and pol.solver and pol.evaluations_per_act == 4
    for bad in (-0.25, NAN, INF, (0.25, -1.0), (NAN, 0.0), (0.0, INF), (0.1, 0.2, 0.3), (0.1,), "0.2", "ab", True, [None, 1]):
        with pytest.raises(ValueError, match="fpu"):
            PUCTSearchPolicy(5, evaluator=ev, fpu=bad)
        for cls in (SearchSelfPlay, AsyncSearchSelfPlay):
            with pytest.raises(ValueError, match="fpu"):
                cls(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", fpu=bad)
    # the refusals
    with pytest.raises(ValueError, match="fpu does not combine with gumbel yet"):
        PUCTSearchPolicy(5, evaluator=ev, gumbel=4, fpu=0.25)
    for cls in (SearchSelfPlay, AsyncSearchSelfPlay):
        with pytest.raises(ValueError, match="fpu does not combine with gumbel yet"):
            cls(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", gumbel=4, fpu=0.25)
    for kw in (dict(leaves=2), dict(leaves=4, solver=True), dict(leaves=8, root_noise=(0.3, 0.25))):
        with pytest.raises(ValueError, match="fpu does not combine with leaves > 1"):
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", fpu=(0.25, 0.5), **kw)


# ----------------------------------------------------------------------------- the rule alone
@pytest.mark.parametrize("name,L,solver", [("3x3x3", 1, True), ("5x5x4", 4, False), ("9x9x5", 4, True)])
def test_without_fpu_the_rule_is_the_rule_it_is_built_on(name, L, solver):
    from puct_solver_rule import SolverPuct
    from puct_reuse_cases import exact_np

    (m, n, k), _, I = CASES[name]
    obs, seen_a, seen_b = positions(name), [], []
    want = SolverPuct(k, I, C_PUCT, exact_np(m * n), L, seed=SEED, env_id0=ENV_ID0, leaves=seen_a, solver=solver).act(obs, step=2)
    got = FpuPuct(k, I, C_PUCT, exact_np(m * n), L, seed=SEED, env_id0=ENV_ID0, leaves=seen_b, solver=solver).act(obs, step=2)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(seen_a, seen_b))
    if solver:
        assert all(np.array_equal(g, w) for g, w in zip(got, reference(name, L)[1]))


def losing_evaluator(C):
    """uniform priors 1/128 on the legal cells and value +1/2 for every position: every move looks bad to the one who
    made it"""

    def evaluate(leaf_obs, leaf_mask):
        return leaf_mask * np.float32(1 / 128), np.full(len(leaf_mask), 0.5, np.float32)

    return evaluate


def root_children(fpu, I=64):
    rule = FpuPuct(5, I, C_PUCT, losing_evaluator(81), 1, seed=SEED, fpu=fpu)
    _, visits, root_value, _, _ = rule.act(np.zeros((1, 2, 9, 9), np.float32), step=0)
    assert visits.sum() == I
    return int((visits[0] > 0).sum()), float(root_value[0])


def test_what_the_rule_is_for():
    """9x9x5, the empty board, I = 64, uniform priors 1/128, value +1/2 everywhere: every visited child has q = -1/2, so
    without fpu every untried move (q = 0) outranks them all and the root visits 64 different children once each.  With
    fpu = 0.25 an untried root move is valued near the root's own value, below the visited ones' score plus their
    exploration term only after several visits.
    Distinct root children visited: fpu=None 64, fpu=0.25 15."""
    plain, value = root_children(None)
    with_fpu, _ = root_children(0.25)
    print("distinct root children visited: fpu=None", plain, "fpu=0.25", with_fpu)
    assert plain == 64 and value < 0  # one visit on each of 64 children, at a root that looks lost for its side to move
    assert with_fpu < plain


def test_fpu_zero_is_not_fpu_none():
    """an untried move gets q_v, not 0"""
    tree = _Tree()
    tree.n[0], tree.w[0] = 4, np.float32(-1.5)  # the root's mean value for its side to move: +3/8
    assert untried_q(tree, 0, np.array([0.5, 0.25], np.float32), as_pair(0)) == np.float32(0.375)
    (m, n, k), _, I = CASES["9x9x5"]
    from puct_reuse_cases import exact_np

    obs = positions("9x9x5")[:5]
    a = FpuPuct(k, I, C_PUCT, exact_np(m * n), 1, seed=SEED, fpu=0).act(obs, step=2)
    b = FpuPuct(k, I, C_PUCT, exact_np(m * n), 1, seed=SEED, fpu=None).act(obs, step=2)
    assert not np.array_equal(a[1], b[1])


def test_the_mass_and_the_clamp():
    """the mass clips every term to [0, 1] and sums integers; a reduction large enough gives exactly -1"""
    assert mass_of(np.array([0.25], np.float32)) == np.float32(0.5)
    assert mass_of(np.array([0.25, 0.5, 0.25], np.float32)) == np.float32(1.0)
    assert mass_of(np.array([3.0, -2.0, 1.0, 2.0], np.float32)) == np.float32(np.sqrt(3.0))  # 1 + 0 + 1 + 1
    assert mass_of(np.array([], np.float32)) == 0.0
    tiny = np.float32(2.0 ** -40)  # below the fixed point's resolution: truncated to nothing
    assert mass_of(np.array([tiny] * 100, np.float32)) == 0.0
    # the order of the terms cannot matter
    p = np.random.default_rng(3).random(361).astype(np.float32) / 64
    assert len({float(mass_of(np.random.default_rng(s).permutation(p))) for s in range(8)}) == 1
    tree = _Tree()
    tree.n[0], tree.w[0] = 2, np.float32(1.0)  # q_v = -1/2
    seen = np.array([0.25], np.float32)  # mass 1/2
    assert untried_q(tree, 0, seen, as_pair((9.0, 0.5))) == np.float32(-0.75)  # the root takes fpu_root
    assert untried_q(tree, 0, seen, as_pair((0.5, 1.0))) == np.float32(-1.0)  # exactly at the bound
    assert untried_q(tree, 0, seen, as_pair((0.0, 64.0))) == np.float32(-1.0)  # clamped
    assert untried_q(tree, 0, seen, as_pair(3.0e38)) == np.float32(-1.0)
    assert untried_q(tree, 0, np.array([], np.float32), as_pair(3.0e38)) == np.float32(-0.5)  # nothing visited: no reduction


# ----------------------------------------------------------------------------- the cases of the per-row GPU tests
# (the rule gives, per case: games, fast / full records, row plies, plies ended by proof, carried plies that kept more
# than one node, noised roots -- printed below)
@pytest.mark.parametrize("case", range(len(async_cases.CASES)))
def test_every_per_row_case_uses_every_option_it_turns_on(case):
    rule = async_cases.mixed_run(case)
    by_proof, kept_many, noised = async_cases.conditions(rule)
    print(f"{async_cases.CASES[case][0]}: games {rule.stats[0]}, fast / full records {rule.fast_records} / "
          f"{rule.full_records}, row plies {rule.row_plies.tolist()}, by proof {by_proof}, kept more than one node "
          f"{kept_many}, noised / plain roots {rule.noised_roots} / {rule.plain_roots}")
    async_cases.assert_every_option_was_used(case, rule)


def test_both_per_row_entry_points_run_on_every_kind_of_board():
    """(words per plane, n, k) of the built-in rows a case runs in, (words, 0, 0) for a generic form: with ``keep_tree``
    the entry point is ``mnk_search_selfplay_advance_keep_fpu``, without it ``..._opts_fpu``"""
    builtin = {(1, 3, 3), (3, 9, 5), (6, 13, 5), (8, 15, 5), (12, 19, 5)}  # (MNK_BUILTIN_BOARDS of csrc/mnk_emit.h)

    def kind(board):
        m, n, k = board
        row = (record_words(m, n), n, k)
        return row if row in builtin else (row[0], 0, 0)

    for keep in (False, True):
        kinds = {kind(c[0]) for c in async_cases.CASES if c[7] == keep}
        assert kinds == builtin | {(5, 0, 0), (2, 0, 0), (10, 0, 0), (21, 0, 0)}, (keep, kinds)
    # the solver, the noise and a tree cut to keep_nodes each run on a multi-word built-in and on a generic form
    for option in (5, 6):
        kinds = {kind(c[0]) for c in async_cases.CASES if c[option]}
        assert any(w > 3 and n for w, n, _ in kinds) and any(w > 1 and not n for w, n, _ in kinds), option
