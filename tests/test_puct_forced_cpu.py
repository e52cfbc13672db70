"""CPU: forced playouts and policy target pruning in the PUCT player -- the C ABI of ``mnk_puct_step_forced`` and
``mnk_search_selfplay_advance_opts_forced`` (header, binding, host checks that reject before anything is enqueued), the
argument checks of ``PUCTSearchPolicy(forced=...)``, ``SearchSelfPlay`` and ``AsyncSearchSelfPlay`` before the GPU is
touched, and the numpy restatement (tests/puct_forced_rule.py) on its own: that it is ``FpuPuct`` with ``forced=None``, the
rule's walk against a bisection, and the cases of tests/test_gpu_puct_forced.py and
tests/test_gpu_search_selfplay_async_forced.py (tests/puct_forced_cases.py) under the rule alone -- each shows what it is
there for, so that no comparison on the device can pass vacuously."""
import re

import numpy as np
import pytest

import puct_forced_cases as cases
import puct_search_rule as ps
from player_cases import HEADER, check_header_and_binding, lib  # noqa: F401 (lib: the fixture)
from puct_forced_rule import floor_of, prune, root_counts, score
from puct_fpu_rule import FpuPuct

STEP, OPTS = "mnk_puct_step_forced", "mnk_search_selfplay_advance_opts_forced"
NAN, INF = float("nan"), float("inf")
LOCKSTEP = [(name,) + opt for name in cases.BOARDS for opt in cases.OPTIONS]


def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl, name
    return [" ".join(a.split()) for a in decl.group(1).split(",") if a.strip()]


# ----------------------------------------------------------------------------- the C ABI
def test_the_header_declares_the_entry_points_and_the_binding_has_them(lib):
    sig = lib.SIGNATURES
    for name in (STEP, OPTS):
        check_header_and_binding(lib, name)
    old = _params("mnk_puct_step_fpu")
    assert _params(STEP) == old[:-1] + ["int fpu_on", "float forced_k", "int32_t* raw_visits", "void* stream"]
    assert sig[STEP][:-4] == sig["mnk_puct_step_fpu"][:-1] and len(sig[STEP]) == len(sig["mnk_puct_step_fpu"]) + 3
    old = _params("mnk_search_selfplay_advance_opts_fpu")
    assert _params(OPTS) == old[:-1] + ["int fpu_on", "float forced_k", "void* stream"]
    assert sig[OPTS][:-3] == sig[OPTS[:-7] + "_fpu"][:-1] and len(sig[OPTS]) == len(sig[OPTS[:-7] + "_fpu"]) + 2
    assert lib.ABI_VERSION == 6  # additive, like every entry point since version 6
    text = open(HEADER).read()  # the rule is stated with the entry point
    for word in ("FORCED PLAYOUTS", "F_a", "n''_a", "bisects"):
        assert word in text, word


def test_the_step_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000  # a non-NULL pointer that must never be touched

    def step(ws=p, N=8, m=9, n=9, k=5, I=256, L=4, pr=p, pdt=0, va=p, vdt=0, c=1.25, last=0, temp=0, lo=p, ldt=0, lm=p,
             acts=p, proof=None, solver=0, fpu=0.25, root=0.5, fpu_on=1, forced=2.0, raw=None):
        return lib.call(STEP, ws, N, m, n, k, I, L, pr, pdt, va, vdt, c, last, temp, 1, None, 0, None, 0, 0, lo, ldt, lm,
                        acts, None, None, proof, solver, fpu, root, fpu_on, forced, raw, None)

    for bad in (dict(forced=0.0), dict(forced=-2.0), dict(forced=NAN), dict(forced=INF), dict(forced=-INF),
                dict(fpu_on=2), dict(fpu_on=-1),
                # and every check of mnk_puct_step_fpu
                dict(fpu=-0.5), dict(fpu=NAN), dict(fpu=INF), dict(root=-0.5), dict(root=NAN), dict(root=INF),
                dict(solver=2), dict(solver=-1), dict(ws=None), dict(pr=None), dict(va=None), dict(N=-1), dict(pdt=2),
                dict(vdt=-1), dict(I=0), dict(I=2052), dict(c=-0.5), dict(c=NAN), dict(temp=2), dict(last=2), dict(lo=None),
                dict(lm=None), dict(ldt=3), dict(last=1, acts=None), dict(k=10), dict(m=40, n=40), dict(L=0), dict(L=-1),
                dict(L=17), dict(L=3), dict(I=250, L=4), dict(I=8, L=16)):
        for N in (8, 0):  # (the checks come before the empty batch's early return)
            with pytest.raises(lib.MnkHipError, match=STEP):
                step(**dict(bad, N=bad.get("N", N)))
    assert step(N=0) == 0 and step(N=0, last=1, lo=None, lm=None, ldt=9, proof=p, solver=1, raw=p) == 0
    assert step(N=0, L=1) == 0 and step(N=0, I=16, L=16) == 0 and step(N=0, solver=1) == 0  # (proof may be NULL)
    assert step(N=0, forced=3.0e38) == 0 and step(N=0, forced=2.0 ** -100) == 0
    # fpu_on = 0: fpu and fpu_root are not read
    assert step(N=0, fpu_on=0, fpu=NAN, root=-1.0) == 0


def test_the_per_row_launch_rejects_bad_arguments_and_enqueues_nothing(lib):
    p = 0x1000

    def adv(ws=p, pl=p, me=p, N=8, m=9, n=9, k=5, I=8, fast=3, thr=2 ** 31, pri=p, pdt=0, val=p, vdt=0, c=1.25, temp=0,
            rows=p, T=81, rp=p, rv=p, rz=p, lo=p, ldt=0, lm=p, solver=1, alpha=0.3, eps=0.25, nfast=0, roots=None,
            fpu=0.25, root=0.5, fpu_on=1, forced=2.0):
        return lib.call(OPTS, ws, pl, me, N, m, n, k, I, fast, thr, pri, pdt, val, vdt, c, temp, 1, None, 0, rows, T, rp, rv,
                        rz, lo, ldt, lm, None, None, None, None, solver, alpha, eps, nfast, roots, fpu, root, fpu_on, forced,
                        None)

    for bad in (dict(forced=0.0), dict(forced=-1.0), dict(forced=NAN), dict(forced=INF), dict(fpu_on=2), dict(fpu_on=-1),
                dict(fpu=-0.5), dict(fpu=NAN), dict(root=INF),
                # and every check of the sibling
                dict(ws=None), dict(pl=None), dict(me=None), dict(pri=None), dict(val=None), dict(rows=None), dict(rp=None),
                dict(rv=None), dict(rz=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(T=80), dict(fast=9),
                dict(fast=0), dict(I=0, fast=0), dict(I=2052, fast=1), dict(thr=2 ** 32 + 1), dict(pdt=2), dict(vdt=-1),
                dict(ldt=3), dict(c=-1.0), dict(c=NAN), dict(temp=-1), dict(k=10), dict(m=40, n=40), dict(solver=2),
                dict(solver=-1), dict(alpha=-0.3), dict(alpha=NAN), dict(alpha=INF), dict(eps=-0.1), dict(eps=1.5),
                dict(eps=NAN), dict(nfast=2), dict(nfast=-1)):
        for N in (8, 0):
            with pytest.raises(lib.MnkHipError, match=OPTS):
                adv(**dict(bad, N=bad.get("N", N)))
    assert adv(N=0) == 0 and adv(N=0, fpu_on=0, fpu=NAN, root=-1.0) == 0 and adv(N=0, forced=3.0e38, solver=0) == 0
    assert adv(N=0, solver=0, alpha=0.0, eps=0.0) == 0 and adv(N=0, alpha=0.0, eps=1.0, nfast=1, roots=p) == 0


# ----------------------------------------------------------------------------- the classes
def test_the_classes_check_forced_before_touching_the_gpu(lib):
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from selfplay.search_selfplay import AsyncSearchSelfPlay, SearchSelfPlay

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731 (never called)
    assert PUCTSearchPolicy(5, evaluator=ev).forced is None
    assert PUCTSearchPolicy(5, evaluator=ev, forced=2).forced == 2.0
    pol = PUCTSearchPolicy(5, evaluator=ev, iterations=48, leaves=16, reuse=True, root_noise=(0.3, 0.25), solver=True,
                           fpu=(0.5, 0.125), forced=0.5)
    assert pol.forced == 0.5 and pol.fpu == (0.5, 0.125) and pol.solver and pol.evaluations_per_act == 4
    for bad in (0, 0.0, -2.0, NAN, INF, -INF, True, "2", "ab", (2.0,), [2.0, 1.0], 1e-60):
        with pytest.raises(ValueError, match="forced"):
            PUCTSearchPolicy(5, evaluator=ev, forced=bad)
        for cls in (SearchSelfPlay, AsyncSearchSelfPlay):
            with pytest.raises(ValueError, match="forced"):
                cls(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", forced=bad)
    # the refusals
    with pytest.raises(ValueError, match="forced does not combine with gumbel"):
        PUCTSearchPolicy(5, evaluator=ev, gumbel=4, forced=2.0)
    for cls in (SearchSelfPlay, AsyncSearchSelfPlay):
        with pytest.raises(ValueError, match="forced does not combine with gumbel"):
            cls(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", gumbel=4, forced=2.0)
    for kw, what in ((dict(keep_tree=True), "keep_tree"), (dict(keep_tree=True, tree_nodes=13, solver=True), "keep_tree"),
                     (dict(leaves=2), "leaves > 1"), (dict(leaves=4, solver=True, root_noise=(0.3, 0.25)), "leaves > 1")):
        with pytest.raises(ValueError, match="forced does not combine with " + what):
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", forced=2.0, **kw)
    with pytest.raises(ValueError, match="raw_visits"):  # an output of the option
        PUCTSearchPolicy(5, evaluator=ev).act({"observation": torch.zeros(1, 2, 9, 9)}, raw_visits=torch.zeros(1, 81))


# ----------------------------------------------------------------------------- the rule alone
@pytest.mark.parametrize("name,L,solver,fpu", [("3x3x3", 1, True, None), ("5x5x4", 4, False, cases.FPU),
                                               ("9x9x5", 4, True, cases.FPU)])
def test_without_forced_the_rule_is_the_rule_it_is_built_on(name, L, solver, fpu):
    (m, n, k), I, _, _ = cases.BOARDS[name]
    obs, seen_a, seen_b = cases.rows_of(name), [], []
    want = FpuPuct(k, I, cases.C_PUCT, cases.evaluator_of(name), L, seed=cases.SEED, env_id0=cases.ENV_ID0, leaves=seen_a,
                   solver=solver, fpu=fpu).act(obs, step=2)
    got = cases.new_rule(name, L, solver, fpu, forced=None, seen=seen_b).act(obs, step=2)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(seen_a, seen_b))
    # and with it the search is another one
    assert not np.array_equal(cases.reference(name, L, solver, fpu)[1][1], want[1])


def bisected(tree, a, n1, lo, sstar, c):
    """the least j in [lo, n1] with s_a(j) < s*, n1 if there is none: the kernel's search"""
    hi = n1
    while lo < hi:
        mid = (lo + hi) // 2
        if score(tree, a, mid, c) < sstar:
            hi = mid
        else:
            lo = mid + 1
    return lo


def check_pruning(tree, raw, pruned, info, c, k_forced, what):
    """condition 4: for every pruned cell s(n'') < s*, and n'' = lo or s(n'' - 1) >= s* -- the walk against a bisection;
    every other cell keeps its count"""
    cells = info.get("cells", {})
    for a in range(len(raw)):
        if a not in cells:
            assert pruned[a] == raw[a], (what, a)
            continue
        lo, n1, j = cells[a]
        assert n1 == raw[a] and lo == n1 - floor_of(tree, a, n1, k_forced) and lo <= j < n1, (what, a)
        assert a != info["cstar"] and tree.prior[0][a] > 0, (what, a)
        assert score(tree, a, j, c) < info["sstar"] and (j == lo or score(tree, a, j - 1, c) >= info["sstar"]), (what, a)
        assert j == bisected(tree, a, n1, lo, info["sstar"], c), (what, a)
        assert pruned[a] == (0 if j == 1 and n1 > 1 else j), (what, a)
        F = floor_of(tree, a, n1, k_forced)  # the least F: F - 1 fails the test, F passes it or is n'
        t = np.float32(np.float32(np.float32(k_forced) * tree.prior[0][a]) * np.float32(tree.n[0] - 1))
        assert F == 0 or np.float32(np.float32(F - 1) * np.float32(F - 1)) < t, (what, a)
        assert F == n1 or np.float32(np.float32(F) * np.float32(F)) >= t, (what, a)


@pytest.mark.parametrize("name,L,solver,fpu,temperature", LOCKSTEP)
def test_every_lockstep_case_forces_and_prunes(name, L, solver, fpu, temperature):
    """conditions 1, 2, 4 and 5 of every case"""
    obs, out, _, rule = cases.reference(name, L, solver, fpu, temperature)
    actions, visits, _, _, proof = out
    raw = rule.raw_visits
    differ = sum(1 for taken, plain in rule.picks if taken != plain)
    print(f"{name} L={L} solver={solver} fpu={fpu}: root selections with a forced cell {len(rule.picks)}, against the "
          f"plain score {differ}, rows pruned {int((raw != visits).any(axis=1).sum())}")
    assert differ > 0  # 1. a forced cell that the plain score would not have taken
    assert (raw != visits).any()  # 2.
    assert (visits <= raw).all() and (visits >= 0).all()
    for i, tree in enumerate(rule.trees):
        counts, wins_only = root_counts(tree, raw.shape[1], solver)
        assert np.array_equal(counts, raw[i])
        if wins_only:  # 5. a row with a WIN child is unpruned
            assert np.array_equal(visits[i], raw[i]) and not rule.pruned_info[i]
            continue
        check_pruning(tree, raw[i], visits[i], rule.pruned_info[i], rule.c, rule.forced, (name, i))
        if raw[i].max():
            assert visits[i].max() == raw[i].max() and visits[i][actions[i]] > 0
    if solver:
        assert any(root_counts(t, raw.shape[1], True)[1] for t in rule.trees)  # row 3: the win at the first spike cell
        assert proof[3] == 1
        # 5. no cell proven LOSS is taken for being short of its floor (from the selection's own record, made ahead of
        # the solver's filter; these cases have few such selections or none: the LOSS cases below are there for them)
        assert all(taken not in lost for lost, taken, held in rule.shunned if held)


@pytest.mark.parametrize("L,fpu", cases.LOSS_OPTIONS)
def test_the_loss_cases_hold_a_proven_loss_short_of_its_floor_and_do_not_force_it(L, fpu):
    """condition 5, the clause itself: at root selections of every row a child proven LOSS has a stored visit and
    n'^2 < k * P * S' -- FORCED but for clause (2) of the rule -- and another cell is taken.  A selection without the
    clause would give it the forced class, which orders above every move that is not proven LOSS, and take it"""
    obs, out, _, rule = cases.loss_reference(L, fpu)
    spikes = set(cases.LOSS_SPIKES[1:])
    seen = [s for s in rule.shunned if s[2]]
    print(f"L={L} fpu={fpu}: root selections with a proven LOSS short of its floor {len(seen)}, forced picks against "
          f"the plain score {sum(1 for t, p in rule.picks if t != p)}")
    assert len(seen) >= len(obs)
    assert all(set(lost) <= spikes and taken not in lost for lost, taken, _ in seen)
    for tree in rule.trees:  # every row proved both moves, with the two stored visits that fall short of the floor
        for a in spikes:
            ch = tree.kids[0][a]
            assert tree.proof[ch] == ps.LOSS and tree.n[ch] == 2
    assert (out[1][:, list(spikes)] == 0).all()  # (the solver's adjusted counts drop them)



def test_the_lockstep_cases_together_show_the_single_visit_cut_and_a_tied_maximum():
    """condition 3"""
    to_zero = tied = 0
    for name, L, solver, fpu, temperature in LOCKSTEP:
        _, _, _, rule = cases.reference(name, L, solver, fpu, temperature)
        to_zero += sum(1 for info in rule.pruned_info for lo, n1, j in info.get("cells", {}).values() if j == 1 and n1 > 1)
        tied += sum(1 for row in rule.raw_visits if row.max() > 0 and (row == row.max()).sum() > 1)
    print("cells pruned to 0 by the single-visit rule", to_zero, "rows whose maximum is tied", tied)
    assert to_zero > 0 and tied > 0


def test_the_single_visit_cut_and_the_tie_on_a_tree_by_hand():
    """root n_0 = 9, c = 1, k = 2: cells 0 and 1 tied on 3 visits (c* = 0, the lowest), cell 2 forced to 2 visits"""
    tree = ps.Tree()
    tree.n[0], tree.w[0] = 9, np.float32(0)
    tree.prior[0] = np.array([0.25, 0.25, 0.25, 0.0], np.float32)
    for a, (n, w) in enumerate([(3, 0.75), (3, 0.75), (2, -2.0), (1, 0.5)]):
        ch = tree.add(a, 0)
        tree.kids[0][a], tree.n[ch], tree.w[ch] = ch, n, np.float32(w)
    info = {}
    out = prune(tree, np.array([3, 3, 2, 1]), np.float32(1), 2.0, info)
    # s* = 1/4 + 3/4 / 4 = 7/16; cell 1: t = 4, F = 2, lo = 1, s(1) = 5/8, s(2) = 1/2, s(3) = 7/16: kept;
    # cell 2: lo = 0, s(0) = -1/4 < s*: 0; cell 3: prior 0: kept
    assert info["cstar"] == 0 and info["sstar"] == np.float32(7 / 16)
    assert out.tolist() == [3, 3, 0, 1] and info["cells"] == {2: (0, 2, 0)}
    tree.w[tree.kids[0][1]] = np.float32(0.5)  # cell 1's q = 1/6: s(1) = .5417, s(2) = .4167 < s*: n'' = 2
    assert prune(tree, np.array([3, 3, 2, 1]), np.float32(1), 2.0).tolist() == [3, 2, 0, 1]
    tree.w[tree.kids[0][1]] = np.float32(-0.75)  # q = -1/4: s(1) = 1/8 < s*: n'' = lo = 1 where n' = 3: cut to 0
    assert prune(tree, np.array([3, 3, 2, 1]), np.float32(1), 2.0).tolist() == [3, 0, 0, 1]


@pytest.mark.parametrize("L", [1, 4])
def test_the_edge_cases_have_a_prior_above_one_and_a_visited_cell_of_prior_zero(L):
    _, out, _, rule = cases.edge_reference("above", L)
    above, raw = cases.EDGES["above"]["above"], rule.raw_visits
    assert any(t.prior[0][above] == 2 and raw[i][above] > 0 for i, t in enumerate(rule.trees))
    assert (raw != out[1]).any() and any(taken != plain for taken, plain in rule.picks)
    _, out, _, rule = cases.edge_reference("zero", L)
    zero, raw = cases.EDGES["zero"]["zero"], rule.raw_visits
    kept = [i for i, t in enumerate(rule.trees) if t.prior[0][zero] == 0 and raw[i][zero] > 0 and rule.pruned_info[i]
            and rule.pruned_info[i]["cstar"] != zero]
    assert kept and all(out[1][i][zero] == raw[i][zero] for i in kept)  # a prior of 0 keeps its count


@pytest.mark.parametrize("name", cases.FLOOR_NAMES)
def test_the_floor_cases_tell_n0_less_one_from_n0(name, monkeypatch):
    """the floor's t from n_0 in the place of n_0 - 1, planted in the rule: other pruned counts on both large boards"""
    _, want, _, rule = cases.floor_reference(name)
    assert (rule.raw_visits != want[1]).any()

    def planted(tree, a, n1, k_forced):
        t = np.float32(np.float32(np.float32(k_forced) * tree.prior[0][a]) * np.float32(tree.n[0]))
        return next((F for F in range(n1) if np.float32(np.float32(F) * np.float32(F)) >= t), n1)

    monkeypatch.setattr(ps, "floor_of", planted)
    got = cases.floor_rule(name).act(cases.rows_of(name), step=2)
    rows = int((got[1] != want[1]).any(axis=1).sum())
    print(name, "rows whose pruned counts differ", rows)
    assert rows > 0


@pytest.mark.parametrize("L,solver", cases.REUSE)
def test_the_kept_tree_case_carries_a_root_whose_visits_exceed_its_childrens(L, solver):
    acts = cases.reuse_reference(L, solver)
    carried = exceeds = pruned = 0
    for _, out, _, raw, n0 in acts:
        carried += int((out[3][:, 0] > 1).sum())
        exceeds += sum(1 for i in range(len(raw)) if out[3][i, 0] > 1 and n0[i] - 1 > raw[i].sum())
        pruned += int((raw != out[1]).any(axis=1).sum())
    print(f"L={L} solver={solver}: rows that carried a subtree {carried}, whose n_0 - 1 exceeds their children's sum "
          f"{exceeds}, rows pruned {pruned}")
    assert carried and exceeds and pruned


# ----------------------------------------------------------------------------- the per-row cases
@pytest.mark.parametrize("case", range(len(cases.ASYNC_CASES)))
def test_every_per_row_case_uses_every_option_it_turns_on(case):
    """condition 6"""
    rule, off = cases.async_run(case), cases.async_run(case, None)
    board, _, _, _, _, noise, on_fast, solver, fpu = cases.ASYNC_CASES[case]
    full_pruned = sum(1 for _, _, full, forces, _, raw, counts, _ in rule.plies if full and forces and (raw != counts).any())
    differ = sum(1 for taken, plain in rule.picks if taken != plain)
    assert all(forces == (full or on_fast) for _, _, full, forces, *_ in rule.plies)
    # a ply that does not force: its search, record and move are those of the run with forced off from the same position
    plain = {(i, p): (root, raw, counts, move) for i, p, full, forces, root, raw, counts, move in off.plies}
    same = 0
    for i, p, full, forces, root, raw, counts, move in rule.plies:
        if not forces and (i, p) in plain and np.array_equal(plain[i, p][0], root):
            assert np.array_equal(raw, counts)
            assert np.array_equal(plain[i, p][1], raw) and np.array_equal(plain[i, p][2], counts) and plain[i, p][3] == move
            same += 1
    print(f"{board}: games {rule.stats[0]}, fast / full records {rule.fast_records} / {rule.full_records}, row plies "
          f"{rule.row_plies.tolist()}, forced picks against the plain score {differ}, full plies with pruned counts "
          f"{full_pruned}, plies without forcing equal to the run without the option {same}, noised / plain roots "
          f"{rule.noised_roots} / {rule.plain_roots}")
    cases.assert_every_option_was_used(case, rule)
    assert differ > 0 and full_pruned > 0
    assert same > 0 or on_fast  # (with noise_on_fast every ply forces)
    assert not np.array_equal(rule.ring_visits, off.ring_visits)


def test_the_per_row_cases_cover_the_options():
    opts = [(c[5] is not None, c[6], c[7], c[8] is not None) for c in cases.ASYNC_CASES]
    for j in range(4):
        assert any(o[j] for o in opts) and any(not o[j] for o in opts), j
