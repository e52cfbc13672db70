"""CPU: the PUCT player with several leaves per row and evaluation -- the numpy restatement (tests/puct_leaves_rule.py) at
one leaf against tests/puct_rule.py; the C ABI of the four ``mnk_puct_*_leaves`` entry points (header, binding, host
checks that reject before anything is enqueued, the workspace of one leaf); the constructors' checks; and, from the rule's
trace alone, that the inputs of the GPU test reach void slots, repeated terminal leaves and shared prefixes."""
import re

import numpy as np
import pytest

from player_cases import HEADER, check_header_and_binding, header_constants, lib, positions  # noqa: F401 (lib: the fixture)
from puct_leaves_cases import CASES, PARAMS, reference
from puct_leaves_rule import LeavesPuct, puct_leaves
from puct_reuse_cases import exact_np
from puct_rule import puct


# ----------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("board,I", [((3, 3, 3), 20), ((4, 6, 3), 24), ((9, 9, 5), 12)])
@pytest.mark.parametrize("temperature", [0, 1])
def test_one_leaf_is_the_rule_of_one_leaf(board, I, temperature):
    m, n, k = board
    obs = positions(m, n, k, 10, seed=m + n, max_fill=0.7)
    a, b = [], []
    want = puct(obs, k, I, 1.25, exact_np(m * n), seed=5, step=3, env_id0=2, temperature=temperature, leaves=a)
    got = puct_leaves(obs, k, I, 1.25, exact_np(m * n), 1, seed=5, step=3, env_id0=2, temperature=temperature, leaves=b)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert len(a) == len(b) == I + 1
    for (lo, lm), (wo, wm) in zip(b, a):
        assert np.array_equal(lo, wo) and np.array_equal(lm, wm)


def test_visits_sum_to_the_budget_less_the_void_slots():
    obs = reference("3x3x3", 8)[0]
    for L in (2, 8, 16):
        _, (_, visits, _), seen, trace = reference("3x3x3", L)
        assert len(seen) == 32 // L + 1 and seen[0][0].shape == (len(obs) * L, 2, 3, 3)
        for i, tr in enumerate(trace):
            assert visits[i].sum() == 32 - tr["void"], (L, i)
        # evaluation 0: the root in slot 0, void slots (the root again) behind it
        assert np.array_equal(seen[0][0].reshape(len(obs), L, 2, 3, 3), np.repeat(obs[:, None], L, axis=1))


def test_a_kept_tree_carries_its_visits():
    m, n, k = 4, 6, 3
    obs = np.zeros((2, 2, m, n), np.float32)
    rule = LeavesPuct(k, 16, 1.25, exact_np(m * n), 4, reuse=True)
    _, v0, _, c0 = rule.act(obs)
    _, v1, _, c1 = rule.act(obs, step=1)
    assert not c0.any() and (c1[:, 1] == 1 + v0.sum(axis=1)).all()  # the whole tree: the root's n
    for i, tr in enumerate(rule.trace):
        assert v1[i].sum() == v0[i].sum() + 16 - tr["void"]


# ----------------------------------------------------------------------------- the GPU test's inputs
def test_the_gpu_cases_reach_every_path():
    """summed over the cases of tests/test_gpu_puct_leaves.py, on rows with a legal cell"""
    tot, clean = dict(void=0, shared=0, repeat=0), []
    for name, L in PARAMS:
        if name == "long":  # (seconds of numpy: the GPU test pays them once; nothing here depends on it)
            continue
        trace = reference(name, L)[3]
        case = {key: sum(t[key] for t in trace if t["live"]) for key in tot}
        for key in tot:
            tot[key] += case[key]
        if not any(case.values()):
            clean.append((name, L))
    print(tot, clean)
    assert tot["void"] >= 20 and tot["repeat"] >= 20 and tot["shared"] >= 50, tot
    assert [c for c in clean if c[1] > 1], clean  # a case of several leaves with none of them: the clean path
    # the full boards of the 4x6x3 and 9x9x5 cases: void slots only
    for name in ("4x6x3", "9x9x5"):
        I = CASES[name][2]
        assert not reference(name, 4)[3][1]["live"] and reference(name, 4)[3][1]["void"] == I


# ----------------------------------------------------------------------------- the C ABI
NAMES = ("mnk_puct_workspace_bytes_leaves", "mnk_puct_begin_leaves", "mnk_puct_rebase_leaves", "mnk_puct_step_leaves")


def test_header_declares_the_entry_points_and_the_binding_matches(lib):
    for name in NAMES[1:]:
        check_header_and_binding(lib, name)
    # (the helper looks for an `int` result; the size is an int64_t)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint64_t\s+" + NAMES[0] + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == len(lib.SIGNATURES[NAMES[0]]) == 5
    assert hasattr(lib.load(), NAMES[0])
    assert header_constants()["MNK_PUCT_LEAVES_MAX"] == "16" == str(lib.PUCT_LEAVES_MAX)
    assert lib.load().mnk_abi_version() == 6


def test_the_workspace_of_one_leaf_is_the_workspace(lib):
    for N, m, n, I in ((1, 3, 3, 1), (7, 9, 9, 256), (1024, 9, 9, 256), (3, 19, 19, 2048), (5, 4, 6, 48), (0, 9, 9, 8)):
        assert lib.puct_workspace_bytes(N, m, n, I, 1) == lib.puct_workspace_bytes(N, m, n, I)
    one = lib.puct_workspace_bytes(1, 9, 9, 256)
    for L in (2, 4, 8, 16):
        more = lib.puct_workspace_bytes(1, 9, 9, 256, L)
        # L - 1 paths of u16[I + 2], leaf planes and {depth, state} behind the tree, each part 16-byte aligned
        assert more % 256 == 0 and one <= more <= one + (L - 1) * (2 * 258 + 16 + 8 * 32 + 8) + 256 + 48
        assert lib.puct_workspace_bytes(3, 9, 9, 256, L) == 3 * more
    for bad in ((4, 9, 9, 256, 0), (4, 9, 9, 256, 17), (4, 9, 9, 256, -1), (4, 9, 9, 48, 5), (4, 9, 9, 0, 1),
                (4, 9, 9, 2049, 1), (-1, 9, 9, 16, 4), (4, 40, 40, 16, 4)):
        with pytest.raises(lib.MnkHipError):
            lib.puct_workspace_bytes(*bad)


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000  # a non-NULL pointer that must never be touched

    def begin(obs=p, dtype=0, N=8, m=9, n=9, k=5, I=256, L=4, ws=p, lo=p, ldt=0, lm=p):
        return lib.call("mnk_puct_begin_leaves", obs, dtype, N, m, n, k, I, L, ws, lo, ldt, lm, None)

    def rebase(obs=p, dtype=0, N=8, m=9, n=9, k=5, I=512, keep=257, L=4, ws=p, lo=p, ldt=0, lm=p):
        return lib.call("mnk_puct_rebase_leaves", obs, dtype, N, m, n, k, I, keep, L, ws, lo, ldt, lm, None, None)

    def step(ws=p, N=8, m=9, n=9, k=5, I=256, L=4, pr=p, pdt=0, va=p, vdt=0, c=1.25, last=0, temp=0, lo=p, ldt=0, lm=p,
             acts=p):
        return lib.call("mnk_puct_step_leaves", ws, N, m, n, k, I, L, pr, pdt, va, vdt, c, last, temp, 1, None, 0, None, 0,
                        0, lo, ldt, lm, acts, None, None, None)

    leaves = (dict(L=0), dict(L=-1), dict(L=17), dict(L=3), dict(I=250, L=4), dict(I=8, L=16))
    for bad in (dict(obs=None), dict(ws=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(dtype=3), dict(ldt=-1),
                dict(I=0), dict(I=2052), dict(k=10), dict(m=40, n=40)) + leaves:
        with pytest.raises(lib.MnkHipError, match="mnk_puct_begin_leaves"):
            begin(**bad)
    for bad in (dict(obs=None), dict(ws=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(dtype=3), dict(ldt=-1),
                dict(I=0), dict(I=2052), dict(k=10), dict(keep=0), dict(keep=510), dict(keep=506, L=8),
                dict(I=16, keep=2, L=16)) + leaves[:4]:
        with pytest.raises(lib.MnkHipError, match="mnk_puct_rebase_leaves"):
            rebase(**bad)
    for bad in (dict(ws=None), dict(pr=None), dict(va=None), dict(N=-1), dict(pdt=2), dict(vdt=-1), dict(I=0),
                dict(I=2052), dict(c=-0.5), dict(c=float("nan")), dict(temp=2), dict(last=2), dict(lo=None), dict(lm=None),
                dict(ldt=3), dict(last=1, acts=None)) + leaves:
        with pytest.raises(lib.MnkHipError, match="mnk_puct_step_leaves"):
            step(**bad)
    assert begin(N=0) == 0 and rebase(N=0) == 0 and step(N=0) == 0 and step(N=0, last=1, lo=None, lm=None, ldt=9) == 0
    assert begin(N=0, I=2048, L=16) == 0 and rebase(N=0, keep=509) == 0 and rebase(N=0, I=16, keep=1, L=16) == 0
    assert step(N=0, L=1) == 0 and step(N=0, I=16, L=16) == 0


def test_the_constructors_refuse_bad_leaves(lib):
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from selfplay.search_selfplay import SearchSelfPlay

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731
    pol = PUCTSearchPolicy(5, evaluator=ev)
    assert pol.leaves == 1 and pol.evaluations_per_act == 257
    pol = PUCTSearchPolicy(5, evaluator=ev, iterations=48, leaves=16)
    assert pol.leaves == 16 and pol.evaluations_per_act == 4
    assert PUCTSearchPolicy(5, evaluator=ev, iterations=16, leaves=16, reuse=True).tree_nodes == 33
    for bad in (dict(leaves=0), dict(leaves=-2), dict(leaves=17), dict(leaves=2.5), dict(iterations=50, leaves=4),
                dict(iterations=8, leaves=16), dict(iterations=16, leaves=4, reuse=True, tree_nodes=19)):
        with pytest.raises(ValueError):
            PUCTSearchPolicy(5, evaluator=ev, **bad)
        with pytest.raises(ValueError):
            SearchSelfPlay(9, 9, 5, 4, evaluator=ev, device="cpu", **{"iterations": 64, **bad})
