"""CPU: the PUCT player that keeps its tree -- the numpy restatement of the rule in tests/puct_reuse_rule.py: it is
``puct_rule.puct`` wherever nothing continues, a played-out game carries the chosen child's visits from ply to ply, a
truncated tree stays well formed, positions that are not 0 / 1 / 2 plies on start fresh; the C ABI of ``mnk_puct_rebase``
(header, binding, host argument checks) and the new arguments of ``PUCTSearchPolicy`` / ``SearchSelfPlay``."""
import numpy as np
import pytest

from player_cases import board, check_header_and_binding, lib, positions  # noqa: F401 (lib: the fixture)
from playout_rule import has_run
from puct_reuse_rule import ReusePuct, match
from puct_rule import puct


def table_evaluator(C):
    """a deterministic function of the leaf: priors that are powers of two, peaked on a few cells, and a value k / 8 from
    a weighted stone difference -- trees narrow enough for a child to own a subtree worth carrying"""
    a = np.arange(C)
    table = (2.0 ** -(((a * 37) % 16) // 2 + 1 + max(int(np.ceil(np.log2(C))) - 3, 0))).astype(np.float32)
    weights = (a % 7 + 1).astype(np.float32)

    def evaluate(leaf_obs, leaf_mask):
        o = leaf_obs.reshape(len(leaf_obs), 2, -1)
        s = ((o[:, 0] - o[:, 1]) * weights).sum(axis=1)
        return leaf_mask * table, ((np.mod(s, 9) - 4) / 8).astype(np.float32)

    return evaluate


def play(obs, actions, k):
    """every row's action played, seen by the next side to move; (next obs, the rows whose game ended)"""
    N, _, m, n = obs.shape
    nxt = np.zeros_like(obs)
    ended = np.zeros(N, bool)
    for i in range(N):
        me = obs[i, 0].reshape(-1).copy()
        assert not me[actions[i]] and not obs[i, 1].reshape(-1)[actions[i]]
        me[actions[i]] = 1
        nxt[i, 0], nxt[i, 1] = obs[i, 1], me.reshape(m, n)
        ended[i] = bool(has_run(me.reshape(1, m, n) != 0, k)[0]) or bool((nxt[i, 0] + nxt[i, 1]).all())
    return nxt, ended


# ----------------------------------------------------------------------------- the rule
def test_positions_that_never_continue_each_other_search_as_puct_does():
    m, n, k, I = 4, 5, 3, 12
    ev = table_evaluator(m * n)
    la, lb = [], []
    rule = ReusePuct(k, I, 1.25, ev, seed=5, env_id0=2, leaves=la)
    last = None
    for call in range(4):
        obs = positions(m, n, k, 7, 100 + call)[1:]  # (without the empty board, which would continue itself)
        if last is not None:  # no accident: no row is one or two plies on from the last call's (row 0, the full board,
            # is the same position again: a tree without a legal cell is not continued)
            assert all(match(r, o) is None for r, o in zip(last.reshape(6, 2, -1)[1:] != 0, obs.reshape(6, 2, -1)[1:] != 0))
            assert match(last.reshape(6, 2, -1)[0] != 0, obs.reshape(6, 2, -1)[0] != 0) == []
        last = obs
        a, v, rv, carried = rule.act(obs, step=call)
        wa, wv, wrv = puct(obs, k, I, 1.25, ev, seed=5, step=call, env_id0=2, leaves=lb)
        assert np.array_equal(a, wa) and np.array_equal(v, wv) and np.array_equal(rv.view(np.uint32), wrv.view(np.uint32))
        assert not carried.any() and rule.kept == [None] * 6
    assert len(la) == len(lb) == 4 * (I + 1)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(la, lb))


@pytest.mark.parametrize("board_,J", [((3, 3, 3), 10), ((5, 5, 4), 16)])
def test_a_played_out_game_carries_the_chosen_childs_visits(board_, J):
    m, n, k = board_
    C, N = m * n, 3
    rule = ReusePuct(k, J, 1.25, table_evaluator(C), tree_nodes=J * (C + 1) + 1, seed=1)  # (never truncates)
    obs = np.zeros((N, 2, m, n), np.float32)
    obs[1, 0, 0, 0] = obs[1, 1, m - 1, n - 1] = 1
    prev, carried_some = None, False
    for ply in range(C):
        a, v, rv, carried = rule.act(obs, step=ply)
        for i in range(N):
            t = rule.trees[i]
            assert v[i].sum() == t.n[0] - 1 and t.n[0] - 1 == carried[i, 1] - (1 if carried[i, 0] else 0) + J
            if prev is not None and not prev[2][i]:
                # the tree of the child that was chosen: its count and its whole subtree
                pa, pv, _ = prev
                assert carried[i, 1] == pv[i, pa[i]] and carried[i, 0] >= 1
                carried_some = True
            else:
                assert (carried[i] == 0).all()
        obs, ended = play(obs, a, k)
        prev = (a, v, ended)
        obs[ended] = 0  # a reset game: an empty board, black to move
    assert carried_some


def test_a_truncated_tree_is_well_formed_and_keeps_creation_order():
    m, n, k, J = 5, 5, 4, 24
    C, N = m * n, 4
    rule = ReusePuct(k, J, 1.25, table_evaluator(C), tree_nodes=J + 4, seed=2)  # (keeps 4 nodes at most)
    obs = np.zeros((N, 2, m, n), np.float32)
    truncated = 0
    for ply in range(6):
        a, v, rv, carried = rule.act(obs, step=ply)
        for i in range(N):
            t, kept = rule.trees[i], rule.kept[i]
            assert len(t.n) <= J + 4
            for u, kids in enumerate(t.kids):  # every child exists, was created after its parent, and only once
                assert all(u < ch < len(t.n) for ch in kids.values())
            assert sorted(ch for kids in t.kids for ch in kids.values()) == list(range(1, len(t.n)))
            if ply:
                assert kept is not None and kept == sorted(kept) and len(kept) == carried[i, 0] <= 4
                truncated += len(kept) == 4
                assert v[i].sum() <= t.n[0] - 1
        obs, ended = play(obs, a, k)
        assert not ended.any()
    assert truncated


def test_two_stones_of_one_colour_or_three_stones_start_fresh():
    m, n, k, J = 4, 4, 3, 8
    ev = table_evaluator(m * n)
    base = board(["x...", "....", "..o.", "...."])

    def with_stones(me=(), other=()):
        o = base.copy()
        for a in me:
            o[0, 0].reshape(-1)[a] = 1
        for a in other:
            o[0, 1].reshape(-1)[a] = 1
        return o

    def second_act(obs2):
        rule = ReusePuct(k, J, 1.25, ev, seed=3)
        rule.act(base, step=0)
        return rule.trees[0], rule.act(obs2, step=1)

    # the same position continues with the whole tree; two plies on through the searched line, with that grandchild's
    first, (_, _, _, carried) = second_act(base)
    assert carried[0, 0] == len(first.n) and carried[0, 1] == J + 1
    a1, ch = max(first.kids[0].items(), key=lambda kv: first.n[kv[1]])
    a2, gch = next(iter(first.kids[ch].items()))
    assert not first.term[gch]
    _, (_, v, _, carried) = second_act(with_stones(me=(a1,), other=(a2,)))
    assert carried[0, 1] == first.n[gch] and 1 <= carried[0, 0] < len(first.n) and v[0].sum() == first.n[gch] - 1 + J
    # one colour gained two stones; three stones; a stone vanished; the planes swapped with nothing played
    for obs2 in (with_stones(me=(1, 2)), with_stones(other=(1, 2)), with_stones(me=(1, 2), other=(3,)),
                 with_stones(me=(1,), other=(2, 3)), base[:, ::-1].copy(), np.zeros_like(base)):
        _, (a, v, rv, carried) = second_act(obs2)
        wa, wv, wrv = puct(obs2, k, J, 1.25, ev, seed=3, step=1)
        assert not carried.any(), obs2
        assert np.array_equal(a, wa) and np.array_equal(v, wv) and np.array_equal(rv, wrv)
    # one ply on, through a child that was never created: fresh as well
    rule = ReusePuct(k, 1, 1.25, ev, seed=3)
    rule.act(base, step=0)
    (cell,) = rule.trees[0].kids[0]
    other = next(c for c in range(m * n) if c != cell and not base.reshape(2, -1)[:, c].any())
    nxt = np.stack([base[0, 1], base[0, 0]])[None].copy()
    nxt[0, 1].reshape(-1)[other] = 1
    assert not rule.act(nxt, step=1)[3].any()


def test_a_terminal_child_is_never_a_new_root():
    obs = board(["xx.", "oo.", "..."])  # x wins at (0, 2)
    uniform = lambda o, msk: ((msk / msk.sum(axis=1, keepdims=True)).astype(np.float32), np.zeros(len(msk), np.float32))  # noqa: E731
    rule = ReusePuct(3, 12, 1.25, uniform, seed=4)
    a, v, _, _ = rule.act(obs)
    assert a[0] == 2 and rule.trees[0].term[rule.trees[0].kids[0][2]] == 1
    nxt, ended = play(obs, a, 3)
    assert ended[0] and not rule.act(nxt, step=1)[3].any()


# ----------------------------------------------------------------------------- the C ABI and the Python arguments
def test_header_declares_the_rebase_and_the_binding_matches(lib):
    check_header_and_binding(lib, "mnk_puct_rebase")


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    p = 0x1000  # a non-NULL pointer that must never be touched

    def rebase(obs=p, dtype=0, N=8, m=9, n=9, k=5, cap=512, keep=257, ws=p, lo=p, ldt=0, lm=p, carried=None):
        return lib.call("mnk_puct_rebase", obs, dtype, N, m, n, k, cap, keep, ws, lo, ldt, lm, carried, None)

    for bad in (dict(obs=None), dict(ws=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(dtype=3), dict(ldt=-1),
                dict(cap=0), dict(cap=2049), dict(keep=0), dict(keep=513), dict(k=10), dict(m=40, n=40)):
        with pytest.raises(lib.MnkHipError, match="mnk_puct_rebase"):
            rebase(**bad)
    assert rebase(N=0) == 0 and rebase(N=0, cap=2048, keep=2048, carried=p) == 0 and rebase(N=0, cap=1, keep=1) == 0


def test_the_policies_validate_the_new_arguments(lib):
    import torch

    from selfplay.policy import PUCTSearchPolicy

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731
    pol = PUCTSearchPolicy(5, evaluator=ev)
    assert pol.reuse is False and pol.tree_nodes == 257
    pol = PUCTSearchPolicy(5, evaluator=ev, iterations=64, reuse=True)
    assert pol.reuse is True and pol.tree_nodes == 129
    pol.reset_tree()  # (no buffers yet: nothing to do)
    assert PUCTSearchPolicy(5, evaluator=ev, iterations=64, reuse=True, tree_nodes=65).tree_nodes == 65
    assert PUCTSearchPolicy(5, evaluator=ev, iterations=2048, reuse=True, tree_nodes=2049).tree_nodes == 2049
    for bad in (dict(iterations=64, tree_nodes=64), dict(iterations=64, tree_nodes=2050), dict(iterations=1025),
                dict(iterations=2048)):
        with pytest.raises(ValueError, match="tree_nodes"):
            PUCTSearchPolicy(5, evaluator=ev, reuse=True, **bad)
    with pytest.raises(ValueError, match="reuse"):
        PUCTSearchPolicy(5, evaluator=ev, tree_nodes=300)
