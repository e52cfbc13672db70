"""CPU: search self-play -- the numpy restatement in tests/search_selfplay_rule.py (outcome labels of won, drawn and running
games; the symmetry maps; the move choice against puct_rule's temperature rules); the C ABI of
``mnk_search_selfplay_step`` / ``mnk_search_gather`` (header, binding, host argument checks, which reject before anything
is enqueued); the argument checks of ``SearchSelfPlay`` and ``SearchReplayBuffer``."""
import itertools
import re

import numpy as np
import pytest

from oracle import philox
from player_cases import HEADER, check_header_and_binding, header_constants, lib, positions  # noqa: F401 (lib: the fixture)
from puct_rule import puct
from search_selfplay_rule import Z_UNKNOWN, SelfPlayRule, gather, pick_by_visits, sym_perm


def one_hot(N, C, cells):
    v = np.zeros((N, C), np.int32)
    v[np.arange(N), cells] = 5
    return v


def play_script(rule, script, temp_plies=0):
    """plays row 0 through the cells of ``script`` (one-hot visits: the move is forced)"""
    for p, a in enumerate(script):
        rule.step(one_hot(1, rule.C, [a]), temp_plies, seed=3, p=p)


# ----------------------------------------------------------------------------- outcome labels
def test_a_won_game_is_labelled_alternately_back_from_the_winner():
    rule = SelfPlayRule(3, 3, 3, 1, 9)
    play_script(rule, [0, 3, 1, 4, 2])  # black takes the top row on ply 5
    assert rule.ring_z[:5, 0].tolist() == [1, -1, 1, -1, 1]
    assert rule.ring_z[5:, 0].tolist() == [Z_UNKNOWN] * 4
    assert rule.stats.tolist() == [1, 1, 0, 0, 5]
    assert not rule.boards.any() and rule.moves[0] == 0 and rule.side[0] == 0  # reset


def test_a_white_win_after_a_wrap_labels_the_records_mod_T():
    rule = SelfPlayRule(3, 3, 3, 1, 9)
    play_script(rule, [0, 3, 1, 4, 2])             # plies 0-4: a black win
    for p, a in enumerate([0, 3, 1, 4, 8, 5], start=5):  # plies 5-10: white completes the middle row
        rule.step(one_hot(1, 9, [a]), 0, seed=3, p=p)
    z = rule.ring_z[:, 0].tolist()
    # records of plies 5..10 sit at rows 5, 6, 7, 8, 0, 1; the last (ply 10, white to move) is a win
    assert [z[r] for r in (5, 6, 7, 8, 0, 1)] == [-1, 1, -1, 1, -1, 1]
    assert z[2:5] == [1, -1, 1]                     # the first game's labels survive
    assert rule.stats.tolist() == [2, 1, 1, 0, 11]


def test_a_draw_is_labelled_zero_and_a_running_game_stays_unknown():
    draw = [0, 1, 2, 4, 3, 5, 7, 6, 8]  # x o x / x o o / o x x: nobody has three
    rule = SelfPlayRule(3, 3, 3, 1, 12)
    play_script(rule, draw)
    assert rule.ring_z[:9, 0].tolist() == [0] * 9 and rule.stats.tolist() == [1, 0, 0, 1, 9]
    rule.step(one_hot(1, 9, [4]), 0, seed=1, p=9)
    assert rule.ring_z[9, 0] == Z_UNKNOWN


def test_a_row_without_visits_is_an_error_and_is_not_played():
    rule = SelfPlayRule(3, 3, 3, 2, 9)
    v = np.zeros((2, 9), np.int32)
    v[0, 4] = 3
    v[1, 4] = -7  # negative counts are no visits
    rule.step(v, 0, seed=0, p=0)
    assert rule.errors == [(4, 1)] and rule.moves.tolist() == [1, 0]
    assert rule.ring_z[0].tolist() == [Z_UNKNOWN, Z_UNKNOWN]


def test_occupied_cells_and_large_counts_are_masked_and_clamped():
    rule = SelfPlayRule(3, 3, 3, 1, 9)
    rule.step(one_hot(1, 9, [4]), 0, seed=0, p=0)
    v = np.full((1, 9), 100000, np.int32)
    v[0, 0] = 1
    rule.step(v, 0, seed=0, p=1)
    assert rule.ring_visits[1, 0, 4] == 0 and rule.ring_visits[1, 0, 1] == 65535 and rule.ring_visits[1, 0, 0] == 1


# ----------------------------------------------------------------------------- symmetries
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4), (9, 9), (3, 5), (6, 4)])
def test_symmetries_are_distinct_bijections_closed_under_composition(m, n):
    count = 8 if m == n else 4
    perms = [sym_perm(s, m, n) for s in range(count)]
    for p in perms:
        assert sorted(p.tolist()) == list(range(m * n))
    keys = {tuple(p) for p in perms}
    assert len(keys) == count
    for a, b in itertools.product(perms, perms):
        assert tuple(a[b]) in keys  # (output reads a[b[x]]: one map after the other)
    assert perms[0].tolist() == list(range(m * n))


@pytest.mark.parametrize("m,n,k", [(3, 3, 3), (5, 5, 4), (4, 6, 3)])
def test_symmetries_map_legal_masks_onto_legal_masks(m, n, k):
    obs = positions(m, n, k, 12, seed=m * n)
    rule = SelfPlayRule(m, n, k, len(obs), m * n)
    count = 8 if m == n else 4
    for i, o in enumerate(obs):
        rule.ring_planes[0, :, :, i] = np.stack([pack(o[c].reshape(-1), m, n) for c in (0, 1)])
    idx = np.arange(len(obs))
    for s in range(count):
        ob, mask, _, _, _, err = gather(rule.ring_planes, rule.ring_visits, rule.ring_z, m, n, idx, np.full(len(obs), s))
        assert not err
        legal = (obs[:, 0] == 0) & (obs[:, 1] == 0)
        assert (mask == legal.reshape(len(obs), -1)[:, sym_perm(s, m, n)]).all()
        assert (ob.reshape(len(obs), 2, -1) == obs.reshape(len(obs), 2, -1)[:, :, sym_perm(s, m, n)]).all()


def pack(cells, m, n):
    from oracle.packing import pack_cells

    return pack_cells(np.asarray(cells)[None], m, n)[:, 0]


def test_gather_targets_and_errors():
    rule = SelfPlayRule(3, 3, 3, 2, 9)
    rule.ring_visits[0, 0] = [1, 2, 0, 0, 3, 0, 0, 0, 1]
    rule.ring_visits[0, 1] = [0] * 9
    rule.ring_z[0] = [-1, Z_UNKNOWN]
    idx = np.array([0, 1, -18, 18, 0])
    sym = np.array([2, 0, 0, 0, 9])
    _, _, pol, val, wt, err = gather(rule.ring_planes, rule.ring_visits, rule.ring_z, 3, 3, idx, sym)
    assert pol[0].tolist() == (np.array([0, 2, 1, 0, 3, 0, 1, 0, 0], np.float32) / np.float32(7)).tolist()
    assert pol[1].tolist() == [0.0] * 9 and val.tolist() == [-1, 0, -1, 0, -1] and wt.tolist() == [1, 0, 1, 0, 0]
    assert err == [(1, 18), (3, 4)]


# ----------------------------------------------------------------------------- the move choice = PUCT's
@pytest.mark.parametrize("temperature", [0, 1])
def test_the_move_choice_is_puct_rule_on_the_same_u32(temperature):
    m, n, k = 4, 4, 3
    obs = positions(m, n, k, 24, seed=5, max_fill=0.6)
    legal = ((obs[:, 0] == 0) & (obs[:, 1] == 0)).reshape(len(obs), -1)
    table = ((np.arange(m * n) * 37) % 16 + 1).astype(np.float32) / 16

    def ev(leaf_obs, leaf_mask):
        cnt = leaf_obs.reshape(len(leaf_obs), 2, -1).sum(axis=2)
        return leaf_mask * table, ((np.mod(cnt[:, 0] - 2 * cnt[:, 1], 5) - 2) / 4).astype(np.float32)

    acts, visits, _ = puct(obs, k, 40, 1.25, ev, seed=11, step=3, temperature=temperature)
    x = philox.rand_u32(11, np.arange(len(obs), dtype=np.uint64), 3, philox.STREAM_SAMPLE)
    checked = 0
    for i in range(len(obs)):
        if legal[i].any() and visits[i].max() > 0:
            assert pick_by_visits(visits[i], x[i], temperature == 1) == acts[i]
            checked += 1
    assert checked >= 12


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_entry_points_and_the_binding_matches(lib):
    check_header_and_binding(lib, "mnk_search_selfplay_step")
    check_header_and_binding(lib, "mnk_search_gather")
    c = header_constants()
    assert c["MNK_STREAM_SELFPLAY"] == "6" == str(lib.STREAM_SELFPLAY)
    assert c["MNK_ERR_SYMMETRY"] == "3" == str(lib.ERR_SYMMETRY) and c["MNK_ERR_VISITS"] == "4" == str(lib.ERR_VISITS)
    assert re.search(r"#define MNK_Z_UNKNOWN \(-128\)", open(HEADER).read()) and lib.Z_UNKNOWN == -128
    assert c["MNK_ABI_VERSION"] == "6" and lib.load().mnk_abi_version() == 6


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 / B = 0 launch nothing either)"""
    p = 0x1000

    def step(pl=p, me=p, N=8, m=9, n=9, k=5, vis=p, temp=0, T=81, rp=p, rv=p, rz=p, obs=p, odt=0):
        return lib.call("mnk_search_selfplay_step", pl, me, N, m, n, k, vis, temp, 1, None, 0, None, 0, T, rp, rv, rz,
                        obs, odt, None, None, None, None)

    def gath(rp=p, rv=p, rz=p, T=81, N=8, m=9, n=9, idx=p, B=4, odt=0):
        return lib.call("mnk_search_gather", rp, rv, rz, T, N, m, n, idx, None, B, p, odt, p, p, p, p, None, None)

    for bad in (dict(pl=None), dict(me=None), dict(vis=None), dict(rp=None), dict(rv=None), dict(rz=None), dict(obs=None),
                dict(N=-1), dict(T=80), dict(T=0), dict(temp=-1), dict(odt=3), dict(k=10), dict(m=40, n=40),
                dict(n=1, m=4, k=1)):
        with pytest.raises(lib.MnkHipError, match="mnk_search_selfplay_step"):
            step(**bad)
    for bad in (dict(rp=None), dict(rv=None), dict(rz=None), dict(idx=None), dict(T=-1), dict(N=-1), dict(B=-1),
                dict(odt=-1), dict(m=40, n=40)):
        with pytest.raises(lib.MnkHipError, match="mnk_search_gather"):
            gath(**bad)
    assert step(N=0) == 0 and step(N=0, T=10**6, temp=10**6) == 0 and gath(B=0) == 0 and gath(B=0, idx=None) == 0


def test_selfplay_and_buffer_validate_their_arguments(lib):
    import torch

    from alg.search_replay_buffer import SearchReplayBuffer
    from selfplay.search_selfplay import SearchSelfPlay

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731
    for bad in (dict(capacity=8), dict(num_envs=0), dict(m=40, n=40), dict(n=1, m=4)):
        args = dict(capacity=9, num_envs=4, m=3, n=3)
        args.update(bad)
        with pytest.raises(ValueError):
            SearchReplayBuffer(args["capacity"], args["num_envs"], args["m"], args["n"], device="cpu")
    for bad in (dict(temp_plies=-1), dict(num_envs=0), dict(capacity=8), dict(k=4), dict(m=40, n=40, k=5),
                dict(iterations=0), dict(iterations=2049), dict(c=-1.0), dict(c=float("nan"))):
        args = dict(m=3, n=3, k=3, num_envs=4, evaluator=ev)
        args.update(bad)
        with pytest.raises(ValueError):
            SearchSelfPlay(**args)
    with pytest.raises(ValueError):
        SearchSelfPlay(3, 3, 3, 4)                                   # neither a model nor an evaluator
    with pytest.raises(TypeError):
        SearchSelfPlay(3, 3, 3, 4, evaluator=ev, leaf_dtype=torch.float16)
    with pytest.raises(RuntimeError):                                # valid arguments, but no GPU device here
        SearchSelfPlay(3, 3, 3, 4, evaluator=ev, device="cpu")
