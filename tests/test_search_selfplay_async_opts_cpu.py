"""CPU: per-row search self-play with root noise and the solver -- the C ABI of ``mnk_search_selfplay_advance_opts``
(header, exports, binding, the host's argument checks, which reject before anything is enqueued), the argument checks of
``AsyncSearchSelfPlay``, and the numpy restatement in tests/search_selfplay_async_opts_rule.py: against the plain rule with
the options off, against the lockstep composition (``SolverPuct`` visits -> ``SelfPlayRule.step``) with the solver, and its
proofs against brute force."""
import functools
import re

import numpy as np
import pytest

import puct_solver_rule as ps
from player_cases import HEADER, check_header_and_binding, lib  # noqa: F401 (lib: the fixture)
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_async_rule import AsyncSelfPlayRule, exact_np
from search_selfplay_rule import Z_UNKNOWN, SelfPlayRule


# ----------------------------------------------------------------------------- a. the entry point
def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl, name
    return [" ".join(a.split()) for a in decl.group(1).split(",") if a.strip()]


def test_the_header_declares_the_entry_point_and_the_binding_has_it(lib):
    check_header_and_binding(lib, "mnk_search_selfplay_advance_opts")
    old, new = _params("mnk_search_selfplay_advance"), _params("mnk_search_selfplay_advance_opts")
    # every argument of the old entry point up to err, the options, the stream
    assert new == old[:-1] + ["int solver", "float noise_alpha", "float noise_eps", "int noise_fast",
                              "float* root_priors", "void* stream"]
    sig = lib.SIGNATURES
    assert sig["mnk_search_selfplay_advance_opts"][:len(old) - 1] == sig["mnk_search_selfplay_advance"][:-1]
    assert lib.ABI_VERSION == 6  # additive, like every entry point since version 6


# ----------------------------------------------------------------------------- b. the host's checks
def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000
    nan, inf = float("nan"), float("inf")

    def adv(ws=p, pl=p, me=p, N=8, m=9, n=9, k=5, I=8, fast=4, thr=2 ** 31, pri=p, pdt=0, val=p, vdt=0, c=1.25, temp=0,
            rows=p, T=81, rp=p, rv=p, rz=p, lo=p, ldt=0, lm=p, solver=1, alpha=0.3, eps=0.25, nfast=0, roots=None):
        return lib.call("mnk_search_selfplay_advance_opts", ws, pl, me, N, m, n, k, I, fast, thr, pri, pdt, val, vdt, c,
                        temp, 1, None, 0, rows, T, rp, rv, rz, lo, ldt, lm, None, None, None, None, solver, alpha, eps,
                        nfast, roots, None)

    for bad in (dict(ws=None), dict(pl=None), dict(me=None), dict(pri=None), dict(val=None), dict(rows=None),
                dict(rp=None), dict(rv=None), dict(rz=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(T=80),
                dict(fast=9), dict(fast=0), dict(I=0, fast=0), dict(I=2049, fast=1), dict(thr=2 ** 32 + 1), dict(pdt=2),
                dict(vdt=-1), dict(ldt=3), dict(c=-1.0), dict(c=nan), dict(temp=-1), dict(k=10), dict(m=40, n=40),
                dict(solver=2), dict(solver=-1), dict(alpha=-0.3), dict(alpha=nan), dict(alpha=inf), dict(eps=-0.1),
                dict(eps=1.5), dict(eps=nan), dict(eps=1.5, alpha=0.0), dict(nfast=2), dict(nfast=-1)):
        for N in (8, 0):  # (the checks come before the empty batch's early return)
            with pytest.raises(lib.MnkHipError, match="mnk_search_selfplay_advance_opts"):
                adv(**dict(bad, N=bad.get("N", N)))
    assert adv(N=0) == 0 and adv(N=0, thr=2 ** 32, fast=8) == 0 and adv(N=0, thr=0, fast=1, I=2048) == 0
    assert adv(N=0, solver=0, alpha=0.0, eps=0.0) == 0 and adv(N=0, alpha=0.0, eps=1.0, nfast=1, roots=p) == 0
    assert adv(N=0, alpha=3.0e38, eps=0.0) == 0 and adv(N=0, m=25, n=25, T=625) == 0  # (a large board)


# ----------------------------------------------------------------------------- c. the class
def test_the_class_checks_its_options_before_touching_the_gpu(lib):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    ev = lambda o, m: None  # noqa: E731 (never called)
    for bad in (dict(root_noise=(0.3,)), dict(root_noise=(0, 0.25)), dict(root_noise=(0.3, 2)), dict(noise_on_fast=True),
                dict(root_noise=(float("nan"), 0.25)), dict(root_noise=0.3)):
        with pytest.raises(ValueError):
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", **bad)


# ----------------------------------------------------------------------------- d. the rule
M, N_, K = 3, 3, 3
C = M * N_
FULL, FAST, THRESHOLD = 6, 2, 3 * 2 ** 30


def run(rule, rounds, other=None):
    """``rounds`` launches of ``rule`` with the dyadic evaluator; ``other``: a rule that must go the same way"""
    ev = exact_np(rule.C)
    obs, mask = rule.view()
    for r in range(rounds):
        out = rule.advance(*ev(obs, mask))
        if other is not None:
            want = other.advance(*ev(obs, mask))
            for a, b, what in zip(out, want, ("leaves", "masks", "fresh")):
                assert np.array_equal(a, b), f"{what}, round {r}"
        obs, mask, _ = out
    return rule


def assert_same_games(a, b):
    assert np.array_equal(a.ring_planes, b.ring_planes) and np.array_equal(a.ring_visits, b.ring_visits)
    assert np.array_equal(a.ring_z, b.ring_z) and np.array_equal(a.boards, b.boards) and np.array_equal(a.meta(), b.meta())
    assert a.row_plies.tolist() == b.row_plies.tolist() and a.stats.tolist() == b.stats.tolist()
    assert a.plies_max == b.plies_max and a.errors == b.errors == []
    assert (a.full_records, a.fast_records) == (b.full_records, b.fast_records)


def test_with_the_options_off_it_is_the_plain_rule_round_by_round():
    args = (M, N_, K, 7, C, FULL, FAST, THRESHOLD, 1.25, 2, 6, 3)
    plain = AsyncSelfPlayRule(*args)
    rule = run(AsyncOptsRule(*args), 130, plain)
    assert_same_games(rule, plain)
    assert plain.stats[0] > 0 and plain.fast_records > 0 and plain.full_records > 0 and plain.row_plies.min() > 2 * C
    assert rule.noised_roots == 0 and rule.plain_roots > 0 and not rule.proven_plies


def test_noise_of_weight_zero_is_no_noise():
    args = (M, N_, K, 7, C, FULL, FAST, THRESHOLD, 1.25, 2, 6, 3)
    off = AsyncOptsRule(*args)
    rule = run(AsyncOptsRule(*args, root_noise=(0.3, 0.0), noise_on_fast=True), 130, off)
    assert_same_games(rule, off)
    assert rule.noised_roots > 0 and rule.plain_roots == 0
    # and noise of some weight plays other games; without noise_on_fast only the full plies' roots take it
    noisy = run(AsyncOptsRule(*args, root_noise=(0.3, 0.25)), 130)
    assert not np.array_equal(noisy.ring_visits, off.ring_visits)
    assert noisy.noised_roots > 0 and noisy.plain_roots > 0


SOLVER_N, SOLVER_I, SOLVER_TEMP, SOLVER_SEED, SOLVER_ID0 = 6, 16, 3, 13, 5


@functools.lru_cache(maxsize=None)
def solver_runs(board=(M, N_, K), N=SOLVER_N, I=SOLVER_I, temp=SOLVER_TEMP, seed=SOLVER_SEED, id0=SOLVER_ID0):
    """every ply full, T = 8 C: the rule with the solver until every row has P = 2 C plies, and the lockstep composition
    for P plies: (rule, lockstep rule, P, launches used)"""
    m, n, k = board
    cells = m * n
    T, P = 8 * cells, 2 * cells
    ev = exact_np(cells)
    rule = AsyncOptsRule(m, n, k, N, T, I, I, 2 ** 32, 1.25, temp, seed, id0, solver=True)
    obs, mask = rule.view()
    rounds = 0
    while rule.row_plies.min() < P:
        obs, mask, _ = rule.advance(*ev(obs, mask))
        rounds += 1
        assert rounds <= 3 * P * (I + 1)
    lock = SelfPlayRule(m, n, k, N, T)
    search = ps.SolverPuct(k, I, 1.25, ev, seed=seed, env_id0=id0)
    for p in range(P):
        _, visits, _, _, _ = search.act(lock.view()[0], step=p)
        lock.step(visits, temp, seed, p, id0)
    return rule, lock, P, rounds


def test_with_the_solver_the_games_are_the_lockstep_solvers_and_proven_roots_play_at_once():
    rule, lock, P, rounds = solver_runs()
    assert not rule.errors and not lock.errors
    for i in range(rule.N):
        assert np.array_equal(rule.ring_planes[:P, :, :, i], lock.ring_planes[:P, :, :, i]), f"planes, row {i}"
        assert np.array_equal(rule.ring_visits[:P, i], lock.ring_visits[:P, i]), f"visits, row {i}"
    known = lock.ring_z[:P] != Z_UNKNOWN
    assert known.any() and np.array_equal(rule.ring_z[:P][known], lock.ring_z[:P][known])
    assert rule.row_plies.max() > P, "no row ran ahead"
    assert rule.row_plies.max() <= rule.T  # (no slot below P was written twice)
    assert rounds < P * (SOLVER_I + 1)
    assert lock.stats[0] > 0 and lock.ring_visits[:P].any()


def _large_cases():
    from test_gpu_search_selfplay_async_opts import LARGE_CASES

    return LARGE_CASES


@pytest.mark.parametrize("case", _large_cases(), ids=lambda c: "x".join(map(str, c[0])))
def test_the_large_cases_use_every_option_they_turn_on(case):
    """the GPU test's runs on 17x17x5 and 25x25x5 (ten and 21 words a plane) with the rule alone and its own noise: a
    game ends, fast and full plies are recorded, the rows run out of step, a ply ends by proof, roots take the noise"""
    from test_gpu_search_selfplay_async_opts import new_rule

    board, N, _, _, _, temp, rounds, start, seed, noise, on_fast, solver = case
    rule = new_rule(board, N, temp, seed, start, noise, on_fast, solver)
    ev = exact_np(rule.C)
    obs, mask = rule.view()
    for _ in range(rounds):
        obs, mask, _ = rule.advance(*ev(obs, mask))
    by_proof = sum(1 for rec in rule.proven_plies if rec[4])
    print(f"{board}: games {rule.stats[0]}, fast / full records {rule.fast_records} / {rule.full_records}, row plies "
          f"{rule.row_plies.tolist()}, by proof {by_proof}, noised / plain roots {rule.noised_roots} / {rule.plain_roots}")
    assert N % 4 and noise and solver and not on_fast and not rule.errors
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0
    assert len(set(rule.row_plies.tolist())) > 1 and by_proof > 0 and rule.noised_roots > 0 and rule.plain_roots > 0


def test_every_root_proven_by_the_rule_has_the_value_brute_force_gives_it():
    rule, _, _, _ = solver_runs()
    early = [rec for rec in rule.proven_plies if rec[4]]
    assert len(early) >= 10, "hardly a ply ended by proof"
    seen = set()
    for i, p, root, proof, _ in rule.proven_plies:
        # (the proof is from the view of the player who moved into the root: _VALUE turns it to the side to move's)
        assert ps._VALUE[proof] == ps.negamax(root, M, N_, K), (i, p)
        seen.add(proof)
    assert seen == {ps.WIN, ps.DRAW, ps.LOSS}
