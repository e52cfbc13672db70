"""CPU: search self-play with per-row budgets -- the numpy restatement in tests/search_selfplay_async_rule.py against the
lockstep composition it must reduce to (``puct_rule.puct`` visits -> ``SelfPlayRule.step``), its budgets against the Philox
word, the records of fast plies; the C ABI of ``mnk_search_selfplay_advance`` (header, binding, host argument checks,
which reject before anything is enqueued); the argument checks of ``AsyncSearchSelfPlay``."""
import numpy as np
import pytest

from player_cases import check_header_and_binding, header_constants, lib  # noqa: F401 (lib: the fixture)
import search_selfplay_async_rule
from puct_rule import puct
from search_selfplay_async_rule import STREAM_BUDGET, AsyncSelfPlayRule, budget_word, exact_np
from search_selfplay_rule import Z_UNKNOWN, SelfPlayRule


def run_rule(rule, rounds, on_round=None):
    """``rounds`` launches of the rule with the dyadic evaluator; on_round(r, fresh) after each"""
    ev = exact_np(rule.C)
    obs, mask = rule.view()  # (right after begin(): the roots)
    for r in range(rounds):
        obs, mask, fresh = rule.advance(*ev(obs, mask))
        if on_round:
            on_round(r, fresh)


def test_with_every_ply_full_the_rule_is_the_lockstep_composition():
    m, n, k, N, I, c, temp, seed, id0 = 3, 3, 3, 3, 4, 1.25, 2, 11, 5
    C = m * n
    plies = 2 * C + 3
    ev = exact_np(C)
    lock = SelfPlayRule(m, n, k, N, C)
    rule = AsyncSelfPlayRule(m, n, k, N, C, I, I, 2 ** 32, c, temp, seed, id0)
    obs, mask = rule.view()
    for p in range(plies):
        l_obs, _ = lock.view()
        _, visits, _ = puct(l_obs, k, I, c, ev)
        l_obs, l_mask = lock.step(visits, temp, seed, p, id0)
        for r in range(I + 1):
            obs, mask, fresh = rule.advance(*ev(obs, mask))
            assert fresh.tolist() == [int(r == I)] * N
        assert np.array_equal(obs, l_obs) and np.array_equal(mask, l_mask), f"next roots, ply {p}"
        assert np.array_equal(rule.ring_planes, lock.ring_planes) and np.array_equal(rule.ring_visits, lock.ring_visits)
        assert np.array_equal(rule.ring_z, lock.ring_z), f"ply {p}"
        assert np.array_equal(rule.boards, lock.boards) and np.array_equal(rule.meta(), lock.meta())
        assert rule.stats.tolist() == lock.stats.tolist()
        assert rule.row_plies.tolist() == [p + 1] * N and rule.plies_max == p + 1
    assert lock.stats[0] > 0 and not rule.errors


@pytest.mark.parametrize("threshold", [0, 2 ** 31, 2 ** 32])
def test_the_budgets_follow_the_philox_word(threshold):
    m, n, k, N, full, fast, seed, id0 = 3, 3, 3, 4, 4, 1, 3, 2
    T = 200  # no wrap: every record of the run stays in the ring
    rule = AsyncSelfPlayRule(m, n, k, N, T, full, fast, threshold, 1.25, 2, seed, id0)
    since = np.zeros(N, np.int64)  # launches since the row's last ply
    diverged = []

    def on_round(r, fresh):
        since[:] += 1
        for i in np.flatnonzero(fresh):
            p = int(rule.row_plies[i]) - 1
            is_full = budget_word(seed, id0 + i, p) < threshold
            assert since[i] == (full if is_full else fast) + 1, (i, p)
            since[i] = 0
        diverged.append(len(set(rule.row_plies.tolist())) > 1)

    run_rule(rule, 120, on_round)
    assert not rule.errors and rule.stats[0] > 0
    if threshold == 0:
        assert rule.full_records == 0 and rule.fast_records == rule.row_plies.sum() and not any(diverged)
    elif threshold == 2 ** 32:
        assert rule.fast_records == 0 and rule.full_records == rule.row_plies.sum() and not any(diverged)
    else:
        assert rule.fast_records > 0 and rule.full_records > 0
        assert any(diverged), "the rows' ply counts never differed"
    assert rule.plies_max == rule.row_plies.max() < T
    # a fast ply's record carries no visits; a full ply's carries the search's; both get their outcome
    labelled = {True: 0, False: 0}
    for i in range(N):
        for p in range(int(rule.row_plies[i])):
            is_full = budget_word(seed, id0 + i, p) < threshold
            tot = int(rule.ring_visits[p, i].astype(np.int64).sum())
            assert tot == (full if is_full else 0), (i, p)
            labelled[is_full] += int(rule.ring_z[p, i] != Z_UNKNOWN)
    assert threshold == 2 ** 32 or labelled[False] > 0
    assert threshold == 0 or labelled[True] > 0


def test_a_root_without_a_legal_cell_is_reported_and_left_alone():
    rule = AsyncSelfPlayRule(3, 3, 3, 2, 9, 4, 2, 2 ** 31, 1.25, 0, 1)
    rule.boards[1, 0, ::2] = True  # a full board handed in: x o x / o x o / x o x with the move count to match
    rule.boards[1, 1, 1::2] = True
    rule.moves[1], rule.side[1] = 9, 1
    before = (rule.boards[1].copy(), rule.ring_z.copy())
    rule.begin()
    run_rule(rule, 12)
    assert set(rule.errors) == {(4, 1)} and rule.row_plies[1] == 0 and rule.row_plies[0] > 0
    assert np.array_equal(rule.boards[1], before[0]) and np.array_equal(rule.ring_z[:, 1], before[1][:, 1])


def _planted_cases():
    """one run of the GPU test per sibling board: 8x3x3 from the empty board, the others from their stored states"""
    from test_gpu_search_selfplay_async import SIBLING_BOARDS, SIBLING_CASES

    cases = [c for c in SIBLING_CASES if c[0] == (8, 3, 3) or c[7] == "golden"]
    assert [c[0] for c in cases] == list(SIBLING_BOARDS)
    return cases


@pytest.mark.parametrize("case", _planted_cases(), ids=lambda c: "x".join(map(str, c[0])))
def test_the_sibling_cases_reject_the_variants_own_board(case, monkeypatch):
    """the GPU test's run on every sibling board (tests/test_gpu_search_selfplay_async.py) with the cell and row count of
    the board its built-in variant is named after (9 / 3 for 8x3x3, 81 / 9 for 7x9x5, 169 / 13 for 12x13x5, 225 / 15 for
    16x15x5, 361 / 19 for 18x19x5): a game ends at that many stones, a row is live below that many, a run is seen in that
    many rows.  On 8x3x3 every game is cut short at 9 stones; on 16x15x5 the rows at 238 stones are not live; on the other
    three the boards that fill are never drawn, their rows sit on a full board and are reported.  (7x9x5 from the empty
    board fills no board: the stored start is the run that tells the rules apart there.)"""
    from playout_rule import has_run
    import test_gpu_search_selfplay_async as gpu_cases
    from test_gpu_search_selfplay_async import new_rule

    board, N, _, _, _, temp, rounds, start, seed = case
    (m, n, k), vm = board, board[1]
    assert vm != m

    class Planted(AsyncSelfPlayRule):
        def _ply(self, i, visits, full):
            self.C = vm * n
            try:
                return super()._ply(i, visits, full)
            finally:
                self.C = m * n

        def _fresh(self, i):
            super()._fresh(i)
            self.live[i] &= self.moves[i] < vm * n

    true = new_rule(board, N, temp, seed, start)
    run_rule(true, rounds)
    assert true.stats[0] > 0 and not true.errors
    assert true.stats[3] > 0 or board == (8, 3, 3)  # a board filled: a draw at m * n stones
    monkeypatch.setattr(search_selfplay_async_rule, "has_run", lambda planes, run: has_run(planes[:, :vm], run))
    monkeypatch.setattr(gpu_cases, "AsyncSelfPlayRule", Planted)
    wrong = new_rule(board, N, temp, seed, start)
    assert type(wrong) is Planted
    run_rule(wrong, rounds)
    print(board, true.stats.tolist(), wrong.stats.tolist(), len(wrong.errors))
    assert wrong.stats.tolist() != true.stats.tolist() and not np.array_equal(wrong.ring_z, true.ring_z)
    assert not np.array_equal(wrong.ring_planes, true.ring_planes) or not np.array_equal(wrong.planes(), true.planes())
    assert wrong.row_plies.tolist() != true.row_plies.tolist() or board == (8, 3, 3)


def _large_cases():
    from test_gpu_search_selfplay_async import LARGE_CASES

    return LARGE_CASES


@pytest.mark.parametrize("case", _large_cases(), ids=lambda c: "x".join(map(str, c[0])))
def test_the_large_cases_end_games_out_of_step_and_reject_a_cell_count_from_the_word_count(case, monkeypatch):
    """the GPU test's runs on 17x17x5 and 25x25x5 (ten and 21 words a plane) with the rule alone: a game ends, a board
    fills and is drawn at m * n stones, fast and full plies are recorded, the rows run out of step -- and with 32 cells
    a plane word for the cell count (320 for 289, 672 for 625) no board is ever full: other statistics, labels and rows"""
    import test_gpu_search_selfplay_async as gpu_cases
    from test_gpu_search_selfplay_async import new_rule

    board, N, _, _, _, temp, rounds, start, seed = case
    m, n, k = board
    cells = 32 * ((m * (n + 1) + 31) // 32)
    assert N % 4 and start == "late" and cells > m * n

    class Planted(AsyncSelfPlayRule):
        def _ply(self, i, visits, full):
            self.C = cells
            try:
                return super()._ply(i, visits, full)
            finally:
                self.C = m * n

    true = new_rule(board, N, temp, seed, start)
    run_rule(true, rounds)
    print(board, true.stats.tolist(), true.fast_records, true.full_records, true.row_plies.tolist())
    assert true.stats[0] > 0 and true.stats[3] > 0 and not true.errors
    assert true.fast_records > 0 and true.full_records > 0 and len(set(true.row_plies.tolist())) > 1
    monkeypatch.setattr(gpu_cases, "AsyncSelfPlayRule", Planted)
    wrong = new_rule(board, N, temp, seed, start)
    assert type(wrong) is Planted
    run_rule(wrong, rounds)
    assert wrong.stats.tolist() != true.stats.tolist() and not np.array_equal(wrong.ring_z, true.ring_z)


OLD_STARTS = {"12x12x5_meta": "1f5418751e261d337a1822836f24449adab097df432544ae05dec7e1464da01f",
              "12x12x5_planes": "f0c533aff52d3acfa622b6d989dcb6c46e16adbecefb02476bc4e688d2785ba9",
              "19x19x5_meta": "4402b87f47e4e9ba8fa460cea93dd1c265ea689ae68e6215beddb77cd047942c",
              "19x19x5_planes": "303e727d92e9acf1fb44a4e691f205f8bea398f4477df248326e4cdbcb03be79"}


def test_the_stored_starts_are_what_their_script_writes_and_the_first_two_are_unchanged():
    """every entry of search_selfplay_async_starts.npz is what make_golden_search_selfplay_async.py computes today, and the
    two entries the file held before the sibling boards were added are bit for bit the ones it held (SHA-256 of the array
    bytes, taken from the file before it was written again)"""
    import hashlib
    import importlib.util
    import os

    from test_gpu_search_selfplay_async import GOLDEN

    spec = importlib.util.spec_from_file_location("make_starts", os.path.join(os.path.dirname(GOLDEN),
                                                                              "make_golden_search_selfplay_async.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    with np.load(GOLDEN) as z:
        stored = {name: z[name] for name in z.files}
    assert set(stored) == {name + part for name in make.CASES for part in ("_planes", "_meta")}
    for name, digest in OLD_STARTS.items():
        assert hashlib.sha256(stored[name].tobytes()).hexdigest() == digest, name
    assert stored["12x12x5_planes"].dtype == np.uint64 and stored["12x12x5_meta"].dtype == np.uint32
    for name, (m, n, k, rows, plies, late) in make.CASES.items():
        planes, meta = make.starts(m, n, k, rows, plies, late)
        assert planes.dtype == stored[name + "_planes"].dtype and np.array_equal(planes, stored[name + "_planes"]), name
        assert meta.dtype == stored[name + "_meta"].dtype and np.array_equal(meta, stored[name + "_meta"]), name


def test_the_header_declares_the_entry_point_and_the_binding_has_it(lib):
    check_header_and_binding(lib, "mnk_search_selfplay_advance")
    assert header_constants()["MNK_STREAM_BUDGET"] == "9" and lib.STREAM_BUDGET == 9 and STREAM_BUDGET == 9


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000

    def adv(ws=p, pl=p, me=p, N=8, m=9, n=9, k=5, I=8, fast=4, thr=2 ** 31, pri=p, pdt=0, val=p, vdt=0, c=1.25, temp=0,
            rows=p, T=81, rp=p, rv=p, rz=p, lo=p, ldt=0, lm=p):
        return lib.call("mnk_search_selfplay_advance", ws, pl, me, N, m, n, k, I, fast, thr, pri, pdt, val, vdt, c, temp,
                        1, None, 0, rows, T, rp, rv, rz, lo, ldt, lm, None, None, None, None, None)

    for bad in (dict(ws=None), dict(pl=None), dict(me=None), dict(pri=None), dict(val=None), dict(rows=None),
                dict(rp=None), dict(rv=None), dict(rz=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(T=80),
                dict(fast=9), dict(fast=0), dict(I=0, fast=0), dict(I=2049, fast=1), dict(thr=2 ** 32 + 1), dict(pdt=2),
                dict(vdt=-1), dict(ldt=3), dict(c=-1.0), dict(c=float("nan")), dict(temp=-1), dict(k=10),
                dict(m=40, n=40)):
        with pytest.raises(lib.MnkHipError, match="mnk_search_selfplay_advance"):
            adv(**bad)
    assert adv(N=0) == 0 and adv(N=0, thr=2 ** 32, fast=8) == 0 and adv(N=0, thr=0, fast=1, I=2048) == 0


def test_the_class_checks_its_arguments_before_touching_the_gpu(lib):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    ev = lambda o, m: None  # noqa: E731 (never called)
    for bad in (dict(iterations=0), dict(fast_iterations=0), dict(fast_iterations=9), dict(full_prob=1.5),
                dict(full_prob=-0.1), dict(temp_plies=-1), dict(capacity=8), dict(num_envs=0), dict(k=10), dict(c=-1.0)):
        args = dict(m=3, n=3, k=3, num_envs=4, evaluator=ev, iterations=8)
        args.update(bad)
        with pytest.raises(ValueError):
            AsyncSearchSelfPlay(**args)
    with pytest.raises(ValueError):
        AsyncSearchSelfPlay(3, 3, 3, 4)  # neither a model nor an evaluator
    with pytest.raises(TypeError):
        AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, reuse=True)  # (a follow-up: DESIGN section 10)
