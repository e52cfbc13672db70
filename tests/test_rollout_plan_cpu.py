"""CPU: which kernel ``mnk_rollout_random`` picks for a launch (``mnk_rollout_form``, no GPU needed).

Every kernel form computes the same bits, so no parity test notices a launcher that picks the wrong one -- it only
runs at the wrong speed.  Here the rules are restated in Python from their description (include/mnk_hip.h)
without calling the library, and compared with the library's answer over the full product of boards, batch sizes,
launch lengths, record / log combinations and developer knobs; a short list of literal rows stands beside it for
the case that restatement and code share a misreading."""
import itertools
import os

import pytest

import __graft_entry__ as entry

U8, U16, BITS7, U8P1 = 1, 2, 3, 4
LANE, PAIR, PAIRW, WS2, WS4 = 1, 2, 3, 4, 5
SADDR, JIT, JIT_ONLY = 0x10, 0x20, 0x40
ELAUNCH = -3

BUILTIN = [(9, 9, 5), (3, 3, 3), (13, 13, 5), (15, 15, 5), (19, 19, 5)]
BOARDS = BUILTIN + [(7, 9, 5), (8, 3, 3), (12, 13, 5), (16, 15, 5), (18, 19, 5)] + \
    [(12, 12, 5), (6, 7, 4), (7, 9, 7), (11, 11, 5)] + [(25, 25, 5)]
BATCHES = [1, 64, 32768, 32769, 65536, 65537, 131072]
PLIES = [1, 4, 256, 65535]
KNOBS = {"MNK_ROLLOUT_PAIR": [None, "0", "1"],
         "MNK_ROLLOUT_FORM": [None, "lane", "pair", "pairw", "ws2", "ws4", "diagonal"],
         "MNK_JIT": [None, "0", "1"],
         "MNK_ROLLOUT_SADDR": [None, "0"]}


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    entry._ensure_path()
    import mnk_hip

    saved = {key: os.environ.get(key) for key in KNOBS}
    yield mnk_hip
    for key, val in saved.items():
        if val is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = val
    mnk_hip.reload_config()


def set_knobs(lib, **knobs):
    for key in KNOBS:
        val = knobs.get(key)
        if val is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = val
    lib.reload_config()


def words(m, n):
    return (m * (n + 1) + 31) // 32


def log_formats(c):
    """what mnk_act_format_ok admits for a board of c cells, plus no log"""
    return [0, U16] + ([U8] if c <= 256 else []) + ([BITS7] if c <= 128 else []) + ([U8P1] if 256 < c <= 512 else [])


def restated(board, N, T, rec, act, jit_failed, pair, form, jit, saddr):
    """the rule list, first match wins; knobs as the environment holds them (None: unset)"""
    m, n, k = board
    nw = words(m, n)
    builtin = (n, k, nw) in {(bn, bk, words(bm, bn)) for bm, bn, bk in BUILTIN}  # matched by width, k and words, never by m
    fits32 = (T * nw + 1) * N * 8 < 2 ** 32
    small = (pair == "1") if pair is not None else N <= 32768
    use_pair = builtin and fits32 and act != BITS7 and small
    saddr_ok = saddr != "0" and N <= 65536 and fits32
    # 1. a forced waves-per-group form, where the board has it and there is no log
    if form in ("ws2", "ws4") and builtin and n in (9, 19) and act == 0:
        return WS2 if form == "ws2" else WS4
    # 2. boards without ahead-of-time variants: their run-time compiled kernel
    if not builtin:
        only = nw > 16
        want = only or ((jit == "1") if jit is not None else N * T >= 2 ** 20)
        if want and not jit_failed:
            flags = JIT | (JIT_ONLY if only else 0)
            # (SADDR here is the compiled ONE-LANE kernel's: the form itself, or the next try behind a compiled pair kernel)
            flags |= SADDR if rec and saddr_ok else 0
            if fits32 and act not in (BITS7, U8P1) and form != "lane" and small:
                return PAIR | flags
            return LANE | flags
        if jit_failed and only:
            return ELAUNCH
    # 3. two lanes per env, the board's words split
    if builtin and k == 5 and fits32 and act != BITS7 and \
            (form == "pairw" or (use_pair and n >= 13 and not (form == "pair" and act != U8P1))):
        return PAIRW
    # 4. two lanes per env, the scan directions split
    if use_pair and act != U8P1:
        return PAIR
    # 5. one lane per env
    return LANE | (SADDR if rec and saddr_ok and builtin else 0)


def test_the_launchers_choice_equals_the_restated_rules_over_the_full_product(lib):
    query = lib.load().mnk_rollout_form
    launches = [(b, N, T, rec, act, failed) for b in BOARDS for N in BATCHES for T in PLIES for rec in (0, 1)
                for act in log_formats(b[0] * b[1]) for failed in (0, 1)]
    seen = set()
    for pair, form, jit, saddr in itertools.product(*KNOBS.values()):
        set_knobs(lib, MNK_ROLLOUT_PAIR=pair, MNK_ROLLOUT_FORM=form, MNK_JIT=jit, MNK_ROLLOUT_SADDR=saddr)
        for b, N, T, rec, act, failed in launches:
            got = query(N, b[0], b[1], b[2], T, rec, act, failed)
            want = restated(b, N, T, rec, act, failed, pair, form, jit, saddr)
            if got != want:
                pytest.fail(f"{b} N={N} T={T} records={rec} log={act} jit_failed={failed} MNK_ROLLOUT_PAIR={pair} "
                            f"MNK_ROLLOUT_FORM={form} MNK_JIT={jit} MNK_ROLLOUT_SADDR={saddr}: library {got:#x}, rules {want:#x}")
            seen.add(want)
    # the product reaches every form, every flag and the error
    assert {LANE, PAIR, PAIRW, WS2, WS4, LANE | SADDR, PAIR | JIT, LANE | JIT | SADDR, LANE | JIT | JIT_ONLY, ELAUNCH} <= seen


# board, N, T, records, log, knobs, jit_failed -> the answer; each row can be checked against the launcher by eye
ROWS = [
    ((9, 9, 5), 65536, 256, 1, 0, {}, 0, LANE | SADDR),                  # the headline launch
    ((9, 9, 5), 131072, 256, 1, 0, {}, 0, LANE),                         # bound by the HBM write rate: 64-bit stores
    ((9, 9, 5), 32768, 256, 1, 0, {}, 0, PAIR),
    ((9, 9, 5), 32768, 256, 0, BITS7, {}, 0, LANE),                      # the 7-bit log exists in the one-lane form only
    ((13, 13, 5), 32768, 256, 1, 0, {}, 0, PAIRW),
    ((15, 15, 5), 32768, 256, 1, 0, {}, 0, PAIRW),
    ((19, 19, 5), 32768, 256, 1, 0, {}, 0, PAIRW),
    ((19, 19, 5), 32768, 65535, 1, 0, {}, 0, LANE),                      # the record rows do not fit 32-bit offsets
    ((19, 19, 5), 16384, 256, 1, U8P1, {"MNK_ROLLOUT_FORM": "pair"}, 0, PAIRW),  # only the word split writes that log
    ((3, 3, 3), 64, 16, 0, 0, {"MNK_ROLLOUT_FORM": "ws4"}, 0, PAIR),     # no ws form on this board: the knob is ignored
    ((9, 9, 5), 64, 16, 0, 0, {"MNK_ROLLOUT_FORM": "lane"}, 0, PAIR),    # the quirk: `lane` alone does not select one lane
    ((9, 9, 5), 64, 16, 0, 0, {"MNK_ROLLOUT_PAIR": "0"}, 0, LANE),       # ... MNK_ROLLOUT_PAIR=0 does
    ((12, 12, 5), 64, 4, 0, 0, {}, 0, LANE),                             # generic kernel, too small to compile for
    ((12, 12, 5), 4096, 256, 0, 0, {}, 0, PAIR | JIT),                   # 2^20 env-steps: compiled, two lanes per env
    ((12, 12, 5), 65536, 256, 1, 0, {}, 0, LANE | JIT | SADDR),
    ((12, 12, 5), 65536, 256, 1, 0, {}, 1, LANE),                        # the compile failed: generic, 64-bit stores
    ((25, 25, 5), 1, 1, 0, 0, {}, 0, PAIR | JIT | JIT_ONLY),             # more than 16 words per plane: compiled or nothing
    ((25, 25, 5), 65536, 256, 1, 0, {"MNK_JIT": "0"}, 0, LANE | JIT | JIT_ONLY | SADDR),
    ((25, 25, 5), 1, 1, 0, 0, {}, 1, ELAUNCH),
    ((25, 25, 5), 65536, 256, 1, 0, {"MNK_JIT": "0"}, 1, ELAUNCH),
]


@pytest.mark.parametrize("board,N,T,rec,act,knobs,failed,want", ROWS)
def test_literal_rows(lib, board, N, T, rec, act, knobs, failed, want):
    set_knobs(lib, **knobs)
    assert lib.rollout_form(N, *board, T, rec, act, failed) == want


def test_the_query_rejects_what_the_launch_rejects(lib):
    set_knobs(lib)
    assert lib.rollout_form(0, 9, 9, 5, 256) == 0 and lib.rollout_form(64, 9, 9, 5, 0) == 0  # nothing to launch
    assert lib.rollout_form(64, 40, 40, 5, 4) == -2          # MNK_EGEOM
    assert lib.rollout_form(-1, 9, 9, 5, 4) == -1 and lib.rollout_form(64, 9, 9, 5, 65536) == -1
    assert lib.rollout_form(64, 13, 13, 5, 4, act_bytes=BITS7) == -1 and lib.rollout_form(64, 9, 9, 5, 4, act_bytes=U8P1) == -1
    assert lib.rollout_form(64, 19, 19, 5, 4, act_bytes=U8) == -1 and lib.rollout_form(64, 9, 9, 5, 4, act_bytes=5) == -1
