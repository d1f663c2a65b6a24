"""Lexicon snap (retto_amd/csrc/ctc_lexicon_align.h) on the MI355X: the device path (rt_debug_ctc_lexicon's, with
k_ctc_lexicon_topk per chunk and k_ctc_lexicon_align behind it) through rt_debug_ctc_lexicon_align against the fp64 restatement in
ctc_align_ref.py.  The checks are margin-free and leave no line out (ctc_align_ref.check_align).

Measured on an MI355X over the grid of test_device_rule_against_fp64 (LR.grid_case at N in 5, 65, 6625 with the thresholds
AR.GRID_MIN_POST, default chunking and one line per chunk; fp64 reference on the same features): the worst Viterbi deviation (the
larger of |vit_out - fp64 score of the returned path| and fp64 optimum - that score) is 7.830e-5 (N = 65; 6.730e-5 at N = 5,
6.743e-5 at N = 6625) and the worst |prob - fp64 softmax| is 1.753e-6 (N = 6625; 9.734e-7 at N = 5, 1.080e-6 at N = 65): the
MEASURED_WORST_VIT / MEASURED_WORST_PROB of ctc_align_ref.py, whose VIT_TOL / PROB_TOL are four times the one and the other.  On
the long lines of test_long_lines_send_their_backpointers_through_memory (up to 513 steps, |Viterbi value| up to 3024) the worst
Viterbi deviation is 8.681e-4 (MEASURED_WORST_VIT_LONG; VIT_TOL_LONG is four times it) and the worst |prob - fp64| 8.60e-7.  The grid's planted lines leave a path margin of at least ten times VIT_TOL
(test_lexicon_align_cpu.test_grid_planted_lines_leave_a_path_margin), so their paths are held to the fp64 path itself."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_align_ref as AR
import ctc_lexicon_ref as LR

pytestmark = pytest.mark.gpu

KEYS = ("idx", "prob", "snapped", "vit", "table", "matches", "n")


def run_dev(sess, case, min_post, chunk=0):
    lib = _lib.load()
    rc, out = AR.call(lib.rt_debug_ctc_lexicon_align, sess._hd.h, *case, min_post, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case, min_post):
    rc, out = AR.call(_lib.load().rt_debug_ctc_lexicon_align_host, None, *case, min_post)
    assert rc == 0
    return out


def same_lexicon_half(sess, case, out, chunk=0):
    """the table, matches and counts are rt_debug_ctc_lexicon's, bit for bit"""
    rc, plain = LR.call(_lib.load().rt_debug_ctc_lexicon, sess._hd.h, *case, chunk=chunk)
    assert rc == 0
    for key in ("table", "matches", "n"):
        assert out[key].tobytes() == plain[key].tobytes(), key


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs and their fp64 logits, computed once"""
    out = {}
    for N in LR.GRID_N:
        case = LR.grid_case(N)
        out[N] = (case, LR.logits64(case[0], case[1], case[2]))
    return out


@pytest.mark.parametrize("N", LR.GRID_N)
def test_device_rule_against_fp64(hip_session, grid, N):
    """T = 1, T = need, T = need - 1 (infeasible: no snap) and T = 40; entry lengths 1, 7, 8, 15, 16, 31; thresholds under which
    lines snap, stay below, and never snap; once with the default chunking and once with one line per chunk, bit for bit"""
    case, l64 = grid[N]
    z, W, b, tpl, line_lex, lexicons = case
    out = run_dev(hip_session, case, AR.GRID_MIN_POST)
    wv, wp = AR.figures(out, l64, tpl, line_lex, lexicons, AR.GRID_MIN_POST)   # (printed even when a check below fails)
    print("N=%d: worst Viterbi deviation %.3e, worst |prob - fp64| %.3e" % (N, wv, wp))
    _, _, n_snapped, n_exact = AR.check_align(out, l64, tpl, line_lex, lexicons, AR.GRID_MIN_POST, AR.VIT_TOL, AR.PROB_TOL, what=N)
    LR.check_outputs(out, LR.reference(*case), tpl, line_lex, lexicons, LR.HOOK_TOL, LR.HOOK_PTOL, N)
    same_lexicon_half(hip_session, case, out)
    held = sum(1 for i, k in enumerate(line_lex) if AR.GRID_MIN_POST[k - 1] > 0 and out["n"][i] >= 1 and out["snapped"][i] == 0)
    infeasible = sum(1 for i in range(len(tpl)) if out["n"][i] == 0)
    assert n_snapped >= 10 and n_exact >= 8 and held >= 1 and infeasible >= 1, (n_snapped, n_exact, held, infeasible)
    each = run_dev(hip_session, case, AR.GRID_MIN_POST, chunk=1)   # every line a chunk of its own
    for key in KEYS:
        assert each[key].tobytes() == out[key].tobytes(), key
    print("N=%d: %d snapped, %d held to the fp64 path, %d below their threshold, %d without a match" % (N, n_snapped, n_exact, held, infeasible))


def test_long_lines_send_their_backpointers_through_memory(hip_session):
    """T = 300 with a 31-id entry (63 states): longer than the la::TILE = 256 steps that stay in LDS, so the ballots go through
    the scratch buffer and come back tile by tile; T = 256 and 257 sit on the edge, T = 513 takes three tiles; a line of 12 steps
    between them takes the LDS path in the same launch (only the 7-id entry fits it: posterior 1).  Moderate gain and little
    noise: the planted alignment's margin over any other is above 2, far beyond ten times VIT_TOL_LONG, so the four long lines
    are held to the fp64 path itself.  The Viterbi tolerance is the one measured on these lines (AR.VIT_TOL_LONG): the grid's
    belongs to 40 steps"""
    rng = np.random.default_rng(300)
    N = 65
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    long_e = LR.random_entry(rng, N, 31)
    lex = [LR.random_entry(rng, N, 7), long_e, LR.random_entry(rng, N, 16)]
    tpl = [300, 12, 256, 257, 513]
    paths = []
    for T in tpl:   # the planted alignment spreads over the line: every token's run is T // need frames long
        if T < LR.need(long_e):
            paths.append((T, None))
            continue
        short = LR.alignment(long_e, LR.need(long_e))
        rep = T // len(short)
        paths.append((T, [c for c in short for _ in range(rep)] + [short[-1]] * (T - rep * len(short))))
    z = LR.planted_features(rng, W.astype(np.float64), paths, gain=1.5, noise=0.3)
    case = (z, W, b, tpl, [1] * len(tpl), [lex])
    l64 = LR.logits64(z, W, b)
    out = run_dev(hip_session, case, [0.5], chunk=1)
    vtol, ptol = AR.VIT_TOL_LONG, AR.PROB_TOL
    print("long lines: figures", AR.figures(out, l64, tpl, [1] * len(tpl), [lex], [0.5]), "tolerances", (vtol, ptol))
    _, _, n_snapped, n_exact = AR.check_align(out, l64, tpl, [1] * len(tpl), [lex], [0.5], vtol, ptol)
    assert out["snapped"].tolist() == [1, 1, 1, 1, 1] and n_exact >= 4   # (the four long lines: a path margin above 2)
    assert out["n"][1] == 1 and out["matches"][1]["entry"][0] == 0   # the short line: the 7-id entry alone fits
    for i in (0, 2, 3, 4):
        assert out["matches"][i]["entry"][0] == 1   # the 31-id entry
    same_lexicon_half(hip_session, case, out, chunk=1)
    whole = run_dev(hip_session, case, [0.5])
    for key in KEYS:
        assert whole[key].tobytes() == out[key].tobytes(), key
    # adds and compares only: where host and device logits agree the paths do; here they are held to the same fp64 path
    host = run_host(case, [0.5])
    assert host["snapped"].tolist() == out["snapped"].tolist()


def test_known_answers_equal_the_host_entry_bit_for_bit(hip_session):
    """all-zero features, one bias on every class: every logit of a line equal, so every alignment of an entry ties and the tie
    rule alone decides -- the alignment packs to the left.  The lexicons are duplicate-heavy: the tied entries come out by index,
    and match 0 is the first copy"""
    for N in (5, 6625):
        a, b_ = 1, N - 2
        tpl = [5, 5, 1]
        z, W, b = LR.zero_feature_case(N, [-1.0] * N, sum(tpl))
        lexicons = [[[a, b_], [a, b_], [b_, a], [a, b_]], [[a, a], [a, a], [b_, b_]], [[a], [a], [b_], [a, b_]]]
        line_lex = [1, 2, 3]
        want = [a, b_, 0, 0, 0] + [a, 0, a, 0, 0] + [a]
        case = (z, W, b, tpl, line_lex, lexicons)
        min_post = [0.2, 0.2, 0.2]
        dev, host = run_dev(hip_session, case, min_post), run_host(case, min_post)
        assert dev["snapped"].tolist() == [1, 1, 1] and dev["matches"]["entry"][:, 0].tolist() == [0, 0, 0]
        assert dev["idx"].tolist() == want
        for key in ("idx", "snapped", "vit", "n"):
            assert dev[key].tobytes() == host[key].tobytes(), (N, key)
        assert dev["matches"]["entry"].tobytes() == host["matches"]["entry"].tobytes()
        l64 = LR.logits64(z, W, b)
        for o in (dev, host):
            AR.check_align(o, l64, tpl, line_lex, lexicons, min_post, AR.VIT_TOL, AR.PROB_TOL, exact_logits=True, what=N)


def test_two_equal_entries_share_the_posterior(hip_session, grid):
    """a lexicon [e, e]: each copy's posterior is about 0.5, so the line does not snap at 0.9 and snaps to entry 0 at 0.4"""
    case, l64 = grid[65]
    z, W, b, tpl, line_lex, lexicons = case
    e = max(lexicons[1], key=len)
    i = max(j for j, k in enumerate(line_lex) if k == 2)          # lexicon 2's line of 40 steps, where e is planted
    o = int(np.sum(tpl[:i]))
    one = (z[o:o + tpl[i]], W, b, [tpl[i]], [1], [[e, e]])
    for mp, fires in ((0.9, 0), (0.4, 1)):
        out = run_dev(hip_session, one, [mp])
        assert out["n"][0] == 2 and abs(float(out["matches"][0]["posterior"][0]) - 0.5) <= 1e-3
        assert out["matches"][0]["entry"][:2].tolist() == [0, 1] and out["snapped"][0] == fires
        AR.check_align(out, l64[o:o + tpl[i]], [tpl[i]], [1], [[e, e]], [mp], AR.VIT_TOL, AR.PROB_TOL)
        if fires:
            assert AR.collapse(out["idx"]) == e


def test_lines_without_a_lexicon_and_thresholds_of_zero_are_untouched(hip_session, grid):
    """line_lex mixing 0, a lexicon with snap on and one with threshold 0 in one call: rows, Viterbi slot and (lexicon 0) the flag
    of the lines that take no part keep the canaries; with every threshold 0 nothing of any line is written, the flags are 0"""
    case, l64 = grid[65]
    z, W, b, tpl, line_lex, lexicons = case
    two = [lexicons[4], lexicons[1]]
    mixed = [0, 1, 2, 0, 2, 1, 0, 0, 1, 2] + [0] * (len(tpl) - 10)
    mcase = (z, W, b, tpl, mixed, two)
    mp = [1e-6, 0.0]
    for chunk in (0, 16):
        out = run_dev(hip_session, mcase, mp, chunk=chunk)
        _, _, n_snapped, _ = AR.check_align(out, l64, tpl, mixed, two, mp, AR.VIT_TOL, AR.PROB_TOL, what=chunk)
        assert n_snapped >= 2
        same_lexicon_half(hip_session, mcase, out, chunk=chunk)
        assert all(out["snapped"][i] == (AR.CANARY_IDX if k == 0 else 0 if k == 2 else out["snapped"][i]) for i, k in enumerate(mixed))
    off = run_dev(hip_session, mcase, [0.0, 0.0])
    AR.check_align(off, l64, tpl, mixed, two, [0.0, 0.0], AR.VIT_TOL, AR.PROB_TOL)
    assert (off["idx"] == AR.CANARY_IDX).all() and not off["snapped"][[i for i, k in enumerate(mixed) if k]].any()
    same_lexicon_half(hip_session, mcase, off)


def test_bad_arguments_are_rejected(hip_session):
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f, h = lib.rt_debug_ctc_lexicon_align, hip_session._hd.h
    for case, mp, chunk, msg in ((([4], [2], [[[1]]]), [0.5], 0, b"line 0 names lexicon 2, outside [0, 1]"),
                                 (([4], [1], [[[1]]]), [float("nan")], 0, b"lex_min_post[0] = nan is outside [0, 1]"),
                                 (([4], [1], [[[1]]]), [1.25], 0, b"lex_min_post[0] = 1.25"),
                                 (([4], [1], [[[1]]]), [0.5], -1, b"chunk_rows is negative")):
        assert AR.call(f, h, z, W, b, *case, mp, chunk=chunk)[0] == 8
        assert msg in lib.rt_last_error(h), lib.rt_last_error(h)   # each failure has its own message
