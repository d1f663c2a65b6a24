"""Rec keywords (retto_amd/csrc/ctc_keyword.h) without a GPU: the fp64 restatement in ctc_keyword_ref.py against the definition by
enumeration of every class path, the rule in plain fp32 loops (rt_debug_ctc_keywords_host) against that restatement and against
the hand-built tie cases, the exact checker against the mutants it must refuse, what rt_keywords_create's arguments are held to
(the entries go through the lexicon's compiler, which test_lexicon_cpu.py covers), and the surface: exports, header, Python
mirror."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_keyword_ref as KR
import ctc_lexicon_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host(case):
    rc, out = KR.call(_lib.load().rt_debug_ctc_keywords_host, None, *case)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


@pytest.fixture(scope="module")
def small():
    """the random exact cases with what the rule gives for them, computed once"""
    return [(c, KR.expected(*c)) for c in KR.small_cases(150)]


def tie_cases():
    """exact cases in which the rules about ties, the threshold and the pad columns decide: the hand-built ones, duplicates in a
    list, a threshold between the scores"""
    cases = [KR.known_case(rows, entry) for _, rows, entry, _ in KR.KNOWN]
    rows = [[-6, -1, -2, -5, -3], [-6, -3, -1, -5, -2], [-6, -1, -4, -2, -3]]   # (all negative: a pad column of 0 would be the maximum)
    dup = [[1], [2], [1], [1, 2], [2], [1], [3], [1, 2], [4], [1], [2, 1], [1]]
    cases.append(KR.case([(rows, 1), (rows[:2], 2), (rows[:1], 0)], 5, [dup, [[3], [1, 2], [4, 4]]], [-np.inf, -1.0]))
    cases.append(KR.case([(rows, 1)], 5, [dup], [0.0]))
    return cases


# ---------------------------------------------------------------- the rule
def test_restatement_is_the_definition_by_enumeration(small):
    """the fp64 recurrence against the largest path sum over all N^T paths whose collapsed string contains the entry; whenever
    the collapsed per-frame argmax contains the entry the score is exactly 0"""
    checked = zeros = 0
    for (z, W, b, tpl, line_kw, lists, mins), _ in small:
        d = KR.cost64(z, W, b)
        o = 0
        for T in tpl:
            if T > 0:
                sc, fi, la = KR.spot64(d[o:o + T], lists[0])
                for e, s in zip(lists[0], sc):
                    assert s == KR.brute(d[o:o + T], e), (tpl, e)
                    checked += 1
                conf, _, _ = KR.spot64(d[o:o + T], lists[0], windows=(fi, la))   # (the span holds an alignment of exactly the score)
                assert np.array_equal(conf, sc)
                am = [int(c) for c in d[o:o + T].argmax(axis=1)]
                col = [c for t, c in enumerate(am) if c != 0 and (t == 0 or c != am[t - 1])]
                for e, s in zip(lists[0], sc):
                    if any(col[i:i + len(e)] == e for i in range(len(col))) and (d[o:o + T] == 0).sum() == T:   # (a unique argmax per row)
                        assert s == 0.0
                        zeros += 1
            o += T
    assert checked > 300 and zeros > 10


@pytest.mark.parametrize("name,rows,entry,want", KR.KNOWN, ids=[k[0] for k in KR.KNOWN])
def test_known_tie_cases(name, rows, entry, want):
    c = KR.known_case(rows, entry)
    sc, fi, la = KR.spot64(KR.cost64(*c[:3]), [entry])
    assert (float(sc[0]), int(fi[0]), int(la[0])) == want
    out = run_host(c)
    assert (float(out["score"][0]), int(out["span"][0][0]), int(out["span"][0][1])) == want
    assert int(out["n"][0]) == (1 if want[0] > -np.inf else 0)
    if out["n"][0]:
        h = out["hits"][0][0]
        assert (int(h["entry"]), float(h["score"]), int(h["first_col"]), int(h["last_col"])) == (0,) + want
    assert (out["hits"]["quad"] == KR.CANARY_F).all()


def test_host_rule_is_the_restatement_bit_for_bit(small):
    for c, want in small + [(c, KR.expected(*c)) for c in tie_cases()]:
        out = run_host(c)
        assert KR.same(out, want), (c[3], c[5])
        KR.check_hits(out, *c[3:])


@pytest.mark.parametrize("N", LR.GRID_N)
def test_host_rule_on_the_grid_against_fp64(N):
    """the grid of test_gpu_keywords.py through the plain fp32 loops, by the GPU test's own checker; the figure its tolerance is
    four times of (ctc_keyword_ref.HOST_WORST) is what these loops deviate from fp64 by, measured here again"""
    c = KR.grid_case(N)
    out = run_host(c)
    worst = KR.check_grid(out, *c, tol_of=KR.tol_of)
    short = max(max(w) for T, w in worst.items() if T <= 40)
    print("host fp32 against fp64, N = %d: %.3e up to 40 steps" % (N, short), {T: "%.2e / %.2e" % w for T, w in sorted(worst.items())})
    assert short <= KR.HOST_WORST * 1.001 and KR.TOL == 4 * KR.HOST_WORST
    assert out["n"].max() == KR.HITS and (out["n"][[i for i, k in enumerate(c[4]) if k == 0]] == 0).all()


def test_stand_in_is_the_rule_and_every_mutant_is_caught(small):
    cases = small + [(c, KR.expected(*c)) for c in tie_cases()]
    for c, want in cases:
        assert KR.same(KR.stand_in(*c), want)
    for m in KR.MUTANTS:
        assert any(not KR.same(KR.stand_in(*c, mutant=m), want) for c, want in cases), m
    # ... and by the cases meant for them: the hand-built ties for the tie rules
    known = {k[0]: (KR.known_case(k[1], k[2]), k[3]) for k in KR.KNOWN}
    for m, name in (("restart_on_tie", "start_tie"), ("latest_end", "end_tie"), ("skip_across_equal", "equal_neighbours")):
        c, want = known[name]
        out = KR.stand_in(*c, mutant=m)
        assert (float(out["score"][0]), int(out["span"][0][0]), int(out["span"][0][1])) != want, m


def test_grid_checker_refuses_a_wrong_span_and_a_wrong_score():
    c = KR.grid_case(5)
    tol_of = KR.tol_of
    good = run_host(c)
    i = int(np.flatnonzero(np.isfinite(good["score"]) & (good["span"][:, 1] > good["span"][:, 0]))[0])
    for key, delta in (("score", np.float32(0.01)), ("span", np.array([1, 0], np.int32))):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][i] += delta
        with pytest.raises(AssertionError):
            KR.check_grid(bad, *c, tol_of=tol_of)


# ---------------------------------------------------------------- arguments
def test_host_entry_rejects_bad_arguments():
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f = lib.rt_debug_ctc_keywords_host
    for (tpl, line_kw, lists, mins), msg in ((([4], [2], [[[1]]], [0.0]), b"line 0 names list 2, outside [0, 1]"),
                                             (([4], [1], [[[5]]], [0.0]), b"class id 5 in entry 0 is outside [1, 5)"),
                                             (([4], [1], [[[1] * 32]], [0.0]), b"entry 0 has 32 ids"),
                                             (([-4], [1], [[[1]]], [0.0]), b"line 0 has a negative number of time steps"),
                                             (([4], [1], [[[1]]], [0.5]), b"kw_min_score[0]"),
                                             (([4], [1], [[[1]]], [np.nan]), b"kw_min_score[0]")):
        assert KR.call(f, None, z, W, b, tpl, line_kw, lists, mins)[0] == 8
        assert msg in lib.rt_last_error(None), lib.rt_last_error(None)


def test_min_score_decides_what_is_a_hit():
    rows = [[-6, -1, -2, -5, -3], [-6, -3, -1, -5, -2]]
    lst = [[1], [2], [3], [4], [1, 2]]   # costs: frame 0 [-5, 0, -1, -4, -2], frame 1 [-5, -2, 0, -4, -1]
    scores = run_host(KR.case([(rows, 1)], 5, [lst], [-np.inf]))["score"][:5].tolist()
    assert scores == [0.0, 0.0, -4.0, -1.0, 0.0]
    for floor, want in ((-np.inf, [0, 1, 4, 3, 2]), (-4.0, [0, 1, 4, 3, 2]), (-3.5, [0, 1, 4, 3]), (-1.0, [0, 1, 4, 3]), (-0.5, [0, 1, 4]), (0.0, [0, 1, 4])):
        out = run_host(KR.case([(rows, 1)], 5, [lst], [floor]))
        assert out["hits"][0]["entry"][:out["n"][0]].tolist() == want, floor


# ---------------------------------------------------------------- surface
def test_exports_header_and_python_mirror():
    names = ["rt_keywords_create", "rt_keywords_entries", "rt_keywords_entry", "rt_keywords_entry_text", "rt_keywords_min_score",
             "rt_set_rec_keywords", "rt_run_regions_keywords", "rt_results_rec_keywords", "rt_results_rec_keywords_id",
             "rt_debug_ctc_keywords", "rt_debug_ctc_keywords_host", "rt_debug_span_quad"]
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n) and ("RT_API" in header and n + "(" in header), n
    assert "#define RT_MAX_KEYWORD_LISTS 16" in header and "#define RT_KEYWORD_HITS 8" in header
    assert (_lib.MAX_KEYWORD_LISTS, _lib.KEYWORD_HITS) == (16, 8) == (16, KR.HITS)
    assert C.sizeof(_lib.KeywordHit) == KR.HIT.itemsize == 48
    assert [f[0] for f in _lib.KeywordHit._fields_] == list(KR.HIT.names)
    S = retto_amd.RettoSession
    for m in ("create_keywords", "keywords_entries", "set_rec_keywords"):
        assert callable(getattr(S, m))
    assert "keywords" in inspect.signature(S.run_regions).parameters and "keywords" in inspect.signature(S.run_regions_raw).parameters
    assert inspect.signature(S.create_keywords).parameters["min_score"].default == float("-inf")
    assert retto_amd.RecProcessorSingleResult("", 0.0).keywords is None


def test_span_quad_is_an_alnum_words_quad():
    """rt_debug_span_quad against rt_debug_word_boxes: one ALNUM word over the kept columns first_col .. last_col has the span's
    quad, bit for bit, rotated crops and rot180 included"""
    lib = _lib.load()
    dic = "a\nb\n".encode()
    for box, rot180 in (([10, 20, 210, 24, 208, 60, 8, 56], 0), ([10, 20, 210, 24, 208, 60, 8, 56], 1), ([30, 10, 60, 12, 58, 200, 28, 198], 0)):
        box = np.array(box, np.float32)
        T, Wd, rw, first, last = 40, 320, 300, 7, 19
        toks = np.array([1, 2, 1], np.int32); cols = np.array([first, 11, last], np.int32)
        words = (_lib.Word * 3)(); nw = C.c_int(0)
        assert lib.rt_debug_word_boxes(dic, len(dic), toks.ctypes.data_as(C.POINTER(C.c_int32)), cols.ctypes.data_as(C.POINTER(C.c_int32)),
                                       3, T, Wd, rw, box.ctypes.data_as(C.POINTER(C.c_float)), rot180, 640, 480, 1280, 960, words,
                                       C.byref(nw)) == 0 and nw.value == 1
        quad = np.zeros(8, np.float32)
        assert lib.rt_debug_span_quad(T, Wd, rw, box.ctypes.data, rot180, 640, 480, 1280, 960, first, last, quad.ctypes.data) == 0
        assert quad.tobytes() == np.array(list(words[0].quad), np.float32).tobytes()
    assert lib.rt_debug_span_quad(T, Wd, rw, box.ctypes.data, 0, 640, 480, 1280, 960, 5, 4, quad.ctypes.data) == 8
    assert lib.rt_debug_span_quad(T, Wd, rw, box.ctypes.data, 0, 640, 480, 1280, 960, 0, T, quad.ctypes.data) == 8
