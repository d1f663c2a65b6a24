"""Lexicon snap (retto_amd/csrc/ctc_lexicon_align.h) without a GPU: the rule in plain fp32 loops (rt_debug_ctc_lexicon_align_host)
against the fp64 restatement in ctc_align_ref.py on the lexicon grid's inputs, the known answers of the tie rule, the checker
against the mutants it must refuse, the path margin the grid's planted lines leave, and the surface: exports, header, NULL
sessions, argument errors, Python mirror, CLI flag."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, cli

import ctc_align_ref as AR
import ctc_lexicon_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_MIN_POST = AR.GRID_MIN_POST


def host_case_tol(l64, tpl):
    """fmt_tol for the longest line and the largest |Viterbi value| a case can have: T times its largest |logit|"""
    return AR.fmt_tol(max(tpl), max(tpl) * float(np.abs(l64).max()))


def run_host(case, min_post):
    rc, out = AR.call(_lib.load().rt_debug_ctc_lexicon_align_host, None, *case, min_post)
    assert rc == 0, retto_amd._lib.load().rt_last_error(None)
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs and their fp64 logits, computed once"""
    out = {}
    for N in LR.GRID_N:
        case = LR.grid_case(N)
        out[N] = (case, LR.logits64(case[0], case[1], case[2]))
    return out


# ---------------------------------------------------------------- the host rule against fp64
@pytest.mark.parametrize("N", LR.GRID_N)
def test_host_rule_against_fp64(grid, N):
    case, l64 = grid[N]
    z, W, b, tpl, line_lex, lexicons = case
    if N == 6625:   # (plain loops, 6625 x 120 multiplications per row: the three small lexicons' lines, as test_lexicon_cpu.py)
        keep = [i for i, k in enumerate(line_lex) if k <= 3]
        offs = np.concatenate([[0], np.cumsum(tpl)])
        z = np.concatenate([z[offs[i]:offs[i + 1]] for i in keep]); l64 = np.concatenate([l64[offs[i]:offs[i + 1]] for i in keep])
        tpl = [tpl[i] for i in keep]; line_lex = [line_lex[i] for i in keep]
        case = (z, W, b, tpl, line_lex, lexicons)
    out = run_host(case, GRID_MIN_POST)
    vtol, ptol = host_case_tol(l64, tpl)
    wv, wp, n_snapped, n_exact = AR.check_align(out, l64, tpl, line_lex, lexicons, GRID_MIN_POST, vtol, ptol, what=N)
    # the lexicon half of the call is rt_debug_ctc_lexicon_host's, bit for bit
    rc, plain = LR.call(_lib.load().rt_debug_ctc_lexicon_host, None, *case)
    assert rc == 0
    for key in ("table", "matches", "n"):
        assert out[key].tobytes() == plain[key].tobytes(), key
    # both outcomes occur: lines that snapped, and lines with a match and a positive threshold that did not
    held = sum(1 for i, k in enumerate(line_lex) if k > 0 and GRID_MIN_POST[k - 1] > 0 and out["n"][i] >= 1 and out["snapped"][i] == 0)
    assert n_snapped >= 3 and n_exact >= 2 and held >= 1, (N, n_snapped, n_exact, held)
    print("host N=%d: %d snapped (%d held to the exact path), %d below their threshold; worst Viterbi deviation %.3e (tol %.3e), "
          "worst |prob - fp64| %.3e (tol %.3e)" % (N, n_snapped, n_exact, held, wv, vtol, wp, ptol))


def known_answer_case(N=5, a=1, b=3, bias=-1.0):
    """all-zero features and the same bias on every class, the blank included: every logit of every line equal, bit for bit"""
    tpl = [5, 5, 1]
    z, W, bb = LR.zero_feature_case(N, [bias] * N, sum(tpl))
    lexicons = [[[a, b]], [[a, a]], [[a]]]
    want = [[a, b, 0, 0, 0], [a, 0, a, 0, 0], [a]]
    return (z, W, bb, tpl, [1, 2, 3], lexicons), want


def test_known_answers_ties_pack_the_alignment_to_the_left():
    case, want = known_answer_case()
    z, W, b, tpl, line_lex, lexicons = case
    out = run_host(case, [0.5, 0.5, 0.5])
    assert out["snapped"].tolist() == [1, 1, 1]
    assert out["idx"].tolist() == [c for p in want for c in p]
    # every logit is the bias: the Viterbi value is T adds of it, bit for bit, and every probability 1 / N
    for i, T in enumerate(tpl):
        v = np.float32(-1.0)
        for _ in range(T - 1):
            v = np.float32(v + np.float32(-1.0))
        assert out["vit"][i].tobytes() == v.tobytes()
    assert np.abs(out["prob"].astype(np.float64) - 0.2).max() <= 1e-6
    l64 = LR.logits64(z, W, b)
    AR.check_align(out, l64, tpl, line_lex, lexicons, [0.5] * 3, *host_case_tol(l64, tpl), exact_logits=True)


# ---------------------------------------------------------------- the checker refuses the stand-in's mutants
def _random_case():
    """N = 5 (three pad columns), negative biases, noise-only lines: entries with equal neighbours, one that does not fit, a line
    of lexicon 0 between lexicon lines, a lexicon whose threshold no line reaches and one with threshold 0"""
    rng = np.random.default_rng(11)
    N = 5
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = (-1.0 - rng.random(N)).astype(np.float32)
    tpl = [6, 3, 5, 7, 6, 4, 9, 5]
    z = rng.normal(0.0, 0.7, (sum(tpl), LR.D)).astype(np.float32)
    lex1 = [[1, 1, 2], [2], [3, 4], [2, 2, 2, 2], [4, 4], [1, 2, 3], [2, 1]]
    lex2 = [[1, 1], [2, 2, 3], [4, 1, 1, 4]]
    return (z, W, b, tpl, [1, 2, 0, 2, 3, 1, 2, 4], [lex1, lex2, lex1, lex2]), [1e-4, 1e-4, 1.0, 0.0]


def test_stand_in_passes_and_every_mutant_is_refused():
    refused = set()
    known, _ = known_answer_case()
    for case, min_post, exact in ((known, [0.5] * 3, True), _random_case() + (False,)):
        z, W, b, tpl, line_lex, lexicons = case
        l64 = LR.logits64(z, W, b)
        vtol, ptol = host_case_tol(l64, tpl)
        good = AR.stand_in(*case, min_post)
        AR.check_align(good, l64, tpl, line_lex, lexicons, min_post, vtol, ptol, exact_logits=exact)
        for mut in AR.MUTANTS:
            bad = AR.stand_in(*case, min_post, mutant=mut)
            if all(np.array_equal(bad[k].view(np.uint8), good[k].view(np.uint8)) for k in good):
                continue   # this case's data cannot tell the mutant apart
            with pytest.raises(AssertionError):
                AR.check_align(bad, l64, tpl, line_lex, lexicons, min_post, vtol, ptol, exact_logits=exact)
            refused.add(mut)
    assert refused == set(AR.MUTANTS)


def test_stand_in_equals_the_host_entry_where_the_rule_is_exact():
    """adds and compares only: on the known answers (equal logits, exact) the stand-in and the host entry agree bit for bit in
    path, flags and Viterbi value"""
    case, _ = known_answer_case()
    out, good = run_host(case, [0.5] * 3), AR.stand_in(*case, [0.5] * 3)
    for key in ("idx", "snapped", "vit"):
        assert out[key].tobytes() == good[key].tobytes(), key


# ---------------------------------------------------------------- the GPU grid's inputs
@pytest.mark.parametrize("N", LR.GRID_N)
def test_grid_planted_lines_leave_a_path_margin(grid, N):
    """what makes the exact-path assertion of test_gpu_lexicon_align.py apply to the planted lines: the fp64 gap between the
    planted entry's best and second-best alignment is at least ten times VIT_TOL"""
    case, l64 = grid[N]
    z, W, b, tpl, line_lex, lexicons = case
    planted, o = 0, 0
    for T, k in zip(tpl, line_lex):
        e = max(lexicons[k - 1], key=len)
        if T >= LR.need(e):
            opt, path, second = AR.viterbi64(l64[o:o + T], e)
            assert opt - second >= 10 * AR.VIT_TOL, (N, T, k, opt - second)
            assert AR.collapse(path) == e
            planted += 1
        o += T
    assert planted >= 2 * len(lexicons)


def test_fp64_viterbi_against_enumeration():
    """the restatement itself: optimum and second-best value against every class path of a small line"""
    import itertools
    rng = np.random.default_rng(3)
    T, N = 5, 3
    l = rng.normal(0.0, 2.0, (T, N))
    for entry in ([1], [1, 1], [1, 2], [2, 1, 2], [1, 1, 2]):
        scores = sorted((sum(l[t, c] for t, c in enumerate(p)), p) for p in itertools.product(range(N), repeat=T)
                        if AR.collapse(p) == entry)
        opt, path, second = AR.viterbi64(l, entry)
        assert abs(opt - scores[-1][0]) <= 1e-12 and tuple(path) == scores[-1][1]
        assert abs(second - scores[-2][0]) <= 1e-12 if len(scores) > 1 else second == -np.inf
        assert AR.path_states(path, entry) is not None


# ---------------------------------------------------------------- the surface
NEW_INT = ("rt_lexicon_set_snap", "rt_results_rec_lexicon_snapped", "rt_debug_ctc_lexicon_align", "rt_debug_ctc_lexicon_align_host")


def test_exports_and_header_declarations():
    hdr = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    lib = _lib.load()
    for name in NEW_INT:
        assert "RT_API int %s(" % name in hdr
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "RT_API float rt_lexicon_snap(" in hdr and "rt_lexicon_snap" in _lib.EXPORTS and lib.rt_lexicon_snap.restype is C.c_float
    rule = open(os.path.join(ROOT, "retto_amd", "csrc", "ctc_lexicon_align.h")).read()
    for words in ("strictly greater", "Why the path exists", "Out of scope", "rt_rec and rt_ctc_decode", "per-region threshold"):
        assert words.lower() in rule.lower(), words
    assert "ctc_lexicon_align.h" in open(os.path.join(ROOT, "retto_amd", "csrc", "ctc_lexicon.h")).read()
    assert not any("snap" in f[0] for f in _lib.Config._fields_)   # (no rt_config field: test_lexicon_cpu.py pins the last one)


def test_session_calls_reject_a_null_session():
    lib = _lib.load()
    assert lib.rt_lexicon_set_snap(None, 1, 0.5) == 8
    assert b"rt_lexicon_set_snap: null session" in lib.rt_last_error(None)
    assert lib.rt_lexicon_snap(None, 1) == 0.0
    assert lib.rt_results_rec_lexicon_snapped(None, 0, 0) == 0
    case, _ = known_answer_case()
    rc, _ = AR.call(lib.rt_debug_ctc_lexicon_align, C.c_void_p(None), *case, [0.5] * 3, chunk=0)
    assert rc == 8 and b"rt_debug_ctc_lexicon_align: null session" in lib.rt_last_error(None)


@pytest.mark.parametrize("min_post,msg", [
    ([0.5, float("nan"), 0.5], rb"lex_min_post\[1\] = nan is outside \[0, 1\]"),
    ([1.5, 0.5, 0.5], rb"lex_min_post\[0\] = 1.5\d* is outside \[0, 1\]"),
    ([0.5, 0.5, -0.25], rb"lex_min_post\[2\] = -0.25\d* is outside \[0, 1\]"),
])
def test_threshold_errors_and_their_messages(min_post, msg):
    import re
    lib = _lib.load()
    case, _ = known_answer_case()
    rc, out = AR.call(lib.rt_debug_ctc_lexicon_align_host, None, *case, min_post)
    assert rc == 8 and re.search(msg, lib.rt_last_error(None)), lib.rt_last_error(None)
    assert (out["idx"] == AR.CANARY_IDX).all() and (out["snapped"] == AR.CANARY_IDX).all()   # nothing was written


def test_bad_arguments_are_rejected():
    lib = _lib.load()
    (z, W, b, tpl, line_lex, lexicons), _ = known_answer_case()
    f = lib.rt_debug_ctc_lexicon_align_host
    assert AR.call(f, None, z, W, b, tpl, [1, 4, 3], lexicons, [0.5] * 3)[0] == 8            # a lexicon index past n_lex
    assert AR.call(f, None, z, W, b, tpl, line_lex, [[[1, 5]]] * 3, [0.5] * 3)[0] == 8       # a class id outside [1, N)
    assert AR.call(f, None, z, W, b, [5, -1, 1], line_lex, lexicons, [0.5] * 3)[0] == 8
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = AR.new_outputs(tpl, line_lex, lexicons)
    ids, lens, first = LR.flat_lexicons(lexicons)
    tp, ll, mp = np.array(tpl, np.int32), np.array(line_lex, np.int32), np.full(3, 0.5, np.float32)
    base = [p(z), p(W), p(b), 5, p(tp), 3, p(ll), p(ids), p(lens), p(first), 3]
    tail = [p(out["table"]), p(out["matches"]), p(out["n"])]
    assert f(*base, p(mp), p(out["idx"]), p(out["prob"]), p(out["snapped"]), p(out["vit"]), *tail) == 0
    for hole in range(5):   # lex_min_post, idx, prob, snapped_out, vit_out: each is required
        mid = [p(mp), p(out["idx"]), p(out["prob"]), p(out["snapped"]), p(out["vit"])]
        mid[hole] = None
        assert f(*base, *mid, *tail) == 8 and b"a required pointer is null" in lib.rt_last_error(None)


def test_python_mirror_and_cli_flag(tmp_path):
    for name in ("set_lexicon_snap", "lexicon_snap"):
        assert callable(getattr(retto_amd.RettoSession, name))
    assert list(inspect.signature(retto_amd.RettoSession.set_lexicon_snap).parameters) == ["self", "lexicon", "min_posterior"]
    r = retto_amd.RecProcessorSingleResult("x", 1.0)
    assert r.lexicon_snapped is None and r.lexicon_matches is None
    fields = [f.name for f in __import__("dataclasses").fields(retto_amd.RecProcessorSingleResult)]
    assert fields.index("lexicon_snapped") == fields.index("lexicon_matches") + 1
    a = cli.build_parser().parse_args(["-i", "x", "--rec-lexicon", str(tmp_path / "w.txt"), "--rec-lexicon-snap", "0.9"])
    assert a.rec_lexicon_snap == 0.9
    assert cli.build_parser().parse_args(["-i", "x"]).rec_lexicon_snap is None
