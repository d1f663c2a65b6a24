"""Rec lexicons (retto_amd/csrc/ctc_lexicon.h) without a GPU: what rt_lexicon_create compiles (rt_debug_lexicon_compile), the fp64
restatement in ctc_lexicon_ref.py against the definition by enumeration, the rule in plain fp32 loops
(rt_debug_ctc_lexicon_host) against that restatement, its checker against the mutants it must refuse, the margin the GPU grid's
inputs leave, and the surface: exports, header, Python mirror, CLI flag, an unchanged rt_config."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, cli, synth

import ctc_lexicon_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a small hand-written dictionary: ASCII, CJK, a duplicate ("A" twice), a two-code-point entry, a line that is only U+3000
SMALL = "A\nb\n7\n中\nA\nab\n　\n文\n".encode("utf-8")
SMALL_ENTRIES = ["blank", "A", "b", "7", "中", "A", "ab", "", "文", " "]


def host_tol(ref, tpl):
    """What plain fp32 loops may differ from fp64 by, from the number formats: the logits carry an error of order 1e-5 (120
    products of magnitude up to ~2.6: test_candidates_cpu.py), so each step's lp one of about 2e-5 plus half an ulp of |lp|;
    alpha then takes per step one rounding of the sum and a few ulp from logf / expf at its own magnitude M <= max |loglik|: at
    most 3 ulp32(M) + 3e-5 a step, over T steps, summed in the worst case.  The posterior moves by at most p (1 - p) <= 1/4 of
    (its entry's error + the LSE's), both within that bound: half of it."""
    big = max([float(np.abs(r[0][np.isfinite(r[0])]).max()) for r in ref if r is not None and np.isfinite(r[0]).any()] + [1.0])
    tol = max(tpl) * (3.0 * float(np.spacing(np.float32(big))) + 3e-5)
    return tol, 0.5 * tol


def test_small_dictionary_is_what_the_cases_assume():
    assert retto_amd.parse_dictionary(SMALL) == SMALL_ENTRIES


# ---------------------------------------------------------------- compile rules and errors
@pytest.mark.parametrize("entries,ids,want", [
    (["b7", "A"], (), [[2, 3], [1]]),                       # the lowest class id of a duplicate entry
    (["文中文"], (), [[8, 4, 8]]),
    (["A b"], (), [[1, 9, 2]]),                             # U+0020 is the appended " " class
    (["AA"], (), [[1, 1]]),                                 # equal neighbours are allowed
    (b"b\r\n\r\n  7 \n\nA", (), [[2], [3], [1]]),           # split and trimmed as dictionary lines; empty lines skipped
    ([], ([6, 7], [5]), [[6, 7], [5]]),                     # ids name anything but the blank, multi-code-point entries included
    (["7"], ([9, 9, 9],), [[3], [9, 9, 9]]),                # text entries first, then the id entries
    (["A" * 31], (), [[1] * 31]),
])
def test_compile_rules_on_the_small_dictionary(entries, ids, want):
    assert retto_amd.debug_lexicon_compile(SMALL, entries, ids) == want


@pytest.mark.parametrize("entries,ids,exc,msg", [
    (["A", "a"], (), retto_amd.InvalidArgument, r"U\+0061 in entry 1 matches no dictionary entry"),   # only "ab" holds an a
    (["\U0001F600"], (), retto_amd.InvalidArgument, r"U\+1F600 in entry 0"),
    (b"A\xc3", (), retto_amd.Utf8Error, r"byte offset 1"),
    (b"b\n\xed\xa0\x80", (), retto_amd.Utf8Error, r"byte offset 2"),            # a surrogate
    ([], ([0],), retto_amd.InvalidArgument, r"class id 0 in entry 0 is outside \[1, 10\)"),
    (["A"], ([3, 10],), retto_amd.InvalidArgument, r"class id 10 in entry 1"),
    ([], ([-1],), retto_amd.InvalidArgument, r"class id -1"),
    (["A" * 32], (), retto_amd.InvalidArgument, r"entry 0 has 32 tokens, more than RT_LEXICON_MAX_LEN \(31\)"),
    ([], ([1] * 32,), retto_amd.InvalidArgument, r"more than RT_LEXICON_MAX_LEN"),
    (["b"], ([],), retto_amd.InvalidArgument, r"entry 1 is empty"),
    ([], (), retto_amd.InvalidArgument, r"no entry"),
    (b"\n \n", (), retto_amd.InvalidArgument, r"no entry"),
    (b"A\n" * 65537, (), retto_amd.CapacityError, r"RT_LEXICON_MAX_ENTRIES \(65536\)"),
])
def test_compile_errors_and_their_messages(entries, ids, exc, msg):
    with pytest.raises(exc, match=msg):
        retto_amd.debug_lexicon_compile(SMALL, entries, ids)


def test_compile_on_the_synthetic_dictionary_and_the_caps_of_the_c_entry():
    dic = synth.synth_models(0)[3]
    ents = retto_amd.parse_dictionary(dic)
    n = len(ents)
    word = ents[40] + ents[n - 2] + " " + ents[40]
    first = lambda t: min(c for c in range(1, n) if ents[c] == t)
    assert retto_amd.debug_lexicon_compile(dic, [word], [[n - 1, 1]]) == [[first(ents[40]), first(ents[n - 2]), n - 1, first(ents[40])],
                                                                          [n - 1, 1]]
    assert len(retto_amd.debug_lexicon_compile(dic, b"\n".join([ents[50].encode()] * 65536))) == 65536   # the cap itself is fine
    lib = _lib.load()
    ni, ne, nc = C.c_int(), C.c_int(), C.c_int(); err = C.create_string_buffer(256)
    small = np.zeros(2, np.int32); lens = np.zeros(1, np.int32)
    raw = word.encode("utf-8")
    assert lib.rt_debug_lexicon_compile(dic, len(dic), raw, len(raw), None, None, 0, small.ctypes.data, 2, lens.ctypes.data, 1,
                                        C.byref(ni), C.byref(ne), C.byref(nc), err, 256) == 8
    assert (ni.value, ne.value, nc.value) == (4, 1, n) and b"4 ids" in err.value and not small.any()


# ---------------------------------------------------------------- the fp64 restatement against the definition
@pytest.mark.parametrize("N,T", [(3, 1), (3, 4), (4, 5), (3, 6), (4, 6)])
def test_fp64_forward_equals_the_enumeration(N, T):
    rng = np.random.default_rng(100 * N + T)
    lp = LR.logp64(rng.normal(0.0, 2.0, (T, N)))
    a, b = 1, 2
    entries = [[a], [a, a], [a, b, a], [b], [a, b], [b, b, a], [a, a, a], [N - 1, a, N - 1, a]]
    ll = LR.loglik64(lp, entries)
    for e, v in zip(entries, ll):
        want = LR.brute64(lp, e)
        assert np.isneginf(v) == (T < LR.need(e)) == np.isneginf(want), (e, v, want)
        if np.isfinite(want):
            assert abs(v - want) <= 1e-12 * max(1.0, abs(want)), (e, v, want)
    # every path collapses to exactly one sequence: over all of them (up to length T) the likelihoods sum to 1
    every = [list(e) for L in range(1, T + 1) for e in __import__("itertools").product(range(1, N), repeat=L)]
    total = np.logaddexp(LR._lse(LR.loglik64(lp, every)), lp[:, 0].sum())   # (+ the all-blank path: the empty sequence)
    assert abs(total) <= 1e-10


# ---------------------------------------------------------------- the host rule against fp64
def run_host(case, want_table=True):
    rc, out = LR.call(_lib.load().rt_debug_ctc_lexicon_host, None, *case, want_table=want_table)
    assert rc == 0
    return out


def _exact_case():
    """all-zero features, N = 5 (three pad columns), negative biases: every logit its bias bit for bit.  The lexicon has equal
    neighbours, an entry that does not fit, and entries given twice (exact ties)"""
    N, T = 5, 4
    z, W, b = LR.zero_feature_case(N, [-1.0, -0.5, -2.0, -0.5, -3.0], 2 * T + 2)
    lex = [[1, 1], [3], [1, 2, 2, 1], [1, 1], [3], [2, 1], [1, 3], [3], [1, 1, 1], [3, 1]]
    return z, W, b, [T, 2, T], [1, 0, 1], [lex]


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs and their fp64 reference, computed once"""
    out = {}
    for N in LR.GRID_N:
        case = LR.grid_case(N)
        out[N] = (case, LR.reference(*case))
    return out


@pytest.mark.parametrize("N", LR.GRID_N)
def test_host_rule_against_fp64(grid, N):
    case, ref = grid[N]
    z, W, b, tpl, line_lex, lexicons = case
    if N == 6625:   # (plain loops, 6625 x 120 multiplications per row: the three small lexicons' lines)
        keep = [i for i, k in enumerate(line_lex) if k <= 3]
        offs = np.concatenate([[0], np.cumsum(tpl)])
        z = np.concatenate([z[offs[i]:offs[i + 1]] for i in keep])
        tpl = [tpl[i] for i in keep]; line_lex = [line_lex[i] for i in keep]; ref = [ref[i] for i in keep]
        case = (z, W, b, tpl, line_lex, lexicons)
    out = run_host(case)
    tol, ptol = host_tol(ref, tpl)
    wl, wp = LR.check_outputs(out, ref, tpl, line_lex, lexicons, tol, ptol, N)
    assert out["n"].max() == LR.MATCHES or N == 6625
    print("host N=%d: worst |loglik - fp64| %.3e (tol %.3e), worst |posterior - fp64| %.3e" % (N, wl, tol, wp))


def test_exact_case_on_the_host():
    case = _exact_case()
    z, W, b, tpl, line_lex, lexicons = case
    ref = LR.reference(*case)
    out = run_host(case)
    tol, ptol = host_tol(ref, tpl)
    LR.check_outputs(out, ref, tpl, line_lex, lexicons, tol, ptol)
    assert out["n"].tolist() == [4, 0, 4]
    m = out["matches"][0]
    # classes 1 and 3 share a bias, so [1, 3] and [3, 1] tie bit for bit, and so do the copies of [3]: each tie comes out by index
    assert m["entry"].tolist() == [6, 9, 1, 4]
    assert m["loglik"][0].tobytes() == m["loglik"][1].tobytes() and m["loglik"][2].tobytes() == m["loglik"][3].tobytes()
    assert m["loglik"][1] > m["loglik"][2]
    table = LR.split_table(out["table"], line_lex, lexicons)[0]
    assert np.isneginf(table[2]) and np.isneginf(table[8]) and np.isfinite(table[[0, 1, 3, 4, 5, 6, 7, 9]]).all()
    # without the table the matches are the same
    out2 = run_host(case, want_table=False)
    assert out2["matches"].tobytes() == out["matches"].tobytes() and out2["n"].tolist() == out["n"].tolist()
    assert (out2["table"] == LR.CANARY_F).all()


def test_bad_arguments_are_rejected():
    lib = _lib.load()
    z, W, b, tpl, line_lex, lexicons = _exact_case()
    f = lib.rt_debug_ctc_lexicon_host
    assert LR.call(f, None, z, W, b, tpl, [1, 2, 1], lexicons)[0] == 8          # a lexicon index past n_lex
    assert LR.call(f, None, z, W, b, tpl, line_lex, [[[1, 5]]])[0] == 8         # a class id outside [1, N)
    assert LR.call(f, None, z, W, b, tpl, line_lex, [[[0]]])[0] == 8            # the blank
    assert LR.call(f, None, z, W, b, tpl, line_lex, [[[1] * 32]])[0] == 8       # longer than RT_LEXICON_MAX_LEN
    assert LR.call(f, None, z, W, b, tpl, line_lex, [[[1]]] * 17)[0] == 8       # more than RT_MAX_LEXICONS
    assert LR.call(f, None, z, W, b, [4, -1, 4], line_lex, lexicons)[0] == 8


# ---------------------------------------------------------------- the reference refuses its mutants
def _random_case():
    """N = 5 (pad columns), negative biases, short lines, entries with equal neighbours and one that does not fit"""
    rng = np.random.default_rng(5)
    N = 5
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = (-1.0 - rng.random(N)).astype(np.float32)
    tpl = [6, 3, 5]
    z = rng.normal(0.0, 0.7, (sum(tpl), LR.D)).astype(np.float32)
    lex = [[1, 1, 2], [2], [3, 4], [2, 2, 2, 2], [4, 4], [1, 2, 3], [2, 1]]
    return z, W, b, tpl, [1, 1, 0], [lex]


def test_stand_in_passes_and_every_mutant_is_refused():
    refused = set()
    for case in (_exact_case(), _random_case()):
        z, W, b, tpl, line_lex, lexicons = case
        ref = LR.reference(*case)
        tol, ptol = host_tol(ref, tpl)
        good = LR.stand_in(*case)
        LR.check_outputs(good, ref, tpl, line_lex, lexicons, tol, ptol)
        for mut in LR.MUTANTS:
            bad = LR.stand_in(*case, mutant=mut)
            if all(np.array_equal(bad[k].view(np.uint8), good[k].view(np.uint8)) for k in good):
                continue   # this case's data cannot tell the mutant apart
            with pytest.raises(AssertionError):
                LR.check_outputs(bad, ref, tpl, line_lex, lexicons, tol, ptol)
            refused.add(mut)
    assert refused == set(LR.MUTANTS)


# ---------------------------------------------------------------- the GPU grid's inputs
@pytest.mark.parametrize("N", LR.GRID_N)
def test_grid_inputs_leave_a_margin_on_every_line(grid, N):
    """what makes the GPU grid's winners meaningful: on every line the fp64 gap between the two best entries is at least ten
    times the tolerance test_gpu_lexicon.py ends up with; and the grid is what its docstring says"""
    case, ref = grid[N]
    z, W, b, tpl, line_lex, lexicons = case
    assert [len(lex) for lex in lexicons] == list(LR.GRID_COUNTS)
    assert sorted({len(e) for lex in lexicons for e in lex}) == list(LR.GRID_LENS)
    gaps = [LR.top2_gap(r[0]) for r in ref]
    assert min(gaps) >= 10 * LR.HOOK_TOL, (N, min(gaps))
    planted = infeasible = 0
    for (ll, post), T, k in zip(ref, tpl, line_lex):
        lex = lexicons[k - 1]
        e = max(range(len(lex)), key=lambda i: len(lex[i]))
        if T >= LR.need(lex[e]):
            planted += 1
            assert int(np.argmax(ll)) == e and post[e] > 0.99, (N, T, k)    # the planted entry wins
        else:
            infeasible += 1
            assert np.isneginf(ll[e])
    assert planted >= 2 * len(lexicons) and infeasible >= 2 * len(lexicons)


# ---------------------------------------------------------------- the surface
NEW = ("rt_lexicon_create", "rt_lexicon_entries", "rt_lexicon_entry", "rt_set_rec_lexicon", "rt_run_regions_lexicons",
       "rt_results_rec_lexicon", "rt_results_rec_lexicon_id", "rt_debug_lexicon_compile", "rt_debug_ctc_lexicon",
       "rt_debug_ctc_lexicon_host")


def test_exports_and_header_declarations():
    hdr = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert "RT_API int %s(" % name in hdr
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "RT_API const char* rt_lexicon_entry_text(" in hdr and "rt_lexicon_entry_text" in _lib.EXPORTS
    for name, v in (("RT_MAX_LEXICONS", 16), ("RT_LEXICON_MAX_ENTRIES", 65536), ("RT_LEXICON_MAX_LEN", 31), ("RT_LEXICON_MATCHES", 4)):
        assert "#define %s %d" % (name, v) in hdr
    assert (_lib.MAX_LEXICONS, _lib.LEXICON_MAX_ENTRIES, _lib.LEXICON_MAX_LEN, _lib.LEXICON_MATCHES) == (16, 65536, 31, 4)
    assert C.sizeof(_lib.LexiconMatch) == 12 == LR.MATCH.itemsize
    rule = open(os.path.join(ROOT, "retto_amd", "csrc", "ctc_lexicon.h")).read()
    assert "Out of scope" in rule and "Viterbi" in rule


def test_rt_config_is_unchanged():
    """lexicons are session objects: no rt_config field was added for them"""
    assert _lib.Config._fields_[-1][0] == "rec_return_word_box"
    assert not any("lexicon" in f[0] for f in _lib.Config._fields_)
    c = _lib.Config(); _lib.load().rt_config_default(C.byref(c))
    assert c.struct_size == C.sizeof(_lib.Config)


def test_python_mirror_and_cli_flag(tmp_path):
    for name in ("create_lexicon", "set_rec_lexicon", "lexicon_entries", "run_regions", "run_regions_raw"):
        assert callable(getattr(retto_amd.RettoSession, name))
    assert inspect.signature(retto_amd.RettoSession.run_regions).parameters["lexicons"].default is None
    assert inspect.signature(retto_amd.RettoSession.run_regions_raw).parameters["lexicons"].default is None
    r = retto_amd.RecProcessorSingleResult("x", 1.0)
    assert r.lexicon_matches is None
    a = cli.build_parser().parse_args(["-i", "x", "--rec-lexicon", str(tmp_path / "words.txt")])
    assert a.rec_lexicon == str(tmp_path / "words.txt")
    assert cli.build_parser().parse_args(["-i", "x"]).rec_lexicon is None


def test_session_calls_reject_a_null_session():
    lib = _lib.load()
    out = C.c_int(5)
    assert lib.rt_lexicon_create(None, b"A", 1, None, None, 0, C.byref(out)) == 8
    assert lib.rt_set_rec_lexicon(None, 0) == 8
    assert lib.rt_lexicon_entries(None, 1) == 0 and lib.rt_lexicon_entry(None, 1, 0, None) == 0
    assert lib.rt_lexicon_entry_text(None, 1, 0) is None
    assert lib.rt_results_rec_lexicon(None, 0, 0, None) == 0 and lib.rt_results_rec_lexicon_id(None, 0, 0) == 0
