"""Rec charsets (retto_amd/csrc/ctc_charset.h) without a GPU: what rt_charset_create compiles (rt_debug_charset_compile), the rule
in plain fp32 loops (rt_debug_ctc_charset_host) against the fp64 restatement in ctc_charset_ref.py, that restatement's checker
against the mutants it must refuse, and the surface: exports, header, Python mirror, CLI flag, an unchanged rt_config."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, cli, synth

import ctc_charset_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The logits are the sums test_candidates_cpu.py bounds (120 products of magnitude up to ~2.6: an accumulated rounding error of
# order 1e-5), and a softmax over a subset of the classes moves by at most p (1 - p) <= 1/4 of a logit error just as the full one
# does, plus a few ulp of expf and of a sum of at most 6625 terms: the same tolerance, 4 x the 5.0e-6 measured there.
TOL = 2e-5

# a small hand-written dictionary: ASCII, CJK, a duplicate ("A" twice), a two-code-point entry, a line that is only U+3000
SMALL = "A\nb\n7\n中\nA\nab\n　\n文\n".encode("utf-8")
SMALL_ENTRIES = ["blank", "A", "b", "7", "中", "A", "ab", "", "文", " "]


def members(mask, n):
    return CR.members(mask, n)


def test_small_dictionary_is_what_the_cases_assume():
    assert retto_amd.parse_dictionary(SMALL) == SMALL_ENTRIES


@pytest.mark.parametrize("text,ids,want", [
    ("", (), [0]),                       # the blank is always in
    ("b7", (), [0, 2, 3]),               # ASCII
    ("文中", (), [0, 4, 8]),             # CJK, in any order
    ("A", (), [0, 1, 5]),                # duplicate entries all join
    (" ", (), [0, 9]),                   # U+0020 selects the appended " " class
    ("b", (6,), [0, 2, 6]),              # a two-code-point entry is reachable through ids only
    ("", (0, 7, 7), [0, 7]),             # ids may name anything, the empty U+3000 line included; repeats are harmless
    ("AA文", (8, 1), [0, 1, 5, 8]),
])
def test_compile_rules_on_the_small_dictionary(text, ids, want):
    m = retto_amd.debug_charset_compile(SMALL, text, ids)
    assert m.dtype == np.uint32 and len(m) == 1
    assert members(m, len(SMALL_ENTRIES)) == want
    assert int(m[0]) >> len(SMALL_ENTRIES) == 0   # no bit past the classes


@pytest.mark.parametrize("text,ids,exc,msg", [
    ("a", (), retto_amd.InvalidArgument, r"U\+0061"),              # only "ab" holds an a: no whole entry
    ("A　", (), retto_amd.InvalidArgument, r"U\+3000"),        # the U+3000 line was trimmed to the empty entry
    ("\U0001F600", (), retto_amd.InvalidArgument, r"U\+1F600"),
    (b"A\xc3", (), retto_amd.Utf8Error, r"byte offset 1"),
    (b"\xed\xa0\x80", (), retto_amd.Utf8Error, r"byte offset 0"),  # a surrogate
    ("", (10,), retto_amd.InvalidArgument, r"class id 10 is outside \[0, 10\)"),
    ("", (-1,), retto_amd.InvalidArgument, r"class id -1"),
])
def test_compile_errors_and_their_messages(text, ids, exc, msg):
    with pytest.raises(exc, match=msg):
        retto_amd.debug_charset_compile(SMALL, text, ids)


def test_compile_on_the_synthetic_dictionary():
    dic = synth.synth_models(0)[3]
    ents = retto_amd.parse_dictionary(dic)
    n = len(ents)
    text = ents[1] + ents[n - 2] + ents[33] + " "
    m = retto_amd.debug_charset_compile(dic, text, [64, 6000])
    assert len(m) == CR.mask_words(n)
    want = sorted({0, 64, 6000, n - 1} | {c for c in range(1, n) if ents[c] in (ents[1], ents[n - 2], ents[33])})
    assert members(m, n) == want
    with pytest.raises(retto_amd.InvalidArgument, match=r"U\+0041 matches no dictionary entry"):
        retto_amd.debug_charset_compile(dic, "A")
    # the C entry with a mask buffer that is too small
    lib = _lib.load()
    ncls = C.c_int(); err = C.create_string_buffer(256); small = np.zeros(3, np.uint32)
    assert lib.rt_debug_charset_compile(dic, len(dic), b"", 0, None, 0, small.ctypes.data, 3, C.byref(ncls), err, 256) == 8
    assert ncls.value == n and b"words" in err.value


# ---------------------------------------------------------------- the reference refuses its mutants
def _exact_case():
    """all-zero features, N = 37 (three pad columns), negative biases with exact ties inside and outside the set"""
    N, T = 37, 8
    bias = -1.0 - (np.arange(N) % 5).astype(np.float32)      # -1 at 0, 5, 10 ...: tied maxima
    bias[7] = 3.0                                            # the global maximum, outside the set
    z, W, b = CR.zero_feature_case(N, bias, T)
    masks = np.stack([CR.mask_of([5, 10, 11, 30], N)])       # + the blank: 0, 5, 10, 30 tie at -1
    idx = np.full(T, 7, np.int32); prob = np.full(T, 0.5, np.float32)
    return z, W, b, idx, prob, [T], [1], masks


def _random_case():
    return CR.grid_case(37)


@pytest.mark.parametrize("K", [0, 5])
def test_stand_in_passes_and_every_mutant_is_refused(K):
    refused = set()
    for case in (_exact_case(), _random_case()):
        good = CR.stand_in(*case, K)
        CR.check_outputs(good, *case, K, TOL)
        for mut in CR.MUTANTS:
            bad = CR.stand_in(*case, K, mutant=mut)
            if all(np.array_equal(bad[k].view(np.uint8), good[k].view(np.uint8)) for k in good):
                continue   # this case's data cannot tell the mutant apart
            with pytest.raises(AssertionError):
                CR.check_outputs(bad, *case, K, TOL)
            refused.add(mut)
    assert refused == set(CR.MUTANTS)


# ---------------------------------------------------------------- the host rule against fp64
def run_host(case, K):
    rc, out = CR.call(_lib.load().rt_debug_ctc_charset_host, None, *case, K)
    assert rc == 0
    return out


@pytest.mark.parametrize("K", [0, 1, 5])
@pytest.mark.parametrize("N", [5, 37, 64, 65, 6625])
def test_host_rule_against_fp64(N, K):
    case = CR.grid_case(N)
    if N == 6625:   # (plain loops: 6625 x 120 multiplications per row)
        z, W, b, idx, prob, tpl, ls, masks = case
        case = (z[:81], W, b, idx[:81], prob[:81], [40, 1, 33, 7], [1, 3, 2, 0], masks)
    out = run_host(case, K)
    worst = CR.check_outputs(out, *case, K, TOL, (N, K))
    assert out["ntok"].sum() > 0
    print("worst |p - q| N=%d K=%d: %.3e" % (N, K, worst))


@pytest.mark.parametrize("N", [5, 37, 64, 65, 6625])
def test_grid_inputs_have_a_clear_winner_on_every_row(N):
    """what lets test_gpu_charset.py expect the fp64 argmax itself: the fp64 gap between the two best allowed logits"""
    z, W, b, idx, prob, tpl, ls, masks = CR.grid_case(N)
    assert CR.min_top2_gap(z, W, b, tpl, ls, masks) >= 6e-4


def test_exact_cases_on_the_host():
    case = _exact_case()
    out = run_host(case, 8)
    assert list(out["idx"]) == [0] * 8 and out["ntok"][0] == 0 and np.isnan(out["scores"][0])   # the tie goes to the lowest id
    CR.check_outputs(out, *case, 8, TOL)
    # a set whose members beat the blank: they tie among themselves, |S| = 4 < K = 8
    z, W, b, idx, prob, tpl, ls, _ = case
    b2 = b.copy(); b2[[5, 10, 30]] = 0.5
    masks = np.stack([CR.mask_of([5, 10, 30], 37)])
    out = run_host((z, W, b2, idx, prob, tpl, ls, masks), 8)
    assert list(out["idx"]) == [5] * 8 and list(out["tokens"][:1]) == [5] and out["ntok"][0] == 1
    assert list(out["cands"]["id"][0]) == [5, 10, 30, 0, -1, -1, -1, -1]
    assert list(out["cands"]["prob"][0][4:]) == [0.0] * 4
    # S = {blank}: no token, probability exactly 1 on every step
    out = run_host((z, W, b2, idx, prob, tpl, ls, np.zeros((1, 2), np.uint32)), 3)
    assert list(out["idx"]) == [0] * 8 and out["prob"].tobytes() == np.ones(8, np.float32).tobytes() and out["ntok"][0] == 0


def test_bad_arguments_are_rejected():
    case = list(CR.grid_case(5))
    lib = _lib.load()
    bad = list(case); bad[6] = [1, 4, 2, 0, 0, 3]   # a set index past n_sets
    assert CR.call(lib.rt_debug_ctc_charset_host, None, *bad, 2)[0] == 8
    assert CR.call(lib.rt_debug_ctc_charset_host, None, *case, 9)[0] == 8


# ---------------------------------------------------------------- the surface
NEW = ("rt_charset_create", "rt_charset_classes", "rt_set_rec_charset", "rt_run_regions_charsets", "rt_debug_charset_compile",
       "rt_debug_ctc_charset", "rt_debug_ctc_charset_host")


def test_exports_and_header_declarations():
    hdr = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert "RT_API int %s(" % name in hdr
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "#define RT_MAX_CHARSETS 64" in hdr and _lib.MAX_CHARSETS == 64
    rule = open(os.path.join(ROOT, "retto_amd", "csrc", "ctc_charset.h")).read()
    assert "MAX_SETS = 64" in rule


def test_rt_config_is_unchanged():
    """charsets are session objects: no rt_config field was added for them"""
    assert _lib.Config._fields_[-1][0] == "rec_return_word_box"
    assert [f[0] for f in _lib.Config._fields_[-3:]] == ["rec_return_candidates", "crop_source", "rec_return_word_box"]
    assert not any("charset" in f[0] for f in _lib.Config._fields_)
    hdr = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    struct = hdr[hdr.index("typedef struct rt_config"):hdr.index("} rt_config;")]
    assert "charset" not in struct
    assert re.findall(r"int32_t\s+(\w+);", struct)[-1] == "rec_return_word_box"
    c = _lib.Config(); _lib.load().rt_config_default(C.byref(c))
    assert c.struct_size == C.sizeof(_lib.Config)


def test_python_mirror_and_cli_flag():
    for name in ("create_charset", "set_rec_charset", "charset_classes", "run_regions", "run_regions_raw"):
        assert callable(getattr(retto_amd.RettoSession, name))
    import inspect
    assert "charsets" in inspect.signature(retto_amd.RettoSession.run_regions).parameters
    assert inspect.signature(retto_amd.RettoSession.run_regions).parameters["charsets"].default is None
    sig = inspect.signature(retto_amd.RettoSession.create_charset)
    assert sig.parameters["text"].default == "" and tuple(sig.parameters["ids"].default) == ()
    a = cli.build_parser().parse_args(["-i", "x", "--rec-charset", "0123456789"])
    assert a.rec_charset == "0123456789"
    assert cli.build_parser().parse_args(["-i", "x"]).rec_charset is None


def test_session_calls_reject_a_null_session():
    lib = _lib.load()
    out = C.c_int(5)
    assert lib.rt_charset_create(None, b"", 0, None, 0, C.byref(out)) == 8
    assert lib.rt_set_rec_charset(None, 0) == 8
    assert lib.rt_charset_classes(None, 1, None) == 0
