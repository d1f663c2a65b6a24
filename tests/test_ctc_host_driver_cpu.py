"""The host references of the rec CTC tail (retto_amd/csrc/ctc_host_ref.h) under AddressSanitizer + UBSan: a stand-alone driver
(tests/native/ctc_host_driver.cpp, run as a program; nothing is loaded into Python under a sanitizer) runs each kind's check and
reference on the inputs the library's rt_debug_ctc_*_host entry gets, and the two outputs must be the same bytes, with the
driver's exit code 0 and its stderr empty.  The cases are the smallest at which a reference can go wrong: N = 9 classes, lines
of 0, 1, 2, 7 and 40 time steps (an empty line, a one-step line, a line longer than any entry), one line without an option, two
lists / sets / patterns with the lines split between them.  Refused calls: one per shared piece of the checks and kind; where the
kind's check speaks, rt_last_error(NULL) is the entry's name before the driver's message (candidates and charsets only answer
yes or no: there both must refuse).  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_pattern_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 8
D, N = 120, 9
TPL = [0, 1, 2, 7, 40]
KIND = dict(candidates=0, charset=1, lexicon=2, pattern=3, keywords=4, beam=5)
MATCHES, HITS = 4, 8                      # RT_LEXICON_MATCHES, RT_KEYWORD_HITS
CAND_W, MATCH_W, HIT_W, BEAM_W = 2, 3, 12, 2   # 32-bit words of rt_candidate, rt_lexicon_match, rt_keyword_hit, rt_beam
I32, F32 = np.int32, np.float32


def i32(v):
    return np.ascontiguousarray(v, I32)


def f32(v):
    return np.ascontiguousarray(v, F32)


def head(tpl, seed=0):
    """z5, W, bias of a fixed seed; logits of a few units' spread, far from any overflow"""
    rng = np.random.default_rng(1234 + seed)
    rows = sum(max(t, 0) for t in tpl)
    return (f32(rng.standard_normal((rows, D))), f32(0.3 * rng.standard_normal((D, N))), f32(0.5 * rng.standard_normal(N)))


def decoded(z, W, b):
    """the decode's (idx, prob) of every row, as the net's fused argmax hands them on (any class and probability would do)"""
    l = z.astype(np.float64) @ W.astype(np.float64) + b
    p = np.exp(l - l.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    return i32(l.argmax(1)), f32(p.max(1))


class Case:
    """inputs: the driver's arrays behind params, in its order; outs: (dtype, words, initial values or None) in the order of the
    host entry's signature; args(outs): the library entry's arguments"""

    def __init__(self, kind, fn, tpl, params, inputs, outs, args):
        self.kind, self.fn, self.tpl, self.params, self.inputs, self.outs, self.args = kind, fn, i32(tpl), i32(params), inputs, outs, args

    def file_bytes(self):
        b = struct.pack("<3i", KIND[self.kind], N, len(self.tpl)) + self.tpl.tobytes() + struct.pack("<i", 1 + len(self.inputs))
        for a in [self.params] + list(self.inputs):
            b += struct.pack("<i", -1) if a is None else struct.pack("<i", a.size) + a.tobytes()
        return b

    def library(self):
        """(rc, the outputs serialised as the driver writes them)"""
        outs = [np.zeros(max(w, 0), t) if init is None else np.array(init, t) for t, w, init in self.outs]
        for o, (t, w, init) in zip(outs, self.outs):
            assert o.size == w and o.itemsize == 4
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = getattr(_lib.load(), self.fn)(*[p(a) if isinstance(a, np.ndarray) or a is None else a for a in self.args(outs)])
        return rc, struct.pack("<i", 0) + b"".join(struct.pack("<i", o.size) + o.tobytes() for o in outs)


def rows_of(tpl):
    return sum(max(t, 0) for t in tpl)


def candidates(K, tpl=TPL, idx=None):
    z, W, b = head(tpl)
    i0, p0 = decoded(z, W, b)
    i0 = i0 if idx is None else i32(idx)
    rows, n = rows_of(tpl), len(tpl)
    t = i32(tpl)
    return Case("candidates", "rt_debug_ctc_candidates_host", tpl, [K], [z, W, b, i0, p0],
                [(I32, rows * K * CAND_W, None), (I32, rows, None), (I32, n, None)],
                lambda o: [z, W, b, N, i0, p0, t, n, K, o[0], o[1], o[2]])


def charset(K, tpl=TPL, line_set=(1, 2, 0, 1, 2), idx=None, blank_rows=()):
    z, W, b = head(tpl, 1)
    i0, p0 = decoded(z, W, b)
    i0 = i0 if idx is None else i32(idx)
    i0[list(blank_rows)] = 0
    rows, n = rows_of(tpl), len(tpl)
    t, ls = i32(tpl), i32(line_set)
    masks = np.array([0b000001110, 0b111110000], np.uint32)   # set 1: classes 1-3, set 2: classes 4-8 (one word a set at N = 9)
    return Case("charset", "rt_debug_ctc_charset_host", tpl, [K, 2], [z, W, b, i0, p0, ls, masks.view(I32)],
                [(I32, rows, i0), (F32, rows, p0), (I32, rows, None), (I32, n, None), (F32, n, None),
                 (I32, rows * K * CAND_W, None), (I32, rows if K > 0 else 0, None)],
                lambda o: [z, W, b, N, o[0], o[1], t, n, ls, masks, 2, K, o[2], o[3], o[4], o[5] if K > 0 else None, o[6] if K > 0 else None])


# two lists: list 1 = entries 0-2, list 2 = entries 3-4; no entry is longer than 3 ids
ENTRIES = ([1, 2], [3], [1, 1, 4], [5, 6, 7], [8, 2])
FIRST = (0, 3, 5)
LINE_LIST = (1, 2, 0, 1, 2)


def lists_of(entries, first):
    return i32([c for e in entries for c in e]), i32([len(e) for e in entries]), i32(first)


def table_of(line_list, first):
    return sum(first[k] - first[k - 1] for k in line_list if 0 < k < len(first))


def lexicon(min_post=None, tpl=TPL, line_lex=LINE_LIST, entries=ENTRIES, first=FIRST):
    z, W, b = head(tpl, 2)
    ids, lens, fe = lists_of(entries, first)
    rows, n, table = rows_of(tpl), len(tpl), table_of(line_lex, first)
    t, ll = i32(tpl), i32(line_lex)
    tail = [(F32, table, None), (I32, n * MATCHES * MATCH_W, None), (I32, n, None)]
    if min_post is None:
        return Case("lexicon", "rt_debug_ctc_lexicon_host", tpl, [2, 0], [z, W, b, ll, ids, lens, fe], tail,
                    lambda o: [z, W, b, N, t, n, ll, ids, lens, fe, 2, o[0], o[1], o[2]])
    i0, p0 = decoded(z, W, b)
    mp = f32(min_post)
    return Case("lexicon", "rt_debug_ctc_lexicon_align_host", tpl, [2, 1], [z, W, b, ll, ids, lens, fe, mp, i0, p0],
                [(I32, rows, i0), (F32, rows, p0), (I32, n, None), (F32, n, None)] + tail,
                lambda o: [z, W, b, N, t, n, ll, ids, lens, fe, 2, mp, o[0], o[1], o[2], o[3], o[4], o[5], o[6]])


def keywords(min_score=(-np.inf, 0.0), tpl=TPL, line_kw=LINE_LIST, entries=ENTRIES, first=FIRST):
    z, W, b = head(tpl, 3)
    ids, lens, fe = lists_of(entries, first)
    n, table = len(tpl), table_of(line_kw, first)
    t, lk, ms = i32(tpl), i32(line_kw), f32(min_score)
    return Case("keywords", "rt_debug_ctc_keywords_host", tpl, [2], [z, W, b, lk, ids, lens, fe, ms],
                [(F32, table, None), (I32, 2 * table, None), (I32, n * HITS * HIT_W, None), (I32, n, None)],
                lambda o: [z, W, b, N, t, n, lk, ids, lens, fe, 2, ms, o[0], o[1], o[2], o[3]])


def beam(B, nbest, tpl=TPL):
    z, W, b = head(tpl, 4)
    rows, n = rows_of(tpl), len(tpl)
    t = i32(tpl)
    return Case("beam", "rt_debug_ctc_beam_host", tpl, [B, nbest], [z, W, b],
                [(I32, n, None), (I32, n * nbest * BEAM_W, None), (I32, rows * nbest, None)],
                lambda o: [z, W, b, N, t, n, B, nbest, o[0], o[1], o[2]])


DICT9 = "a\nb\nc\nd\ne\nf\ng\n".encode()   # N = 9: the blank, a-g = 1-7, " " = 8
PATTERNS = ("[a-g ]*", "a{3}")             # the second needs 5 time steps (a, blank, a, blank, a)
LINE_PAT = (1, 2, 0, 1, 2)                  # the one-step line carries the pattern it cannot match, the 40-step line too and can


def pattern(tpl=TPL, line_pat=LINE_PAT):
    z, W, b = head(tpl, 5)
    compiled = [retto_amd.debug_pattern_compile(DICT9, t) for t in PATTERNS]
    assert compiled[0]["group_of"].size == N and compiled[1]["min_steps"] == 5
    S, G, group_of, delta, accept = PR.flat_tables(compiled)
    i0, p0 = decoded(z, W, b)
    rows, n = rows_of(tpl), len(tpl)
    t, lp = i32(tpl), i32(line_pat)
    return Case("pattern", "rt_debug_ctc_pattern_host", tpl, [2], [z, W, b, lp, S, G, group_of.ravel(), delta, accept, i0, p0],
                [(I32, rows, i0), (F32, rows, p0), (I32, n, None), (F32, n, None), (F32, n, None), (F32, n, None)],
                lambda o: [z, W, b, N, t, n, lp, S, G, group_of, delta, accept, 2, o[0], o[1], o[2], o[3], o[4], o[5]])


# ---- the stand-alone driver under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ctc_host") / "ctc_host_driver")
    src = os.path.join(ROOT, "tests", "native", "ctc_host_driver.cpp")
    includes = [l.strip() for l in open(src) if l.startswith("#include \"")]
    assert includes == ['#include "ctc_host_ref.h"'], includes   # the header stands alone: no HIP header, nothing else of the project
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the CTC host driver does not build:\n" + r.stderr[-3000:]
    return exe


def run_driver(driver, case, tmp_path):
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(case.file_bytes())
    r = subprocess.run([driver, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    return open(fout, "rb").read()


def words(blob, dtype=I32):
    """the arrays of a driver output"""
    out, o = [], 4
    while o < len(blob):
        n = struct.unpack_from("<i", blob, o)[0]
        out.append(np.frombuffer(blob, dtype, n, o + 4)); o += 4 + 4 * n
    return out


CASES = {
    "candidates K=1": lambda: candidates(1), "candidates K=3": lambda: candidates(3),
    "charset K=0": lambda: charset(0), "charset K=3": lambda: charset(3),
    "charset K=1, the unrestricted line all blank": lambda: charset(1, blank_rows=(1, 2)),   # (its score: 0 / 0)
    "lexicon": lambda: lexicon(), "lexicon snap, thresholds 0 and 1e-30": lambda: lexicon([0.0, 1e-30]),
    "keywords, min_score -inf and 0": lambda: keywords(),
    "beam (4, 2)": lambda: beam(4, 2), "beam off": lambda: beam(0, 0),
    "pattern": lambda: pattern(),
}


@pytest.mark.parametrize("name", list(CASES))
def test_driver_and_library_write_the_same_bytes(driver, tmp_path, name):
    case = CASES[name]()
    rc, want = case.library()
    assert rc == 0, _lib.load().rt_last_error(None)
    got = run_driver(driver, case, tmp_path)
    assert got == want, name
    a = words(got)
    # the cases reach what they are there for
    if case.kind == "candidates":
        assert a[2].sum() > 0                                   # some token is kept
    if "all blank" in name:
        assert a[3][2] == 0 and np.isnan(a[4].view(F32)[[0, 2]]).all()
    if case.kind == "charset":
        assert a[3][3:].min() > 0 and (a[0] != case.inputs[3]).any()   # the long lines keep tokens; a restricted row changed its class
    if case.fn == "rt_debug_ctc_lexicon_host":
        assert list(a[2][[0, 2]]) == [0, 0] and a[2][[3, 4]].min() >= 1   # no match on the empty line and the one without a lexicon
    if case.fn == "rt_debug_ctc_lexicon_align_host":
        assert a[2][[0, 3]].max() == 0 and a[2][[1, 4]].max() == 1        # threshold 0 never snaps; 1e-30 fires
    if case.kind == "keywords":
        assert a[3][2] == 0 and a[3].max() >= 1
    if name == "beam (4, 2)":
        assert a[0][0] <= 1 and a[0][3:].min() == 2
    if name == "beam off":
        assert not any(x.any() for x in a)
    if case.kind == "pattern":
        assert list(a[2]) == [0, 0, 0, 1, 1]   # (a line without a time step matches nothing; one step cannot hold a{3}, forty can)


NEG = [0, 1, 2, -1, 40]
BAD_IDX = [0] * 10 + [N] + [0] * 39
REFUSED = {
    # the line loop: a negative line length
    "candidates, negative line": lambda: candidates(2, tpl=NEG), "charset, negative line": lambda: charset(2, tpl=NEG),
    "lexicon, negative line": lambda: lexicon(tpl=NEG), "lexicon snap, negative line": lambda: lexicon([0.0, 0.5], tpl=NEG),
    "pattern, negative line": lambda: pattern(tpl=NEG), "keywords, negative line": lambda: keywords(tpl=NEG),
    "beam, negative line": lambda: beam(4, 2, tpl=NEG),
    # the line loop: an id past its bound
    "charset, set 3 of 2": lambda: charset(2, line_set=(1, 2, 0, 3, 2)), "lexicon, lexicon 3 of 2": lambda: lexicon(line_lex=(1, 2, 0, 3, 2)),
    "pattern, pattern 3 of 2": lambda: pattern(line_pat=(1, 2, 0, 3, 2)), "keywords, list 3 of 2": lambda: keywords(line_kw=(1, 2, 0, 3, 2)),
    # the entry lists: an entry of length 0, a class id equal to N, first_entry[0] = 1
    "lexicon, empty entry": lambda: lexicon(entries=([1, 2], [], [1, 1, 4], [5, 6, 7], [8, 2])),
    "keywords, empty entry": lambda: keywords(entries=([1, 2], [], [1, 1, 4], [5, 6, 7], [8, 2])),
    "lexicon, class N": lambda: lexicon(entries=([1, 2], [3], [1, N, 4], [5, 6, 7], [8, 2])),
    "keywords, class N": lambda: keywords(entries=([1, 2], [3], [1, N, 4], [5, 6, 7], [8, 2])),
    "lexicon, first_entry[0] = 1": lambda: lexicon(first=(1, 3, 5)), "keywords, first_entry[0] = 1": lambda: keywords(first=(1, 3, 5)),
    # the idx row scan
    "candidates, idx = N": lambda: candidates(2, idx=BAD_IDX), "charset, idx = N": lambda: charset(2, idx=BAD_IDX),
}
WORDS = {"negative line": "negative number of time steps", "3 of 2": "outside [0, 2]", "empty entry": "entry 1 has 0 ids",
         "class N": "class id 9 in entry 2", "first_entry[0] = 1": "_first_entry[0] must be 0"}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_calls_carry_the_drivers_message(driver, tmp_path, name):
    case = REFUSED[name]()
    lib = _lib.load()
    rc, _ = case.library()
    assert rc == INVALID, name
    got = run_driver(driver, case, tmp_path)
    assert struct.unpack_from("<i", got)[0] == 1, name
    msg = got[4:]
    if case.kind in ("candidates", "charset"):   # (a yes-or-no check: the host entry sets no message)
        assert msg == b"bad argument"
        return
    assert lib.rt_last_error(None) == case.fn.encode() + b": " + msg, (lib.rt_last_error(None), msg)
    want = [w for k, w in WORDS.items() if name.endswith(k)]
    assert len(want) == 1 and want[0] in msg.decode(), msg
