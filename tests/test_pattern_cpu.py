"""Rec patterns (retto_amd/csrc/ctc_pattern.h) on the CPU: the text compiler through rt_debug_pattern_compile against Python's
re.fullmatch, the host rule through rt_debug_ctc_pattern_host against a brute force over every frame labelling and against known
answers, the shared checker (ctc_pattern_ref.check_pattern) against mutants it must refuse, and the pattern part of the rec tail
plan through a small native driver.  No GPU.

The language section's "a pattern that accepts nothing" has no test: every atom is a non-empty set and there is no intersection,
so no text of this language compiles to an empty language; the compiler's check stands behind the trim all the same."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_align_ref as AR
import ctc_lexicon_ref as LR
import ctc_pattern_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT7 = "a\nb\nc\na\nbc\n".encode()                       # blank, a, b, c, a again (4), the two-code-point "bc" (5), " " (6)
DICT5 = PR.DICT5                                          # N = 5, no duplicate: a = 1, b = 2, c = 3, " " = 4
DICT_DIGITS = "".join(ch + "\n" for ch in "0123456789-,.").encode()
PATTERNS7 = ["ab", "a|b", "a|bc", "(ab|cb)*", "[a-c]{2,3}", "a*", "a+", "a?b", "bb", "\\c{5}b?", "[^a]+", ".{2}", "(a|b)+c", "a{2,}",
             "a{0,2}b", "", "()|a", "(a?){3}b", "a{0}b", "[ab][bc]", "\\c{5}\\c{5}", "[\\c{5}c]*", "a b", "[^\\c{5} ]{1,2}", ".*c",
             "(a|b|c){3}"]
PATTERNS_DIGITS = ["\\d{2}-\\d", "[0-9]{1,2}(,[0-9]{2})*\\.\\d", "[\\d\\-]+", "\\.\\-", "[-0]{2}", "[0-]{2}"]
INVALID, UTF8, CAPACITY = 8, 5, 9


def compile_status(dict_bytes, raw):
    try:
        retto_amd.debug_pattern_compile(dict_bytes, raw)
    except retto_amd.RettoError as e:
        return e.code, str(e)
    return 0, ""


def walk(c, seq):
    q = 0
    for k in seq:
        q = int(c["delta"][q][c["group_of"][k]])
        if q < 0:
            return False
    return bool(c["accept"][q])


def need(seq):
    return max(1, len(seq) + sum(1 for a, b in zip(seq, seq[1:]) if a == b))


@pytest.mark.parametrize("dict_bytes,patterns,max_len", [(DICT7, PATTERNS7, 5), (DICT_DIGITS, PATTERNS_DIGITS, 4)], ids=["seven", "digits"])
def test_compiled_tables_accept_what_re_accepts(dict_bytes, patterns, max_len):
    entries = PR.entries_of(dict_bytes)
    N = len(entries)
    assert retto_amd.parse_dictionary(dict_bytes) == entries
    strings = [s for L in range(max_len + 1) for s in itertools.product(range(1, N), repeat=L)]
    for text in patterns:
        c = retto_amd.debug_pattern_compile(dict_bytes, text)
        pat = PR.Pattern(text, entries)
        S, G = c["S"], c["G"]
        assert c["classes"] == N and 1 <= S <= 64 and c["delta"].shape == (S, G) and c["group_of"][0] == 0
        assert (c["delta"][:, 0] == -1).all(), (text, "group 0 has an arc")
        best = None
        for s in strings:
            ok = pat.accepts(s)
            assert walk(c, s) == ok, (text, s)
            if ok:
                best = need(s) if best is None else min(best, need(s))
        assert c["min_steps"] == best == PR.min_steps64(pat), (text, c["min_steps"], best)
        live = c["accept"].astype(bool).copy()   # trimmed: every state reaches an accepting one
        for _ in range(S):
            for q in range(S):
                live[q] = live[q] or any(t >= 0 and live[t] for t in c["delta"][q])
        assert live.all(), text
        reach = {0}                               # ... and is reached from the start
        for _ in range(S):
            reach |= {int(t) for q in reach for t in c["delta"][q] if t >= 0}
        assert reach == set(range(S)), text
        # two classes share a group iff they are members of exactly the same atoms
        atoms = [tk[1] for tk in PR.tokens_of(text, entries) if tk[0] == "atom"]
        sig = [tuple(k in a for a in atoms) for k in range(N)]
        for a in range(1, N):
            for b in range(1, N):
                assert (c["group_of"][a] == c["group_of"][b]) == (sig[a] == sig[b]), (text, a, b)
            assert (c["group_of"][a] == 0) == (not any(sig[a])), (text, a)
        pairs = {(int(c["delta"][q][c["group_of"][k]]), k) for q in range(S) for k in range(1, N) if c["delta"][q][c["group_of"][k]] >= 0}
        assert c["P"] == len(pairs), text


ERRORS = [  # (dictionary, pattern bytes, status, what the message holds)
    (DICT7, b"\xff", UTF8, "byte offset 0"), (DICT7, b"a\xc3", UTF8, "byte offset 1"), (DICT7, b"a\xed\xa0\x80", UTF8, "byte offset 1"),
    (DICT7, b"ax", INVALID, "U+0078 matches no dictionary entry (byte offset 1)"),
    (DICT7, b"[a-z]", INVALID, "U+007A matches no dictionary entry (byte offset 3)"),
    (DICT7, b"\\d", INVALID, "U+0030"), (DICT7, "a中".encode(), INVALID, "U+4E2D matches no dictionary entry (byte offset 1)"),
    (DICT7, b"a[]", INVALID, "an empty set (byte offset 1)"), (DICT7, b"[^abc\\c{5} ]", INVALID, "an empty set (byte offset 0)"),
    (DICT7, b"b(a", INVALID, "syntax error: the group is not closed (byte offset 1)"), (DICT7, b"a)", INVALID, "syntax error: an unopened ) (byte offset 1)"),
    (DICT7, b"*a", INVALID, "syntax error: nothing to repeat (byte offset 0)"), (DICT7, b"a|+", INVALID, "nothing to repeat (byte offset 2)"),
    (DICT7, b"a**", INVALID, "no lazy or stacked repeats (byte offset 2)"), (DICT7, b"a*?", INVALID, "no lazy or stacked repeats (byte offset 2)"),
    (DICT7, b"a{2", INVALID, "the repeat is not closed (byte offset 1)"), (DICT7, b"a{3,2}", INVALID, "0 <= m <= n <= 64 (byte offset 1)"),
    (DICT7, b"a{65}", INVALID, "0 <= m <= n <= 64 (byte offset 1)"), (DICT7, b"a{,2}", INVALID, "a number is expected (byte offset 2)"),
    (DICT7, b"b[a", INVALID, "the set is not closed (byte offset 1)"), (DICT7, b"a\\", INVALID, "a backslash ends the pattern (byte offset 1)"),
    (DICT7, b"^a", INVALID, "an unescaped ^ (byte offset 0)"), (DICT7, b"a]", INVALID, "an unescaped ] (byte offset 1)"),
    (DICT7, b"a}", INVALID, "an unescaped } (byte offset 1)"), (DICT7, b"a\\q", INVALID, "U+0071 cannot be escaped (byte offset 1)"),
    (DICT7, b"[c-a]", INVALID, "is reversed (byte offset 1)"),
    (DICT7, b"a\\c{0}", INVALID, "\\c{0} is outside [1, 7) (byte offset 1)"), (DICT7, b"\\c{7}", INVALID, "\\c{7} is outside [1, 7) (byte offset 0)"),
    (DICT7, b"a" * 1025, INVALID, "more than RT_PATTERN_MAX_BYTES (1024) (byte offset 1024)"),
]


@pytest.mark.parametrize("i", range(len(ERRORS)), ids=[repr(e[1][:12]) for e in ERRORS])
def test_every_error_has_its_status_and_offset(i):
    dict_bytes, raw, status, msg = ERRORS[i]
    rc, text = compile_status(dict_bytes, raw)
    assert rc == status and msg in text and text.startswith("pattern: "), (rc, text)


def test_caps_exactly_at_and_one_past():
    assert compile_status(DICT7, b"a*" + b"|a*" * 340 + b"|a")[0] == 0           # 1024 bytes of text pass
    c = retto_amd.debug_pattern_compile(DICT7, "a{63}")                              # a chain of 64 states
    assert c["S"] == 64 and c["min_steps"] == 63
    rc, text = compile_status(DICT7, b"a{64}")
    assert rc == CAPACITY and "RT_PATTERN_MAX_STATES (64) states: reached 65" in text
    data, entries = PR.synthetic_dictionary(6625 + 2 - 2)
    assert len(entries) == 6625
    hi = chr(0x4E00 + 4094)                                                          # classes 1 .. 4095
    c = retto_amd.debug_pattern_compile(data, "[一-%s\\c{5000}]*" % hi)
    assert c["P"] == 4096 and c["S"] == 2 and c["G"] == 2 and c["min_steps"] == 1
    rc, text = compile_status(data, ("[一-%s\\c{5000}\\c{5001}]*" % hi).encode())
    assert rc == CAPACITY and "RT_PATTERN_MAX_PAIRS (4096)" in text and "reached 4097" in text and "use a charset" in text
    rc, text = compile_status(data, b".{8}")
    assert rc == CAPACITY and "RT_PATTERN_MAX_PAIRS" in text and "use a charset" in text
    rc, text = compile_status(DICT7, b"((((a{8}){8}){8}){8}){8}")
    assert rc == CAPACITY and "atoms" in text


# ---- the host rule ---------------------------------------------------------------------------------------------------------
def run_host(z, W, b, tpl, line_pat, compiled, **kw):
    rc, out = PR.call(_lib.load().rt_debug_ctc_pattern_host, None, z, W, b, tpl, line_pat, compiled, **kw)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


def test_host_rule_equals_the_brute_force():
    """eight patterns, T in 1, 2, 3, 5, 6 at N = 5 (`bb` at T = 2 is infeasible): the end value equals the best accepted
    labelling's, the collapse is that labelling's where it stands clear, and check_pattern holds"""
    entries = PR.entries_of(DICT5)
    texts = ["ab", "bb", "a|bc", "(ab|cb)*", "[ab]{2}", "a*", "[^a]+c?", "(a|b)+c"]
    pats = [PR.Pattern(t, entries) for t in texts]
    compiled = [retto_amd.debug_pattern_compile(DICT5, t) for t in texts]
    rng = np.random.default_rng(77)
    N = 5
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    tpl = [T for _ in texts for T in (1, 2, 3, 5, 6)]
    line_pat = [k + 1 for k in range(len(texts)) for _ in range(5)]
    z = rng.normal(0.0, 1.5, (sum(tpl), LR.D)).astype(np.float32)
    l64 = LR.logits64(z, W, b)
    out = run_host(z, W, b, tpl, line_pat, compiled)
    o = 0
    for i, (T, k) in enumerate(zip(tpl, line_pat)):
        vtol = AR.fmt_tol(T, 64.0)[0]
        bv, bc = PR.brute64(l64[o:o + T], pats[k - 1])
        assert int(out["matched"][i]) == (1 if bc is not None else 0), (texts[k - 1], T)
        if bc is not None:
            assert abs(float(out["vit"][i]) - bv) <= vtol, (texts[k - 1], T, float(out["vit"][i]), bv)
        o += T
    assert int(out["matched"][tpl.index(2) + 5]) == 0 and texts[1] == "bb"
    vtol, ptol = AR.fmt_tol(6, 64.0)
    _, _, _, n_matched, n_exact, n_unmatched = PR.check_pattern(out, l64, tpl, line_pat, pats, vtol, ptol, 8 * vtol)
    assert n_matched >= 30 and n_exact >= 20 and n_unmatched >= 3, (n_matched, n_exact, n_unmatched)


def test_known_answers_bit_for_bit():
    z, W, b, tpl, line_pat, compiled, pats, l64 = PR.known_case(retto_amd.debug_pattern_compile)
    out = run_host(z, W, b, tpl, line_pat, compiled)
    o = 0
    for i, (what, text, rows, want, matched) in enumerate(PR.KNOWN):
        T = tpl[i]
        assert int(out["matched"][i]) == matched, what
        if matched:
            assert out["idx"][o:o + T].tolist() == want, (what, out["idx"][o:o + T].tolist())
            assert out["vit"][i] == np.float32(sum(l64[o + t, want[t]] for t in range(T))), what
        else:
            assert (out["idx"][o:o + T] == PR.CANARY_IDX).all() and out["vit"][i] == -np.inf, what
        o += T
    vtol, ptol = AR.fmt_tol(5, 8.0)
    PR.check_pattern(out, l64, tpl, line_pat, pats, vtol, ptol, 8 * vtol, exact_logits=True)


# ---- the checker against mutants -------------------------------------------------------------------------------------------
def test_check_pattern_refuses_every_mutant():
    """the known-answer lines (exact logits: the fp64 recursion is the rule) and, between them, two lines without a pattern; the
    correct stand-in passes, each mutant fails"""
    z, W, b, tpl, line_pat, compiled, pats, l64 = PR.known_case(retto_amd.debug_pattern_compile)
    line_pat = list(line_pat)
    line_pat[2] = 0; line_pat[7] = 0
    vtol, ptol = AR.fmt_tol(5, 8.0)
    good = PR.stand_in(z, W, b, tpl, line_pat, pats)
    PR.check_pattern(good, l64, tpl, line_pat, pats, vtol, ptol, 8 * vtol, exact_logits=True)
    host = run_host(z, W, b, tpl, line_pat, compiled)
    for key in ("idx", "matched", "vit"):
        assert host[key].tobytes() == good[key].tobytes(), key
    for mutant in PR.MUTANTS:
        bad = PR.stand_in(z, W, b, tpl, line_pat, pats, mutant=mutant)
        with pytest.raises(AssertionError):
            PR.check_pattern(bad, l64, tpl, line_pat, pats, vtol, ptol, 8 * vtol, exact_logits=True)
    assert len(PR.MUTANTS) == 7


def test_lines_without_a_pattern_keep_their_rows():
    z, W, b, tpl, line_pat, compiled, pats, l64 = PR.known_case(retto_amd.debug_pattern_compile)
    rng = np.random.default_rng(3)
    idx0 = rng.integers(0, 5, sum(tpl)).astype(np.int32); prob0 = rng.random(sum(tpl)).astype(np.float32)
    line_pat = [k if i % 2 else 0 for i, k in enumerate(line_pat)]
    out = run_host(z, W, b, tpl, line_pat, compiled, idx0=idx0, prob0=prob0)
    vtol, ptol = AR.fmt_tol(5, 8.0)
    PR.check_pattern(out, l64, tpl, line_pat, pats, vtol, ptol, 8 * vtol, idx0=idx0, prob0=prob0, exact_logits=True)


def test_bad_arguments_are_rejected():
    lib = _lib.load()
    z, W, b, tpl, line_pat, compiled, pats, l64 = PR.known_case(retto_amd.debug_pattern_compile)
    f = lib.rt_debug_ctc_pattern_host
    bad = dict(compiled[0]); bad["delta"] = compiled[0]["delta"].copy(); bad["delta"][0, 1] = 9
    grp = dict(compiled[0]); grp["group_of"] = compiled[0]["group_of"].copy(); grp["group_of"][0] = 1
    for lp, comp, msg in (([2] + [0] * (len(tpl) - 1), compiled[:1], b"line 0 names pattern 2, outside [0, 1]"),
                          ([1] + [0] * (len(tpl) - 1), [bad], b"pattern 1: delta[0][1] is outside [-1, S)"),
                          ([1] + [0] * (len(tpl) - 1), [grp], b"pattern 1: the blank is not in group 0")):
        assert PR.call(f, None, z, W, b, tpl, lp, comp)[0] == 8
        assert msg in lib.rt_last_error(None), lib.rt_last_error(None)


# ---- the plan --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pattern_plan") / "pattern_plan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "retto_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "pattern_plan_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the pattern plan driver does not build:\n" + r.stderr[-3000:]
    return exe


def test_plan_lists_the_pattern_lines(plan_exe):
    """lines of 2, 1, 3, 65, 4 steps, the group [1, 4); pattern 1 has S = 11, P = 100, pattern 2 is at the caps: a line's codes
    count towards the scratch buffer only when T * (P + S) exceeds the 8192 the kernel keeps in LDS"""
    T = "5 2 1 3 65 4"
    pats = "2 11 100 64 4096"
    queries = ["1 4 0 %s %s 0" % (T, pats), "1 4 0 %s %s 1 0 0 0 0 0" % (T, pats), "1 4 0 %s %s 1 1 0 0 0 2" % (T, pats),
               "1 4 0 %s %s 1 0 1 2 1 0" % (T, pats), "0 5 0 %s %s 1 2 0 0 1 1" % (T, pats), "1 4 0 5 2 1 3 74 4 %s 1 0 0 0 1 0" % pats]
    r = subprocess.run([plan_exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    none = "rows=69 z5=0 has_pat=0 max_P=0 max_S=0 bp_codes=0 plines=- prows=-"
    assert r.stdout.splitlines() == [
        none, none, none,
        "rows=69 z5=1 has_pat=1 max_P=4096 max_S=64 bp_codes=12480 plines=0:1:0:1:0,1:3:1:2:0,4:65:0:3:12480 prows=" +
        ",".join(str(v) for v in range(69)),
        "rows=75 z5=1 has_pat=1 max_P=4096 max_S=64 bp_codes=8320 plines=0:2:1:0:0,2:65:0:3:8320,67:4:0:4:8320 prows=0,1," +
        ",".join(str(v) for v in range(6, 75)),
        "rows=78 z5=1 has_pat=1 max_P=100 max_S=11 bp_codes=8214 plines=0:74:0:3:0 prows=" + ",".join(str(v) for v in range(4, 78)),
    ]
