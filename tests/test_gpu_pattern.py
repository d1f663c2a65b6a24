"""Rec patterns (retto_amd/csrc/ctc_pattern.h) on the MI355X: the device path (row gather, the CTC FC, k_ctc_row_lse,
k_ctc_row_max, k_ctc_pattern_viterbi) through rt_debug_ctc_pattern against the fp64 restatement in ctc_pattern_ref.py.  The checks
are margin-free and leave no line out (ctc_pattern_ref.check_pattern).  Tolerances are the project's own: AR.VIT_TOL for lines of
up to 40 steps, AR.VIT_TOL_LONG for the long lines, AR.PROB_TOL, and LR.HOOK_TOL for logprob and free_logprob.

Measured on an MI355X over the grid of test_device_rule_against_fp64 (default chunking): the worst Viterbi deviation (the larger
of |vit_out - fp64 score of the returned path| and fp64 optimum - that score) is 1.031e-4 (N = 65; 8.653e-5 at N = 5, 9.026e-5 at
N = 6625), the worst |prob - fp64 softmax| 1.894e-6 (N = 6625) and the worst logprob / free_logprob deviation 1.851e-4 (N = 5).
On the long lines: 3.953e-4, 6.63e-7 and 1.463e-3, the last against PR.LOGPROB_TOL_LONG (ctc_pattern_ref.py says why).

The kernel has two staging boundaries, and both are crossed here:
  * a line's backpointer codes stay in LDS while T * (P + S) <= 8192 (pt::BP_LDS) and go through the scratch buffer beyond:
    test_long_lines_on_both_sides_of_the_lds_boundary, and in the grid every 40-step line of a pattern with P + S > 204;
  * a pattern's predecessor lists stay in LDS up to 2048 bytes (PREDS_LDS in prepost_kernels.hip): the grid's 60-way starred alternation has 3660."""
import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_align_ref as AR
import ctc_lexicon_ref as LR
import ctc_pattern_ref as PR

pytestmark = pytest.mark.gpu

KEYS = ("idx", "prob", "matched", "vit", "logprob", "free")
GRID_N = (5, 65, 6625)


def run_dev(sess, case, compiled, chunk=0, **kw):
    lib = _lib.load()
    rc, out = PR.call(lib.rt_debug_ctc_pattern, sess._hd.h, *case, compiled, chunk=chunk, **kw)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case, compiled, **kw):
    rc, out = PR.call(_lib.load().rt_debug_ctc_pattern_host, None, *case, compiled, **kw)
    assert rc == 0
    return out


def ch(c):
    """class c >= 1 of a synthetic dictionary as its character"""
    return chr(0x4E00 + c - 1)


def grid_patterns(N):
    """the grid's patterns over PR.synthetic_dictionary(N): (what, text)"""
    k = min(N - 2, 9)                       # the "digits": classes 1 .. k
    digits = "[%s-%s]" % (ch(1), ch(k))
    out = [("a fixed string with an equal neighbour", ch(1) + ch(2) + ch(3) + ch(2) + ch(2)),
           ("a digit-group format with a separator", "%s{2}%s%s{2}" % (digits, ch(N - 2), digits) if N > 5 else "[%s%s]{2}%s[%s%s]" % (ch(1), ch(2), ch(3), ch(1), ch(2))),
           ("an alternation of different lengths", "%s%s|%s%s%s%s" % (ch(1), ch(2), ch(3), ch(1), ch(2), ch(3))),
           ("a starred group with two arcs merging into one state", "((%s|%s)%s)*" % (ch(1), ch(3), ch(2))),
           ("a starred set", "%s*" % digits),
           ("a single-class group", "\\c{2}+"),
           ("exactly 64 states", "(\\c{1}\\c{2}){31}\\c{1}")]
    if N >= 65:
        out.append(("predecessor lists past the LDS copy", "(" + "|".join("\\c{%d}" % c for c in range(1, 61)) + ")*"))
    if N == 6625:
        out.append(("exactly 4096 pairs", "[%s-%s\\c{5000}]*" % (ch(1), ch(4095))))
    return out


def sample_string(auto, rng, steps):
    """a string the DFA accepts: up to `steps` random arcs, then the shortest way to an accepting state"""
    q, s = 0, []
    for _ in range(steps):
        arcs = np.nonzero(auto.src == q)[0]
        if len(arcs) == 0:
            break
        a = int(rng.choice(arcs))
        s.append(int(auto.cls[a])); q = int(auto.dst[a])
    seen, todo = {q: []}, [q]
    while todo:
        u = todo.pop(0)
        if auto.accept[u]:
            return s + seen[u]
        for a in np.nonzero(auto.src == u)[0]:
            v = int(auto.dst[a])
            if v not in seen:
                seen[v] = seen[u] + [int(auto.cls[a])]; todo.append(v)
    raise AssertionError("no accepting state is reachable")


def grid_case(N):
    """per pattern lines of T = 1, min_steps - 1 (infeasible), min_steps and 40 steps, an accepted string planted where it fits
    (features from LR.planted_features with the generator and gain of LR.grid_case), and a line without a pattern after every
    third pattern line"""
    rng = np.random.default_rng(9100 + N)
    data, entries = PR.synthetic_dictionary(N)
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    texts = [t for _, t in grid_patterns(N)]
    pats = [PR.Pattern(t, entries) for t in texts]
    compiled = [retto_amd.debug_pattern_compile(data, t) for t in texts]
    tpl, line_pat, paths = [], [], []
    for k, (pat, c) in enumerate(zip(pats, compiled)):
        ms = c["min_steps"]
        for T in sorted({1, ms - 1, ms, 40}):
            s = sample_string(pat.auto, rng, 12)
            if LR.need(s) > T:
                s = sample_string(pat.auto, rng, 0)
            tpl.append(T); line_pat.append(k + 1)
            paths.append((T, LR.alignment(s, T) if s and LR.need(s) <= T else None))
            if len(tpl) % 4 == 3:
                tpl.append(7); line_pat.append(0); paths.append((7, None))
    z = LR.planted_features(rng, W.astype(np.float64), paths)
    return (z, W, b, tpl, line_pat), compiled, pats


@pytest.fixture(scope="module")
def grid():
    out = {}
    for N in GRID_N:
        case, compiled, pats = grid_case(N)
        out[N] = (case, compiled, pats, LR.logits64(case[0], case[1], case[2]))
    return out


def test_grid_reaches_the_caps(grid):
    case, compiled, pats, _ = grid[6625]
    assert max(c["P"] for c in compiled) == 4096 and max(c["S"] for c in compiled) == 64
    assert max(int((c["delta"] >= 0).sum()) for c in compiled) > 2048     # arcs = predecessor bytes
    assert sum(1 for T, k in zip(case[3], case[4]) if k and T * (compiled[k - 1]["P"] + compiled[k - 1]["S"]) > 8192) >= 1


@pytest.mark.parametrize("N", GRID_N)
def test_device_rule_against_fp64(hip_session, grid, N):
    case, compiled, pats, l64 = grid[N]
    z, W, b, tpl, line_pat = case
    out = run_dev(hip_session, case, compiled)
    try:
        wv, wp, wl, n_matched, n_exact, n_unmatched = PR.check_pattern(out, l64, tpl, line_pat, pats, AR.VIT_TOL, AR.PROB_TOL, LR.HOOK_TOL, what=N)
    finally:
        loose = PR.figures(out, l64, tpl, line_pat, pats)
        print("N=%d: worst Viterbi deviation %.3e, worst |prob - fp64| %.3e, worst logprob / free_logprob deviation %.3e" % ((N,) + loose))
    print("N=%d: %d matched, %d held to the fp64 path, %d unmatched" % (N, n_matched, n_exact, n_unmatched))
    assert n_matched >= 10 and n_exact >= 8 and n_unmatched >= 2, (n_matched, n_exact, n_unmatched)
    each = run_dev(hip_session, case, compiled, chunk=1)   # every line a chunk of its own
    for key in KEYS:
        assert each[key].tobytes() == out[key].tobytes(), key


def long_case():
    rng = np.random.default_rng(301)
    N = 65
    data, entries = PR.synthetic_dictionary(N)
    text = "[%s-%s]*" % (ch(1), ch(62))                   # S = 2, P = 62: 64 codes per step, so 128 steps fill the LDS table
    pat, c = PR.Pattern(text, entries), retto_amd.debug_pattern_compile(data, text)
    assert c["P"] + c["S"] == 64
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    tpl = [300, 12, 128, 129, 513]
    paths = []
    for T in tpl:   # a planted string of 10 tokens spread over the line
        s = [int(v) for v in rng.permutation(np.arange(1, 63))[:10]]
        rep = T // len(s)
        paths.append((T, [k for k in s for _ in range(rep)] + [s[-1]] * (T - rep * len(s))))
    z = LR.planted_features(rng, W.astype(np.float64), paths, gain=1.5, noise=0.3)
    return (z, W, b, tpl, [1] * len(tpl)), [c], [pat]


def test_long_lines_on_both_sides_of_the_lds_boundary(hip_session):
    """T = 128 is the last line whose backpointer codes fit the LDS table (128 x 64 = pt::BP_LDS), T = 129 the first that sends
    them through the scratch buffer; T = 300 and 513 lie well beyond, and a line of 12 steps between them takes the LDS path in
    the same launch.  The Viterbi tolerance is the one measured for lines of this length (AR.VIT_TOL_LONG);
    logprob and free_logprob, sums of up to 513 fp32 terms, are held to PR.LOGPROB_TOL_LONG (four times the host entry's own
    deviation on this case: ctc_pattern_ref.py)"""
    case, compiled, pats = long_case()
    z, W, b, tpl, line_pat = case
    l64 = LR.logits64(z, W, b)
    out = run_dev(hip_session, case, compiled)             # one launch: 982 rows fit a chunk
    print("long lines: figures", PR.figures(out, l64, tpl, line_pat, pats), "tolerances", (AR.VIT_TOL_LONG, AR.PROB_TOL, PR.LOGPROB_TOL_LONG))
    print("long lines: the host entry's figures", PR.figures(run_host(case, compiled), l64, tpl, line_pat, pats))
    _, _, _, n_matched, n_exact, _ = PR.check_pattern(out, l64, tpl, line_pat, pats, AR.VIT_TOL_LONG, AR.PROB_TOL, PR.LOGPROB_TOL_LONG)
    assert n_matched == 5 and n_exact == 5
    each = run_dev(hip_session, case, compiled, chunk=1)
    for key in KEYS:
        assert each[key].tobytes() == out[key].tobytes(), key
    host = run_host(case, compiled)
    assert host["matched"].tolist() == out["matched"].tolist() and host["idx"].tolist() == out["idx"].tolist()


def test_known_answers_equal_the_host_entry_bit_for_bit(hip_session):
    """the tie cases of test_pattern_cpu.py: exact logits, so the device's adds and compares are the host's"""
    z, W, b, tpl, line_pat, compiled, pats, l64 = PR.known_case(retto_amd.debug_pattern_compile)
    case = (z, W, b, tpl, line_pat)
    dev, host = run_dev(hip_session, case, compiled), run_host(case, compiled)
    for key in ("idx", "matched", "vit"):
        assert dev[key].tobytes() == host[key].tobytes(), key
    o = 0
    for i, (what, _, _, want, matched) in enumerate(PR.KNOWN):
        assert int(dev["matched"][i]) == matched, what
        if matched:
            assert dev["idx"][o:o + tpl[i]].tolist() == want, what
        o += tpl[i]
    vtol, ptol = AR.fmt_tol(5, 8.0)
    PR.check_pattern(dev, l64, tpl, line_pat, pats, vtol, ptol, 8 * vtol, exact_logits=True)


def test_lines_of_pattern_0_and_caller_rows_come_back_untouched(hip_session, grid):
    """the caller's own rows in place of the canaries: an unmatched line and a line without a pattern keep theirs bit for bit"""
    case, compiled, pats, l64 = grid[65]
    z, W, b, tpl, line_pat = case
    rng = np.random.default_rng(5)
    idx0 = rng.integers(0, 65, max(sum(tpl), 1)).astype(np.int32); prob0 = rng.random(max(sum(tpl), 1)).astype(np.float32)
    half = [k if i % 2 else 0 for i, k in enumerate(line_pat)]
    out = run_dev(hip_session, (z, W, b, tpl, half), compiled, chunk=64, idx0=idx0, prob0=prob0)
    PR.check_pattern(out, l64, tpl, half, pats, AR.VIT_TOL, AR.PROB_TOL, LR.HOOK_TOL, idx0=idx0, prob0=prob0)


def test_bad_arguments_are_rejected(hip_session):
    lib = _lib.load()
    z, W, b, tpl, line_pat, compiled, pats, l64 = PR.known_case(retto_amd.debug_pattern_compile)
    f, h = lib.rt_debug_ctc_pattern, hip_session._hd.h
    bad = dict(compiled[0]); bad["delta"] = compiled[0]["delta"].copy(); bad["delta"][0, 1] = 9
    n = len(tpl)
    for lp, comp, chunk, msg in (([2] + [0] * (n - 1), compiled[:1], 0, b"line 0 names pattern 2, outside [0, 1]"),
                                 ([1] + [0] * (n - 1), [bad], 0, b"pattern 1: delta[0][1] is outside [-1, S)"),
                                 ([1] + [0] * (n - 1), compiled[:1], -1, b"chunk_rows is negative")):
        assert PR.call(f, h, z, W, b, tpl, lp, comp, chunk=chunk)[0] == 8
        assert msg in lib.rt_last_error(h), lib.rt_last_error(h)
