"""Rec keywords (retto_amd/csrc/ctc_keyword.h) on the MI355X: the device path (the row gather in chunks of whole lines, the CTC FC
GEMM, k_ctc_row_max, k_ctc_keyword_spot, k_ctc_keyword_topk) through rt_debug_ctc_keywords against the fp64 restatement in
ctc_keyword_ref.py.  The checks are margin-free and leave no line and no entry out (ctc_keyword_ref.check_grid): for every (line,
entry) the fp64 value of the best alignment confined to the returned span is within the tolerance of the returned score, and the
fp64 optimum is no more than the tolerance above that value; the hits are exactly the top 8 of the returned table.

Measured on an MI355X over the grid of test_device_rule_against_fp64 (N in 5, 65, 6625; per N five lists of 1, 3, 4, 5 and 257
entries whose lengths are exactly 1, 7, 8, 15, 16, 31; per list lines of 1, need - 1, need and 40 steps, a line without a list after
every third, one line of 301 steps; both chunkings give the same figures; fp64 reference on the same features), the larger of
|score - confined| and optimum - confined: on the lines of up to 40 steps 1.187e-4 at N = 5, 1.092e-4 at N = 65, 1.297e-4 at
N = 6625; on the line of 301 steps 1.090e-5, 3.362e-5, 7.050e-5.  The short lines' worst, 1.297e-4, passes a quarter of
ctc_align_ref.VIT_TOL (3.13e-4), so their tolerance is four times what the plain fp32 host loops deviate from fp64 on the same
grid (1.094e-4): ctc_keyword_ref.TOL = 4.376e-4.  The long line's worst is below a quarter of ctc_align_ref.VIT_TOL_LONG (3.47e-3),
which stands (ctc_keyword_ref.TOL_LONG)."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_keyword_ref as KR
import ctc_lexicon_ref as LR

pytestmark = pytest.mark.gpu


tol_of = KR.tol_of


def run_dev(sess, case, chunk=0):
    lib = _lib.load()
    rc, out = KR.call(lib.rt_debug_ctc_keywords, sess._hd.h, *case, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case):
    rc, out = KR.call(_lib.load().rt_debug_ctc_keywords_host, None, *case)
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def grid():
    return {N: KR.grid_case(N) for N in LR.GRID_N}


@pytest.mark.parametrize("chunk", [0, 1], ids=["default_chunks", "one_line_chunks"])
@pytest.mark.parametrize("N", LR.GRID_N)
def test_device_rule_against_fp64(hip_session, grid, N, chunk):
    """chunk_rows = 1: every chunk takes its first line and no other"""
    case = grid[N]
    z, W, b, tpl, line_kw, lists, mins = case
    assert sorted({len(e) for lst in lists for e in lst}) == list(LR.GRID_LENS) and [len(lst) for lst in lists] == list(LR.GRID_COUNTS)
    assert max(tpl) > 300 and 0 in line_kw and 1 in tpl
    out = run_dev(hip_session, case, chunk=chunk)
    worst = KR.check_grid(out, *case, tol_of=tol_of, what=(N, chunk))
    short = max([max(w) for T, w in worst.items() if T <= 40] + [0.0]); long_ = max([max(w) for T, w in worst.items() if T > 40] + [0.0])
    print("N=%d chunk=%d: worst deviation %.3e up to 40 steps, %.3e on the long line" % (N, chunk, short, long_))
    assert out["n"].max() == KR.HITS and (out["n"][[i for i, k in enumerate(line_kw) if k == 0]] == 0).all()
    assert not (out["score"] == KR.CANARY_F).any() and not (out["span"] == KR.CANARY_COL).any()


def test_chunkings_agree(hip_session, grid):
    """a line's table does not depend on the chunk it came in beyond the logits GEMM's rounding; infeasibility and the counts
    agree everywhere"""
    case = grid[65]
    a, b = run_dev(hip_session, case), run_dev(hip_session, case, chunk=1)
    assert np.array_equal(np.isneginf(a["score"]), np.isneginf(b["score"])) and np.array_equal(a["n"], b["n"])
    f = np.isfinite(a["score"])
    assert np.abs(a["score"][f].astype(np.float64) - b["score"][f]).max() <= 2 * KR.TOL_LONG


def exact_case(rng, N, T_lines, n_entries):
    """integer logits in [-3, 0]: every fp32 sum is exact on any device, and ties are everywhere"""
    lst = [LR.random_entry(rng, N, int(rng.integers(1, 9)), 12) for _ in range(n_entries)]
    lst += [lst[0], lst[1], [1], [1, 1], [2, 1], [1, 2, 1]]
    lines = [(rng.integers(-3, 1, (T, N)), 1 if i % 3 else 2) for i, T in enumerate(T_lines)]
    return KR.case(lines, N, [lst, lst[::-1][:5]], [-np.inf, -2.0])


@pytest.mark.parametrize("N", [4, 65])
def test_exact_inputs_equal_the_host_rule_bit_for_bit(hip_session, N):
    """scores, spans and hit order: every tie rule crossed on the device"""
    case = exact_case(np.random.default_rng(500 + N), N, [40, 13, 1, 0, 7, 64, 2], 40)
    host = run_host(case)
    want = KR.expected(*case)
    assert KR.same(host, want)
    for chunk in (0, 1, 16):
        dev = run_dev(hip_session, case, chunk=chunk)
        assert KR.same(dev, host), (chunk, np.flatnonzero(dev["score"] != host["score"])[:8], np.flatnonzero((dev["span"] != host["span"]).any(axis=1))[:8])
    sc = host["score"][np.isfinite(host["score"])]
    assert len(sc) - len(np.unique(sc)) > 50   # ties are abundant


@pytest.mark.parametrize("N", [65, 6625])
def test_planted_keywords_score_zero_on_their_span(hip_session, N):
    """an entry planted into the middle of a line of noise: the greedy path holds it, so its score is exactly 0.0, and its span is
    the planted one (from the first step of its first token to the first step of its last)"""
    rng = np.random.default_rng(4100 + N)
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    entries = [LR.random_entry(rng, N, L, 36) for L in (1, 4, 7, 8, 15, 16, 31)]
    rows, tpl, spans = [], [], []
    for e in entries:
        nd, at, T = LR.need(e), int(rng.integers(1, 6)), 48
        path = LR.alignment(e, nd + 2)       # (the last token held two steps more: the earliest end is its first)
        rows.append(KR.planted_rows(rng, W.astype(np.float64), T, path, at)); tpl.append(T); spans.append((at, at + nd - 1))
    case = (np.concatenate(rows), W, b, tpl, [1] * len(tpl), [entries], [0.0])
    d = KR.cost64(*case[:3])
    for i, e in enumerate(entries):   # (what the rule itself gives in fp64: the planted span, at 0)
        sc, fi, la = KR.spot64(d[48 * i:48 * i + 48], [e])
        assert (float(sc[0]), int(fi[0]), int(la[0])) == (0.0,) + spans[i], (i, sc, fi, la, spans[i])
    out = run_dev(hip_session, case)
    for i, (sc_row, sp_row) in enumerate(KR.split_rows(out, case[4], case[5])):
        assert sc_row[i].tobytes() == np.float32(0.0).tobytes() and tuple(int(x) for x in sp_row[i]) == spans[i], (i, sc_row[i], sp_row[i], spans[i])
        hit = [int(x) for x in out["hits"][i]["entry"][:out["n"][i]]]
        assert i in hit and all(out["hits"][i]["score"][j] == 0.0 for j in range(out["n"][i]))   # (min_score = 0: exact-zero hits only)
    KR.check_grid(out, *case, tol_of=tol_of)


def test_mixed_lists_and_untouched_lines(hip_session, grid):
    """no line at all is no work at all; a line's values do not depend on what else is in the call"""
    z, W, b, tpl, line_kw, lists, mins = grid[65]
    none = run_dev(hip_session, (z, W, b, tpl, [0] * len(tpl), lists, mins))
    assert (none["n"] == 0).all() and (none["hits"]["entry"] == KR.CANARY_ENTRY).all() and (none["score"] == KR.CANARY_F).all()
    out = run_dev(hip_session, (z, W, b, tpl, line_kw, lists, mins))
    i = max(j for j, (T, k) in enumerate(zip(tpl, line_kw)) if k == 2 and T == 40)
    offs = np.concatenate([[0], np.cumsum(tpl)])
    alone = run_dev(hip_session, (z[offs[i]:offs[i + 1]], W, b, [tpl[i]], [2], lists, mins))
    assert alone["hits"][0]["entry"].tolist() == out["hits"][i]["entry"].tolist()
    assert alone["hits"][0]["first_col"].tolist() == out["hits"][i]["first_col"].tolist()


def test_bad_arguments_are_rejected(hip_session):
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f, h = lib.rt_debug_ctc_keywords, hip_session._hd.h
    for (tpl, line_kw, lists, mins), chunk, msg in ((([4], [2], [[[1]]], [0.0]), 0, b"line 0 names list 2, outside [0, 1]"),
                                                    (([4], [1], [[[5]]], [0.0]), 0, b"class id 5 in entry 0 is outside [1, 5)"),
                                                    (([4], [1], [[[1]]], [1.0]), 0, b"kw_min_score[0]"),
                                                    (([4], [1], [[[1]]], [0.0]), -1, b"chunk_rows is negative")):
        assert KR.call(f, h, z, W, b, tpl, line_kw, lists, mins, chunk=chunk)[0] == 8
        assert msg in lib.rt_last_error(h), lib.rt_last_error(h)
