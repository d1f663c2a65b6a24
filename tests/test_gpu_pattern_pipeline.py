"""Rec patterns inside the pipeline on the MI355X (rt_pattern_create, rt_set_rec_pattern, rt_run_regions_patterns,
rt_results_rec_pattern): on test_gpu_lexicon_pipeline.py's page, boxes and session settings -- three lanes, word boxes on,
candidates = 3.  A line whose pattern is its own greedy token string keeps its decode; a line whose pattern forbids one of its
tokens decodes to a string the pattern accepts, with tokens, text, time steps, candidates, score and words consistent the way
test_gpu_lexicon_align_pipeline.check_snapped_line holds a snapped line; every other line and every det and cls result is what it
is without patterns, bit for bit (CS.digest).

logprob against free_logprob on the exact line: both are fp32 sums over the same recomputed logits, each within its own tolerance
of one fp64 value (LR.HOOK_TOL up to 40 steps, PR.LOGPROB_TOL_LONG beyond), so they differ by at most twice that."""
import math

import numpy as np
import pytest

import retto_amd
from retto_amd import synth

import crop_source_cases as CS
import ctc_lexicon_ref as LR
import ctc_pattern_ref as PR
from test_gpu_charset_pipeline import reference_rows
from test_gpu_lexicon_align_pipeline import STATIC, _line, line_geometry
from test_gpu_lexicon_pipeline import _session

pytestmark = pytest.mark.gpu


def atoms(tokens):
    return "".join("\\c{%d}" % int(t) for t in tokens)


def exact_pattern(tokens):
    """the token string as \\c{..} atoms; a line of more than 40 tokens keeps its first 40 as atoms and its rest as a starred set
    of the classes that occur there (the greedy string is accepted either way, and the greedy path is the best path there is)"""
    tokens = [int(t) for t in tokens]
    head, tail = tokens[:40], tokens[40:]
    text = atoms(head) + ("[" + atoms(sorted(set(tail))) + "]*" if tail else "")
    assert len(text.encode()) <= 1024
    return text


def prepare(s):
    page, m = CS.page_with_tall_line()
    B = np.stack([d.boxes.as_array() for d in s.run_batch([page], det_map_override=[m])[0].det_result])
    assert len(B) == 6
    ref = s.run_regions([page], [B])[0]
    rows = reference_rows(s, page, B)
    ntok = [len(g.tokens) for g in ref.rec_result]
    short = [k for k in np.argsort(ntok, kind="stable") if 2 <= ntok[k] <= 40]
    assert len(short) >= 2, ntok     # the exact line and the weakened line are two different lines
    return {"page": page, "map": m, "B": B, "ref": ref, "rows": rows, "T": [len(p) for p in rows], "geom": line_geometry(s, B),
            "exact": int(short[0]), "weak": int(short[1]), "N": len(s._dictionary())}


@pytest.fixture(scope="module")
def session():
    s = _session()
    s.case = prepare(s)
    yield s
    s.close()


def same_but_det_scores(a, b):
    """two digests, all but the det scores: the detector's own in rt_run_batch, 1.0 for a caller's regions"""
    return {k: v for k, v in a.items() if k != "det_scores"} == {k: v for k, v in b.items() if k != "det_scores"}


def pat_bits(r):
    return [None if g.pattern is None else (g.pattern[0], np.float32(g.pattern[1]).tobytes(), np.float32(g.pattern[2]).tobytes())
            for g in r.rec_result]


def check_pattern_line(s, g, accepts, T, quad, page, what, cl, geom):
    """a matched line (cl: its cls result, geom: its (W, resized_w)): everything the decode derives from the rows agrees"""
    rot180 = cl.label.label == 180 and np.float32(cl.label.score) >= np.float32(0.9)   # (rt_config.cls_thresh)
    assert g.pattern is not None and g.pattern[0] is True, what
    assert accepts(g.tokens.tolist()) and g.text == "".join(s._dictionary()[i] for i in g.tokens), what
    cols = g.token_cols.tolist()
    assert len(cols) == len(g.tokens) and all(a < b for a, b in zip(cols, cols[1:])) and 0 <= cols[0] and cols[-1] < T, (what, cols, T)
    assert all(c[0][0] == int(t) for c, t in zip(g.candidates, g.tokens)), what
    assert all(0.0 <= c[0][2] <= 1.0 for c in g.candidates), what
    assert all(i != c[0][0] for c in g.candidates for i, _t, _p2 in c[1:]), what
    assert abs(np.mean([c[0][2] for c in g.candidates]) - g.score) <= 1e-6, what
    want = retto_amd.debug_word_boxes(synth.synth_models(0)[3], g.tokens, cols, T, geom[0], geom[1], quad, rot180, page.shape[1],
                                      page.shape[0], page.shape[1], page.shape[0])
    key = lambda w: (w.text, w.kind, w.first_token, w.n_tokens, w.first_col, w.last_col,
                     np.ascontiguousarray(w.box.as_array(), np.float32).tobytes())
    assert len(g.words) == len(want) >= 1, what
    for x, y in zip(g.words, want):
        assert key(x) == key(y), (what, x, y)
    assert g.pattern[1] <= g.pattern[2] + 2 * LR.HOOK_TOL and math.isfinite(g.pattern[1]), (what, g.pattern)


def test_exact_and_weakened_patterns_and_every_other_line(session):
    s, c = session, session.case
    page, B, ref = c["page"], c["B"], c["ref"]
    ke, kw = c["exact"], c["weak"]
    te = [int(t) for t in ref.rec_result[ke].tokens]; tw = [int(t) for t in ref.rec_result[kw].tokens]
    pe = s.create_pattern(exact_pattern(te))
    info = s.pattern_info(pe)
    assert info["text"] == exact_pattern(te) and info["states"] == len(te) + 1 and info["pairs"] == len(te)
    assert info["min_steps"] == LR.need(te) <= c["T"][ke]
    # the weakened pattern: token j gives way to eight other classes (none of them its own)
    j = len(tw) // 2
    others = [x for x in range(1, c["N"]) if x != tw[j]][:8]
    pw = s.create_pattern(atoms(tw[:j]) + "[" + atoms(others) + "]" + atoms(tw[j + 1:]))
    pats = [0] * 6
    pats[ke], pats[kw] = pe, pw
    r = s.run_regions([page], [B], patterns=[pats])[0]
    d, b = CS.digest(r), CS.digest(ref)
    for key in STATIC:
        assert d[key] == b[key], key
    for k in range(6):
        if k not in (ke, kw):
            assert _line(d, k) == _line(b, k) and r.rec_result[k].pattern is None, k
    assert all(g.pattern is None for g in ref.rec_result)
    # exact: the greedy path is accepted, so it is the answer
    g = r.rec_result[ke]
    assert g.pattern[0] is True and g.tokens.tolist() == te and g.text == ref.rec_result[ke].text
    tol = 2 * (LR.HOOK_TOL if c["T"][ke] <= 40 else PR.LOGPROB_TOL_LONG)
    print("exact line %d, T = %d: logprob %.6f, free_logprob %.6f" % (ke, c["T"][ke], g.pattern[1], g.pattern[2]))
    assert abs(g.pattern[1] - g.pattern[2]) <= tol, (g.pattern, tol)
    check_pattern_line(s, g, lambda t: t == te, c["T"][ke], B[ke], page, "exact", r.cls_result[ke], c["geom"][ke])
    # weakened: the string differs exactly at token j
    g = r.rec_result[kw]
    got = g.tokens.tolist()
    assert len(got) == len(tw) and [i for i in range(len(tw)) if got[i] != tw[i]] == [j] and got[j] in others, (got, tw, j)
    check_pattern_line(s, g, lambda t: len(t) == len(tw) and t[:j] == tw[:j] and t[j + 1:] == tw[j + 1:] and t[j] in others,
                       c["T"][kw], B[kw], page, "weakened", r.cls_result[kw], c["geom"][kw])
    assert g.pattern[1] < g.pattern[2]
    s.case.update(pe=pe, pw=pw, pats=pats, both=r)


def test_the_same_results_from_every_entry_point(session):
    s, c = session, session.case
    page, m, B = c["page"], c["map"], c["B"]
    pe = c.get("pe") or s.create_pattern(exact_pattern(c["ref"].rec_result[c["exact"]].tokens))
    plain = CS.digest(s.run_batch([page], det_map_override=[m])[0])
    explicit = s.run_regions([page], [B], patterns=[[pe] * 6])[0]
    want, wd = pat_bits(explicit), CS.digest(explicit)
    assert all(w is not None for w in want) and want[c["exact"]][0] is True
    s.set_rec_pattern(pe)
    try:
        a = s.run_batch([page], det_map_override=[m])[0]
        assert pat_bits(a) == want and same_but_det_scores(CS.digest(a), wd)
        t = s.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[m])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.set_rec_pattern(0)
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.create_pattern("\\c{1}")
        w = s.wait_batch(t)[0]
        assert pat_bits(w) == want and same_but_det_scores(CS.digest(w), wd)
        assert pat_bits(s.run_regions([page], [B])[0]) == want
        two = s.run_regions([page, page], [B, B], patterns=[None, [0, -1, 0, 0, 0, 0]])
        assert pat_bits(two[0]) == want and CS.digest(two[0]) == wd
        assert [x is None for x in pat_bits(two[1])] == [True, False, True, True, True, True]
        one, all6 = two[1].rec_result[1].pattern, explicit.rec_result[1].pattern     # (alone in its chunk: another GEMM shape)
        assert one[0] == all6[0] and abs(one[2] - all6[2]) <= LR.HOOK_TOL
    finally:
        s.set_rec_pattern(0)
    after = s.run_batch([page], det_map_override=[m])[0]
    assert CS.digest(after) == plain and all(g.pattern is None for g in after.rec_result)


def test_a_kind_per_page_on_three_lanes(session):
    """One run_regions call over three copies of the page, so that each of the three lanes gets one page and reads its own page's
    entry of the call's one per-page option array: page 0's regions carry charsets only (-1 among them: the session default),
    page 1's lexicons only, with no charset entry for the page (the default on every region), page 2's patterns only.  Every
    page is, bit for bit, what it is run alone -- one page, one lane -- with the same options."""
    s, c = session, session.case
    page, B = c["page"], c["B"]
    pe = c.get("pe") or s.create_pattern(exact_pattern(c["ref"].rec_result[c["exact"]].tokens))
    rng = np.random.default_rng(77)
    half, dflt = (s.create_charset(ids=np.flatnonzero(rng.random(c["N"]) < 0.5).tolist()) for _ in range(2))
    lex = s.create_lexicon(ids=[[1], [2], [1, 2]])
    cs0, lx1 = [half, 0, -1, half, -1, 0], [lex, 0, lex, 0, 0, lex]
    pt2 = [pe if k == c["exact"] else 0 for k in range(6)]
    alone = (dict(charsets=[cs0]), dict(lexicons=[lx1]), dict(charsets=[[0] * 6], patterns=[pt2]))
    whole = lambda r: (CS.digest(r), pat_bits(r), [g.lexicon_matches and [(e, t, np.float32(ll).tobytes(), np.float32(p).tobytes())
                                                                           for e, t, ll, p in g.lexicon_matches] for g in r.rec_result])
    s.set_rec_charset(dflt)
    try:
        three = s.run_regions([page] * 3, [B] * 3, charsets=[cs0, None, [0] * 6], lexicons=[None, lx1, None], patterns=[None, None, pt2])
        want = [s.run_regions([page], [B], **kw)[0] for kw in alone]
    finally:
        s.set_rec_charset(0)
    for i in range(3):
        assert whole(three[i]) == whole(want[i]), (i, CS.differing(CS.digest(three[i]), CS.digest(want[i])))
    # each page carries its own kind and no other
    assert [[g.pattern is not None for g in r.rec_result] for r in three] == [[False] * 6, [False] * 6, [p > 0 for p in pt2]]
    assert [[g.lexicon_matches is not None for g in r.rec_result] for r in three] == [[False] * 6, [x > 0 for x in lx1], [False] * 6]
    ref = CS.digest(c["ref"])
    assert CS.digest(three[0]) != ref and CS.digest(three[1]) != ref and CS.digest(three[0]) != CS.digest(three[1])   # the charsets bite
    assert three[2].rec_result[c["exact"]].pattern[0] is True
    assert all(_line(CS.digest(three[2]), k) == _line(ref, k) for k in range(6) if k != c["exact"])   # (0 overrides the default charset)


def test_a_pattern_and_a_charset_on_one_line(session):
    """the charset writes first; a match overwrites its rows, and where the line cannot match the charset's decode stands"""
    s, c = session, session.case
    page, B = c["page"], c["B"]
    ke = c["exact"]
    pe = c.get("pe") or s.create_pattern(exact_pattern(c["ref"].rec_result[ke].tokens))
    half = s.create_charset(ids=np.flatnonzero(np.random.default_rng(2024).random(c["N"]) < 0.5).tolist())
    T = c["T"][ke]
    assert T <= 122
    too_long = s.create_pattern("\\c{1}{%d}" % (T // 2 + 2))     # k equal tokens need 2 k - 1 steps: T + 2 or T + 3
    assert s.pattern_info(too_long)["min_steps"] > T
    only_cs = s.run_regions([page], [B], charsets=[[half] * 6])[0]
    only_pt = s.run_regions([page], [B], patterns=[[pe if k == ke else 0 for k in range(6)]])[0]
    both = s.run_regions([page], [B], charsets=[[half] * 6], patterns=[[pe if k == ke else 0 for k in range(6)]])[0]
    dc, dp, db = CS.digest(only_cs), CS.digest(only_pt), CS.digest(both)
    assert CS.digest(only_cs) != CS.digest(c["ref"])
    g, h = both.rec_result[ke], only_pt.rec_result[ke]
    assert g.pattern[0] is True and g.tokens.tolist() == h.tokens.tolist() and g.token_cols.tolist() == h.token_cols.tolist()
    assert np.float32(g.score).tobytes() == np.float32(h.score).tobytes() and pat_bits(both)[ke] == pat_bits(only_pt)[ke]
    assert [x[0] for x in g.candidates] == [x[0] for x in h.candidates]     # rank 0: the path's (id, prob)
    for k in range(6):
        if k != ke:
            assert _line(db, k) == _line(dc, k), k
    miss = s.run_regions([page], [B], charsets=[[half] * 6], patterns=[[too_long if k == ke else 0 for k in range(6)]])[0]
    assert CS.digest(miss) == dc
    p = miss.rec_result[ke].pattern
    assert p[0] is False and p[1] == -math.inf and math.isfinite(p[2]) and p[2] <= 0.0
    assert abs(p[2] - only_pt.rec_result[ke].pattern[2]) <= LR.HOOK_TOL


def test_a_pattern_and_a_lexicon_on_one_line_are_refused(session):
    s, c = session, session.case
    page, m, B = c["page"], c["map"], c["B"]
    pid = s.create_pattern("\\c{1}+")
    lex = s.create_lexicon(ids=[[1], [2]])
    with pytest.raises(retto_amd.InvalidArgument, match=r"page 1 region 3: both a rec pattern \(%d\) and a rec lexicon \(%d\)" % (pid, lex)):
        s.run_regions([page, page], [B, B], patterns=[None, [0, 0, 0, pid, 0, 0]], lexicons=[None, [0, lex, 0, lex, 0, 0]])
    s.set_rec_lexicon(lex)
    try:
        with pytest.raises(retto_amd.InvalidArgument, match=r"page 0 region 0: both a rec pattern"):
            s.run_regions([page], [B], patterns=[[pid, 0, 0, 0, 0, 0]])      # the default lexicon meets the region's pattern
        s.set_rec_pattern(pid)
        with pytest.raises(retto_amd.InvalidArgument, match="session defaults name both"):
            s.run_batch([page], det_map_override=[m])
        with pytest.raises(retto_amd.InvalidArgument, match="session defaults name both"):
            s.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[m])
    finally:
        s.set_rec_pattern(0); s.set_rec_lexicon(0)
    ok = s.run_regions([page], [B], patterns=[[pid, 0, 0, 0, 0, 0]], lexicons=[[0, lex, 0, 0, 0, 0]])[0]   # side by side is fine
    assert ok.rec_result[0].pattern is not None and ok.rec_result[1].lexicon_matches is not None
    assert CS.digest(s.run_regions([page], [B])[0]) == CS.digest(c["ref"])


def test_unknown_ids_errors_and_the_cap():
    s = _session()
    try:
        c = prepare(s)
        page, B = c["page"], c["B"]
        with pytest.raises(retto_amd.InvalidArgument, match=r"page 0 region 2: unknown pattern id 9"):
            s.run_regions([page], [B], patterns=[[0, 0, 9, 0, 0, 0]])
        with pytest.raises(retto_amd.InvalidArgument, match=r"unknown pattern id 3"):
            s.set_rec_pattern(3)
        with pytest.raises(retto_amd.InvalidArgument, match=r"pattern: U\+0041 matches no dictionary entry \(byte offset 0\)"):
            s.create_pattern("A")   # the synthetic dictionary has no Latin entry
        with pytest.raises(retto_amd.CapacityError, match="RT_PATTERN_MAX_STATES"):
            s.create_pattern("\\c{1}{64}")
        assert s.pattern_info(1) is None
        for k in range(retto_amd._lib.MAX_PATTERNS):
            assert s.create_pattern("\\c{%d}*" % (k + 1)) == k + 1
        with pytest.raises(retto_amd.CapacityError, match="RT_MAX_PATTERNS"):
            s.create_pattern("\\c{1}")
        assert s.pattern_info(16) == {"text": "\\c{16}*", "states": 2, "pairs": 1, "min_steps": 1}
        r = s.run_regions([page], [B], patterns=[[16, 0, 0, 0, 0, 0]])[0]      # the start state accepts: blanks or runs of class 16
        assert r.rec_result[0].pattern[0] is True and set(r.rec_result[0].tokens.tolist()) <= {16}
        assert _line(CS.digest(r), 1) == _line(CS.digest(c["ref"]), 1)
    finally:
        s.close()
