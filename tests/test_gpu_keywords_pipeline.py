"""Rec keywords inside the pipeline on the MI355X (rt_keywords_create, rt_set_rec_keywords, rt_run_regions_keywords,
rt_results_rec_keywords): on test_gpu_lexicon_pipeline.py's page, boxes and session settings -- three lanes, word boxes on,
candidates = 3.  Keywords only read a line: with a charset, a lexicon with snap, a pattern, word boxes and candidates on, every
other result is what it is without the list, bit for bit, the per-stage JSON included.  A keyword cut from a line's own decoded
tokens is a hit at (nearly) 0 -- the fused head's argmax and the recomputed logits may differ at near ties only -- on the time
steps of an occurrence, and every hit's quad is rt_debug_span_quad of its span, with rec_return_word_box on or off."""
import ctypes as C
import math

import numpy as np
import pytest

import retto_amd

import crop_source_cases as CS
import ctc_align_ref as AR
from test_gpu_charset_pipeline import reference_rows
from test_gpu_lexicon_align_pipeline import line_geometry
from test_gpu_lexicon_pipeline import _session, variants
from test_gpu_pattern_pipeline import exact_pattern, pat_bits, same_but_det_scores

pytestmark = pytest.mark.gpu


def own_entries(ref):
    """per line a keyword cut from its own decoded tokens (tokens 1 .. 4, or what there is), None for an empty line"""
    out = []
    for g in ref.rec_result:
        t = [int(x) for x in g.tokens]
        out.append((t[1:5] or t[:1]) or None)
    return out


def prepare(s):
    page, m = CS.page_with_tall_line()
    B = np.stack([d.boxes.as_array() for d in s.run_batch([page], det_map_override=[m])[0].det_result])
    assert len(B) == 6
    ref = s.run_regions([page], [B])[0]
    own = own_entries(ref)
    assert sum(e is not None for e in own) >= 4
    N = len(s._dictionary())
    rng = np.random.default_rng(11)
    noise = [[int(c) for c in rng.integers(1, N, int(rng.integers(1, 6)))] for _ in range(40)]
    entries = [e for e in own if e is not None] + noise
    kid = s.create_keywords(ids=entries)
    assert [e for e, _t in s.keywords_entries(kid)] == entries and s.keywords_min_score(kid) == -math.inf
    return {"page": page, "map": m, "B": B, "ref": ref, "own": own, "entries": entries, "kid": kid, "N": N,
            "T": [len(p) for p in reference_rows(s, page, B)], "geom": line_geometry(s, B)}


@pytest.fixture(scope="module")
def session():
    s = _session()
    s.case = prepare(s)
    yield s
    s.close()


def kw_bits(r):
    return [None if g.keywords is None else [(h.entry, h.text, np.float32(h.score).tobytes(), h.first_col, h.last_col,
                                              np.ascontiguousarray(h.box, np.float32).tobytes()) for h in g.keywords] for g in r.rec_result]


def others(r):
    """everything of a result but the keyword hits"""
    return (CS.digest(r), pat_bits(r), [g.lexicon_snapped for g in r.rec_result],
            [g.lexicon_matches and [(e, t, np.float32(ll).tobytes(), np.float32(p).tobytes()) for e, t, ll, p in g.lexicon_matches]
             for g in r.rec_result])


def stage_json(s, page, B, **kw):
    lib = s._hd.lib
    lib.rt_results_json.restype = C.c_char_p
    r = s.run_regions_raw([page], [page.shape[0]], [page.shape[1]], [B], **kw)
    try:
        return [lib.rt_results_json(r, 0, st) for st in range(3)]
    finally:
        lib.rt_results_free(r)


def check_hits_of_line(s, c, k, g, cl, what):
    """a line's hits: ordered, inside the line, each with the quad rt_debug_span_quad gives for its span"""
    lib = s._hd.lib
    page, T, (W, rw) = c["page"], c["T"][k], c["geom"][k]
    rot180 = 1 if cl.label.label == 180 and np.float32(cl.label.score) >= np.float32(0.9) else 0   # (rt_config.cls_thresh)
    assert g.keywords is not None and len(g.keywords) <= retto_amd._lib.KEYWORD_HITS, what
    for a, b in zip(g.keywords, g.keywords[1:]):
        assert a.score > b.score or (a.score == b.score and a.entry < b.entry), (what, a, b)
    box = np.ascontiguousarray(c["B"][k], np.float32).reshape(8)
    for h in g.keywords:
        assert h.score <= 0.0 and 0 <= h.first_col <= h.last_col < T and h.text == "".join(s._dictionary()[i] for i in c["entries"][h.entry]), (what, h)
        quad = np.zeros(8, np.float32)
        assert lib.rt_debug_span_quad(T, W, rw, box.ctypes.data, rot180, page.shape[1], page.shape[0], page.shape[1], page.shape[0],
                                      h.first_col, h.last_col, quad.ctypes.data) == 0
        assert quad.tobytes() == np.ascontiguousarray(h.box, np.float32).tobytes(), (what, h, quad)


def check_own_keywords(s, c, r, what):
    """a keyword cut from a line's own tokens is a hit at (nearly) 0 whose span covers the time steps of an occurrence"""
    for k, e in enumerate(c["own"]):
        g = r.rec_result[k]
        check_hits_of_line(s, c, k, g, r.cls_result[k], (what, k))
        if e is None:
            continue
        hit = [h for h in g.keywords if c["entries"][h.entry] == e]
        assert hit and hit[0].score >= -AR.VIT_TOL, (what, k, e, g.keywords)
        t, cols = [int(x) for x in g.tokens], g.token_cols.tolist()
        occ = [i for i in range(len(t) - len(e) + 1) if t[i:i + len(e)] == e]
        assert any(hit[0].first_col <= cols[i] and cols[i + len(e) - 1] <= hit[0].last_col for i in occ), (what, k, hit[0], cols, occ)


def test_every_other_result_is_bit_identical(session):
    s, c = session, session.case
    page, B, ref, kid = c["page"], c["B"], c["ref"], c["kid"]
    ntok = [len(g.tokens) for g in ref.rec_result]
    short = [int(k) for k in np.argsort(ntok, kind="stable") if 2 <= ntok[k] <= 40]
    kp, kl = short[0], short[1]
    pe = s.create_pattern(exact_pattern(ref.rec_result[kp].tokens))
    rows = reference_rows(s, page, B)
    lex = s.create_lexicon(ids=[e for e in variants(ref.rec_result[kl].tokens, rows[kl]) if e != [int(t) for t in ref.rec_result[kl].tokens]])
    s.set_lexicon_snap(lex, 0.01)
    half = s.create_charset(ids=np.flatnonzero(np.random.default_rng(2024).random(c["N"]) < 0.5).tolist())
    opts = dict(charsets=[[half if k not in (kp, kl) else 0 for k in range(6)]], lexicons=[[lex if k == kl else 0 for k in range(6)]],
                patterns=[[pe if k == kp else 0 for k in range(6)]])
    without = s.run_regions([page], [B], **opts)[0]
    with_kw = s.run_regions([page], [B], keywords=[[kid] * 6], **opts)[0]
    assert others(with_kw) == others(without), CS.differing(CS.digest(with_kw), CS.digest(without))
    assert CS.digest(without) != CS.digest(ref)     # (the other options bite)
    assert all(g.keywords is None for g in without.rec_result) and all(g.keywords is not None for g in with_kw.rec_result)
    assert stage_json(s, page, B, keywords=[[kid] * 6], **opts) == stage_json(s, page, B, **opts)
    # and on the plain decode: only the keywords are new
    plain = s.run_regions([page], [B], keywords=[[kid] * 6])[0]
    assert others(plain) == others(ref)
    check_own_keywords(s, c, plain, "plain")
    for k in range(6):   # (a charset, a snap or a pattern may have rewritten the line: the hits read the model's own logits)
        check_hits_of_line(s, c, k, with_kw.rec_result[k], with_kw.cls_result[k], ("with options", k))
    assert kw_bits(with_kw) == kw_bits(plain)


def test_the_same_results_from_every_entry_point(session):
    s, c = session, session.case
    page, m, B, kid = c["page"], c["map"], c["B"], c["kid"]
    plain = CS.digest(s.run_batch([page], det_map_override=[m])[0])
    explicit = s.run_regions([page], [B], keywords=[[kid] * 6])[0]
    want, wd = kw_bits(explicit), CS.digest(explicit)
    assert all(w is not None for w in want)
    s.set_rec_keywords(kid)
    try:
        a = s.run_batch([page], det_map_override=[m])[0]
        assert kw_bits(a) == want and same_but_det_scores(CS.digest(a), wd)
        t = s.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[m])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.set_rec_keywords(0)
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.create_keywords(ids=[[1]])
        w = s.wait_batch(t)[0]
        assert kw_bits(w) == want and same_but_det_scores(CS.digest(w), wd)
        assert kw_bits(s.run_regions([page], [B])[0]) == want
        # per region: -1 = the session default, 0 = none, k = that list
        k2 = s.create_keywords(ids=[[1], [2, 3]], min_score=-5.0)
        two = s.run_regions([page, page], [B, B], keywords=[None, [0, -1, 0, 0, 0, k2]])
        assert kw_bits(two[0]) == want and CS.digest(two[0]) == wd
        got = kw_bits(two[1])
        assert [x is None for x in got] == [True, False, True, True, True, False]
        assert [h.entry for h in two[1].rec_result[1].keywords] == [h.entry for h in explicit.rec_result[1].keywords]
        assert all(h.score >= -5.0 and h.entry in (0, 1) for h in two[1].rec_result[5].keywords)
    finally:
        s.set_rec_keywords(0)
    after = s.run_batch([page], det_map_override=[m])[0]
    assert CS.digest(after) == plain and all(g.keywords is None for g in after.rec_result)


def test_min_score_zero_reports_exact_zero_hits_only(session):
    s, c = session, session.case
    page, B = c["page"], c["B"]
    k0 = s.create_keywords(ids=c["entries"], min_score=0.0)
    assert s.keywords_min_score(k0) == 0.0
    every = s.run_regions([page], [B], keywords=[[c["kid"]] * 6])[0]
    zero = s.run_regions([page], [B], keywords=[[k0] * 6])[0]
    n = 0
    for g, z in zip(every.rec_result, zero.rec_result):
        assert all(h.score == 0.0 for h in z.keywords)
        assert [(h.entry, h.first_col, h.last_col) for h in z.keywords] == [(h.entry, h.first_col, h.last_col) for h in g.keywords if h.score == 0.0]
        n += len(z.keywords)
    assert n >= 1


def test_quads_without_word_boxes():
    """rec_return_word_box off, candidates off: the hits and their quads are the same"""
    cfg = retto_amd.synthetic_session_config(0, crop_source="Original", max_side_len=CS.SMALL_LIMIT, lanes=3)
    s = retto_amd.RettoSession(cfg)
    try:
        c = prepare(s)
        r = s.run_regions([c["page"]], [c["B"]], keywords=[[c["kid"]] * 6])[0]
        assert all(g.words is None and g.candidates is None for g in r.rec_result)
        for k in range(6):
            check_hits_of_line(s, c, k, r.rec_result[k], r.cls_result[k], ("no word boxes", k))
        assert sum(len(g.keywords) for g in r.rec_result) >= 6
    finally:
        s.close()


def test_unknown_ids_errors_and_the_cap():
    s = _session()
    try:
        c = prepare(s)     # (list 1)
        page, B = c["page"], c["B"]
        with pytest.raises(retto_amd.InvalidArgument, match=r"page 0 region 2: unknown keywords id 9"):
            s.run_regions([page], [B], keywords=[[0, 0, 9, 0, 0, 0]])
        with pytest.raises(retto_amd.InvalidArgument, match=r"unknown keywords id 3"):
            s.set_rec_keywords(3)
        for bad in (0.5, float("nan"), float("inf")):
            with pytest.raises(retto_amd.InvalidArgument, match="min_score"):
                s.create_keywords(ids=[[1]], min_score=bad)
        with pytest.raises(retto_amd.InvalidArgument, match=r"lexicon: U\+0041 in entry 0 matches no dictionary entry"):
            s.create_keywords(["A"])   # the synthetic dictionary has no Latin entry
        with pytest.raises(retto_amd.InvalidArgument, match="no entry"):
            s.create_keywords()
        assert s.keywords_entries(2) == [] and math.isnan(s.keywords_min_score(2))
        for k in range(1, retto_amd._lib.MAX_KEYWORD_LISTS):
            assert s.create_keywords(ids=[[k + 1]]) == k + 1
        with pytest.raises(retto_amd.CapacityError, match="RT_MAX_KEYWORD_LISTS"):
            s.create_keywords(ids=[[1]])
        r = s.run_regions([page], [B], keywords=[[16, 0, 0, 0, 0, 0]])[0]
        assert [h.entry for h in r.rec_result[0].keywords] == [0] and r.rec_result[1].keywords is None
    finally:
        s.close()
