"""Rec beams inside the pipeline on the MI355X (rt_set_rec_beam, rt_results_rec_beams / _beam_tokens / _beam_text): on
test_gpu_lexicon_pipeline.py's page and session settings -- three lanes, word boxes on, candidates = 3.  Off, a session returns
what it returned before it heard of the option; on, every other result -- with a charset, a lexicon with snap, a pattern and a
keyword list on the lines as well -- is what it is without the beams, bit for bit, the per-stage JSON included.  The hypotheses
of a line are the same from rt_run_batch, rt_submit_batch / rt_wait_batch and rt_run_regions; a hypothesis that is the line's
greedy decode has the line's text; the Python field mirrors the C results."""
import ctypes as C

import numpy as np
import pytest

import retto_amd

import crop_source_cases as CS
import ctc_beam_ref as BR
from test_gpu_charset_pipeline import reference_rows
from test_gpu_keywords_pipeline import kw_bits, others, stage_json
from test_gpu_lexicon_pipeline import _session, variants
from test_gpu_pattern_pipeline import exact_pattern, same_but_det_scores

pytestmark = pytest.mark.gpu

BEAM, NBEST = 16, 4


@pytest.fixture(scope="module")
def session():
    s = _session()
    page, m = CS.page_with_tall_line()
    B = np.stack([d.boxes.as_array() for d in s.run_batch([page], det_map_override=[m])[0].det_result])
    assert len(B) == 6
    T = [len(p) for p in reference_rows(s, page, B)]
    width = [float(np.linalg.norm(b[1] - b[0])) for b in B]
    order = np.argsort(width, kind="stable")
    three = sorted(int(k) for k in (order[0], order[len(order) // 2], order[-1]))   # the shortest line, one between, the widest
    assert width[order[0]] < width[order[len(order) // 2]] < width[order[-1]]
    s.case = {"page": page, "map": m, "B": B, "T": T, "three": three, "B3": B[three], "ref": s.run_regions([page], [B])[0],
              "ref3": s.run_regions([page], [B[three]])[0]}
    yield s
    s.close()


def beam_bits(r):
    return [None if g.beams is None else [(h.tokens.tolist(), h.text, np.float32(h.logprob).tobytes()) for h in g.beams] for g in r.rec_result]


def check_line(s, g, T, what):
    """a line's hypotheses: up to NBEST, distinct, without a blank, no longer than the line, best first, each with its text"""
    dic = s._dictionary()
    assert g.beams is not None and 1 <= len(g.beams) <= NBEST, what
    assert len({tuple(h.tokens.tolist()) for h in g.beams}) == len(g.beams), what
    for a, b in zip(g.beams, g.beams[1:]):
        assert a.logprob >= b.logprob, (what, a, b)
    for h in g.beams:
        assert len(h.tokens) <= T and all(1 <= c < len(dic) for c in h.tokens) and np.isfinite(h.logprob) and h.logprob <= BR.TOL, (what, h)
        assert h.text == "".join(dic[c] for c in h.tokens), (what, h)


def test_off_is_what_it_was(session):
    s, c = session, session.case
    page, B3 = c["page"], c["B3"]
    lib = s._hd.lib
    assert s.rec_beam() == (0, 0) and all(g.beams is None for g in c["ref3"].rec_result)
    before = stage_json(s, page, B3)
    s.set_rec_beam(BEAM, NBEST)
    assert s.rec_beam() == (BEAM, NBEST)
    s.set_rec_beam(0)
    assert s.rec_beam() == (0, 0)
    r = s.run_regions_raw([page], [page.shape[0]], [page.shape[1]], [B3])
    try:
        for k in range(3):
            assert lib.rt_results_rec_beams(r, 0, k, None) == 0 and lib.rt_results_rec_beam_tokens(r, 0, k, 0, None) == 0
            assert lib.rt_results_rec_beam_text(r, 0, k, 0) is None
    finally:
        lib.rt_results_free(r)
    after = s.run_regions([page], [B3])[0]
    assert others(after) == others(c["ref3"]) and beam_bits(after) == [None] * 3 and stage_json(s, page, B3) == before
    for beam, nbest in ((33, 1), (4, 0), (4, 5), (32, 9), (-1, 1)):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_set_rec_beam"):
            s.set_rec_beam(beam, nbest)
    assert s.rec_beam() == (0, 0)


def test_on_every_other_result_is_bit_identical(session):
    s, c = session, session.case
    page, B3, ref3 = c["page"], c["B3"], c["ref3"]
    rows = reference_rows(s, page, B3)
    T = [len(p) for p in rows]
    try:
        s.set_rec_beam(BEAM, NBEST)
        plain = s.run_regions([page], [B3])[0]
        assert others(plain) == others(ref3), CS.differing(CS.digest(plain), CS.digest(ref3))
        greedy = 0
        for k in range(3):
            g = plain.rec_result[k]
            check_line(s, g, T[k], ("plain", k))
            for h in g.beams:   # (a hypothesis that is the line's greedy decode has the line's text)
                if h.tokens.tolist() == g.tokens.tolist():
                    assert h.text == g.text
                    greedy += 1
        print("lines whose greedy decode is among their hypotheses:", greedy)
        assert greedy >= 1
        # with every other option on the lines as well
        fits = [k for k in (0, 1) if 2 <= len(ref3.rec_result[k].tokens) <= 40]
        assert fits
        kp, kl = fits[0], 2
        kc = 1 - kp
        pe = s.create_pattern(exact_pattern(ref3.rec_result[kp].tokens))
        lex = s.create_lexicon(ids=[e for e in variants(ref3.rec_result[kl].tokens, rows[kl]) if e != [int(t) for t in ref3.rec_result[kl].tokens]])
        s.set_lexicon_snap(lex, 0.01)
        N = len(s._dictionary())
        half = s.create_charset(ids=np.flatnonzero(np.random.default_rng(2024).random(N) < 0.5).tolist())
        kid = s.create_keywords(ids=[[int(t) for t in ref3.rec_result[1].tokens][:3] or [1], [2, 3]])
        opts = dict(charsets=[[half if k == kc else 0 for k in range(3)]], lexicons=[[0, 0, lex]],
                    patterns=[[pe if k == kp else 0 for k in range(3)]], keywords=[[kid] * 3])
        with_beam = s.run_regions([page], [B3], **opts)[0]
        json_on = stage_json(s, page, B3, **opts)
        s.set_rec_beam(0)
        without = s.run_regions([page], [B3], **opts)[0]
        assert others(with_beam) == others(without), CS.differing(CS.digest(with_beam), CS.digest(without))
        assert kw_bits(with_beam) == kw_bits(without) and json_on == stage_json(s, page, B3, **opts)
        assert CS.digest(without) != CS.digest(ref3)      # (the other options bite)
        # the beam reads the model's own distribution: a charset, a snap or a pattern on the line does not change it
        assert beam_bits(with_beam) == beam_bits(plain) and beam_bits(without) == [None] * 3
    finally:
        s.set_rec_beam(0)


def test_the_same_beams_from_every_entry_point_and_the_python_mirror(session):
    s, c = session, session.case
    page, m, B = c["page"], c["map"], c["B"]
    lib = s._hd.lib
    plain = CS.digest(s.run_batch([page], det_map_override=[m])[0])
    s.set_rec_beam(BEAM, NBEST)
    try:
        a = s.run_batch([page], det_map_override=[m])[0]
        want, wd = beam_bits(a), CS.digest(a)
        assert all(w is not None for w in want) and wd == plain
        for k in range(6):
            check_line(s, a.rec_result[k], c["T"][k], ("batch", k))
        t = s.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[m])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.set_rec_beam(0)
        w = s.wait_batch(t)[0]
        assert beam_bits(w) == want and CS.digest(w) == wd
        reg = s.run_regions([page], [B])[0]
        assert beam_bits(reg) == want and same_but_det_scores(CS.digest(reg), wd)
        two = s.run_regions([page, page], [B, B[c["three"]]])
        assert beam_bits(two[0]) == want
        # (three of the lines in a call of their own: another chunk, so the logits GEMM may round differently)
        for g, k in zip(two[1].rec_result, c["three"]):
            assert [h.tokens.tolist() for h in g.beams] == [h.tokens.tolist() for h in a.rec_result[k].beams], k
            assert max(abs(x.logprob - y.logprob) for x, y in zip(g.beams, a.rec_result[k].beams)) <= 2 * BR.tol_of(c["T"][k])
        # the Python field against the C results
        r = s.run_regions_raw([page], [page.shape[0]], [page.shape[1]], [B])
        try:
            for k in range(6):
                bp = C.POINTER(retto_amd._lib.Beam)()
                n = lib.rt_results_rec_beams(r, 0, k, C.byref(bp))
                assert n == len(reg.rec_result[k].beams)
                for q in range(n):
                    tp = C.POINTER(C.c_int32)()
                    nt = lib.rt_results_rec_beam_tokens(r, 0, k, q, C.byref(tp))
                    h = reg.rec_result[k].beams[q]
                    assert nt == bp[q].n_tokens == len(h.tokens) and [tp[i] for i in range(nt)] == h.tokens.tolist()
                    assert np.float32(bp[q].logprob).tobytes() == np.float32(h.logprob).tobytes()
                    assert lib.rt_results_rec_beam_text(r, 0, k, q).decode("utf-8") == h.text
                assert lib.rt_results_rec_beam_tokens(r, 0, k, n, None) == 0 and lib.rt_results_rec_beam_text(r, 0, k, n) is None
            assert lib.rt_results_rec_beams(r, 0, 6, None) == 0 and lib.rt_results_rec_beams(r, 1, 0, None) == 0
        finally:
            lib.rt_results_free(r)
        # a narrower beam: rank 0 alone
        s.set_rec_beam(1)
        one = s.run_regions([page], [B])[0]
        assert all(len(g.beams) == 1 for g in one.rec_result) and same_but_det_scores(CS.digest(one), wd)
    finally:
        s.set_rec_beam(0)
    after = s.run_batch([page], det_map_override=[m])[0]
    assert CS.digest(after) == plain and all(g.beams is None for g in after.rec_result)
