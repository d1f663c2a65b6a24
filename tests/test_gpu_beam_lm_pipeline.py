"""The rec language model inside the pipeline on the MI355X (rt_lm_create, rt_set_rec_beam_lm, rt_results_rec_beam_lm): on
test_gpu_beam_pipeline.py's page and session.  With no model set the beams are the beams-only session's bytes; with a model set --
and a charset, a lexicon with snap, a pattern and a keyword list on the lines as well -- every other result, the per-stage JSON
included, is what it is without the model, bit for bit, and only the beams differ.  The hypotheses of a line are the same from
rt_run_batch, rt_submit_batch / rt_wait_batch and rt_run_regions; score = logprob + alpha lm + beta n_tokens and lm is the
model's own sum over the string, to the tolerance test_beam_lm_cpu.py measures; the Python fields mirror the C results."""
import ctypes as C

import numpy as np
import pytest

import retto_amd

import crop_source_cases as CS
import ctc_lm_ref as MR
from test_gpu_beam_pipeline import BEAM, NBEST, beam_bits, session   # noqa: F401  (the fixture)
from test_gpu_charset_pipeline import reference_rows
from test_gpu_keywords_pipeline import kw_bits, others, stage_json
from test_gpu_lexicon_pipeline import variants
from test_gpu_pattern_pipeline import exact_pattern, same_but_det_scores

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.8, 0.6


def lm_bits(r):
    return [None if g.beams is None else [(h.tokens.tolist(), h.text, np.float32(h.logprob).tobytes(),
                                           None if h.lm_logprob is None else np.float32(h.lm_logprob).tobytes(),
                                           None if h.lm_score is None else np.float32(h.lm_score).tobytes()) for h in g.beams] for g in r.rec_result]


@pytest.fixture(scope="module")
def model(session):
    """a trigram model over the session's dictionary around what the lines read, written as ARPA text and created once"""
    s = session
    dic = s._dictionary()
    texts = [tuple(int(t) for t in g.tokens) for g in s.case["ref"].rec_result]
    m = MR.random_model(77, len(dic), 3, texts, per_level=300)
    lm = s.create_lm(MR.write_arpa(m, dic), oov_log10=m.oov / MR.LN10)
    assert lm == 0 and s.lm_info(lm) == {"order": 3, "ngrams": len(m.grams), "dropped": 0, "states": len(m.state_index)}
    assert s.lm_info(1) is None and s.lm_info(-1) is None
    return m, lm


def check_fused_line(s, g, m, T, what):
    dic = s._dictionary()
    assert g.beams is not None and 1 <= len(g.beams) <= NBEST, what
    assert len({tuple(h.tokens.tolist()) for h in g.beams}) == len(g.beams), what
    for a, b in zip(g.beams, g.beams[1:]):
        assert a.lm_score >= b.lm_score, (what, a, b)
    for h in g.beams:
        assert len(h.tokens) <= T and all(1 <= c < len(dic) for c in h.tokens) and h.logprob <= MR.TOL, (what, h)
        assert h.text == "".join(dic[c] for c in h.tokens), (what, h)
        assert abs(h.lm_logprob - m.lm64(h.tokens.tolist())) <= MR.tol_of(T), (what, h, m.lm64(h.tokens.tolist()))
        fused = MR.fused64(h.logprob, h.lm_logprob, len(h.tokens), ALPHA, BETA)
        assert abs(h.lm_score - fused) <= MR.tol_of(T), (what, h, fused)


def test_no_model_set_is_the_beams_only_session(session, model):
    """a model that exists but is not attached changes nothing: the hypotheses are the beams-only bytes, without lm fields"""
    s, c = session, session.case
    page, B3 = c["page"], c["B3"]
    lib = s._hd.lib
    _m, lm = model
    assert s.rec_beam_lm() == (-1, 0.0, 0.0)
    s.set_rec_beam(BEAM, NBEST)
    try:
        want = s.run_regions([page], [B3])[0]
        assert all(h.lm_logprob is None and h.lm_score is None for g in want.rec_result for h in g.beams)
        s.set_rec_beam_lm(lm, ALPHA, BETA)
        assert s.rec_beam_lm() == (lm, np.float32(ALPHA), np.float32(BETA))
        s.set_rec_beam_lm(-1)
        assert s.rec_beam_lm() == (-1, 0.0, 0.0)
        again = s.run_regions([page], [B3])[0]
        assert lm_bits(again) == lm_bits(want) and others(again) == others(want)
        r = s.run_regions_raw([page], [page.shape[0]], [page.shape[1]], [B3])
        try:
            for k in range(3):
                p = C.POINTER(retto_amd._lib.BeamLm)()
                assert lib.rt_results_rec_beams(r, 0, k, None) >= 1 and lib.rt_results_rec_beam_lm(r, 0, k, C.byref(p)) == 0 and not p
        finally:
            lib.rt_results_free(r)
        for bad, a, b in ((1, 1.0, 0.0), (-2, 1.0, 0.0), (lm, -0.1, 0.0), (lm, float("nan"), 0.0), (lm, 1.0, float("inf"))):
            with pytest.raises(retto_amd.InvalidArgument, match="rt_set_rec_beam_lm"):
                s.set_rec_beam_lm(bad, a, b)
        assert s.rec_beam_lm() == (-1, 0.0, 0.0)
    finally:
        s.set_rec_beam(0)
    # legal while beam = 0, and without effect until a beam is set
    s.set_rec_beam_lm(lm, ALPHA, BETA)
    try:
        off = s.run_regions([page], [B3])[0]
        assert others(off) == others(c["ref3"]) and beam_bits(off) == [None] * 3
    finally:
        s.set_rec_beam_lm(-1)


def test_model_set_only_the_beams_differ(session, model):
    s, c = session, session.case
    page, B3, ref3 = c["page"], c["B3"], c["ref3"]
    m, lm = model
    rows = reference_rows(s, page, B3)
    T = [len(p) for p in rows]
    try:
        s.set_rec_beam(BEAM, NBEST)
        plain = s.run_regions([page], [B3])[0]
        s.set_rec_beam_lm(lm, ALPHA, BETA)
        fused = s.run_regions([page], [B3])[0]
        assert others(fused) == others(plain) == others(ref3), CS.differing(CS.digest(fused), CS.digest(ref3))
        for k in range(3):
            check_fused_line(s, fused.rec_result[k], m, T[k], ("fused", k))
        assert beam_bits(fused) != beam_bits(plain)       # (the model bites)
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
        with_lm = s.run_regions([page], [B3], **opts)[0]
        json_on = stage_json(s, page, B3, **opts)
        s.set_rec_beam_lm(-1)
        without = s.run_regions([page], [B3], **opts)[0]
        assert others(with_lm) == others(without), CS.differing(CS.digest(with_lm), CS.digest(without))
        assert kw_bits(with_lm) == kw_bits(without) and json_on == stage_json(s, page, B3, **opts)
        assert CS.digest(without) != CS.digest(ref3)      # (the other options bite)
        # the beam reads the model's own distribution: the other options on the line change neither form of it
        assert lm_bits(with_lm) == lm_bits(fused) and lm_bits(without) == lm_bits(plain)
    finally:
        s.set_rec_beam_lm(-1)
        s.set_rec_beam(0)


def test_the_same_hypotheses_from_every_entry_point_and_the_python_mirror(session, model):
    s, c = session, session.case
    page, mp, B = c["page"], c["map"], c["B"]
    lib = s._hd.lib
    m, lm = model
    plain = CS.digest(s.run_batch([page], det_map_override=[mp])[0])
    s.set_rec_beam(BEAM, NBEST)
    s.set_rec_beam_lm(lm, ALPHA, BETA)
    try:
        a = s.run_batch([page], det_map_override=[mp])[0]
        want, wd = lm_bits(a), CS.digest(a)
        assert all(w is not None for w in want) and wd == plain
        for k in range(6):
            check_fused_line(s, a.rec_result[k], m, c["T"][k], ("batch", k))
        t = s.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[mp])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.set_rec_beam_lm(-1)
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.create_lm("\\data\\\nngram 1=0\n\\1-grams:\n\\end\\\n")
        w = s.wait_batch(t)[0]
        assert lm_bits(w) == want and CS.digest(w) == wd
        reg = s.run_regions([page], [B])[0]
        assert lm_bits(reg) == want and same_but_det_scores(CS.digest(reg), wd)
        two = s.run_regions([page, page], [B, B[c["three"]]])
        assert lm_bits(two[0]) == want
        # (three of the lines in a call of their own: another chunk, so the logits GEMM may round differently)
        for g, k in zip(two[1].rec_result, c["three"]):
            assert [h.tokens.tolist() for h in g.beams] == [h.tokens.tolist() for h in a.rec_result[k].beams], k
            assert max(abs(x.lm_score - y.lm_score) for x, y in zip(g.beams, a.rec_result[k].beams)) <= 2 * MR.tol_of(c["T"][k])
        # the Python fields against the C results
        r = s.run_regions_raw([page], [page.shape[0]], [page.shape[1]], [B])
        try:
            for k in range(6):
                bp = C.POINTER(retto_amd._lib.Beam)(); lp = C.POINTER(retto_amd._lib.BeamLm)()
                n = lib.rt_results_rec_beams(r, 0, k, C.byref(bp))
                assert n == len(reg.rec_result[k].beams) == lib.rt_results_rec_beam_lm(r, 0, k, C.byref(lp))
                for q in range(n):
                    h = reg.rec_result[k].beams[q]
                    assert np.float32(bp[q].logprob).tobytes() == np.float32(h.logprob).tobytes()
                    assert np.float32(lp[q].lm).tobytes() == np.float32(h.lm_logprob).tobytes()
                    assert np.float32(lp[q].score).tobytes() == np.float32(h.lm_score).tobytes()
            assert lib.rt_results_rec_beam_lm(r, 0, 6, None) == 0 and lib.rt_results_rec_beam_lm(r, 1, 0, None) == 0
        finally:
            lib.rt_results_free(r)
        # alpha = beta = 0: the beams-only hypotheses with the model's sums beside them
        s.set_rec_beam_lm(lm, 0.0, 0.0)
        zero = s.run_regions([page], [B])[0]
        s.set_rec_beam_lm(-1)
        only = s.run_regions([page], [B])[0]
        assert beam_bits(zero) == beam_bits(only)
        assert all(np.float32(h.lm_score).tobytes() == np.float32(h.logprob).tobytes() for g in zero.rec_result for h in g.beams)
    finally:
        s.set_rec_beam_lm(-1)
        s.set_rec_beam(0)
    after = s.run_batch([page], det_map_override=[mp])[0]
    assert CS.digest(after) == plain and all(g.beams is None for g in after.rec_result)


def test_the_session_holds_four_models(session, model):
    s = session
    tiny = "\\data\\\nngram 1=1\n\n\\1-grams:\n-1.0\t<sp>\n\n\\end\\\n"
    with pytest.raises(retto_amd.InvalidArgument, match="rt_lm_create: lm: line 5: a number is not finite"):
        s.create_lm(tiny.replace("-1.0", "nan"))
    while s.lm_info(MR.MAX_LMS - 1) is None:
        s.create_lm(tiny)
    with pytest.raises(retto_amd.CapacityError, match="RT_MAX_LMS"):
        s.create_lm(tiny)
    assert s.lm_info(3) == {"order": 1, "ngrams": 1, "dropped": 0, "states": 1}


def test_cli_beam_and_lm_flags(tmp_path, session, monkeypatch):
    """--rec-beam B,N alone gives "beams" without lm fields; with --rec-lm and --rec-lm-weights every hypothesis carries
    lm_logprob and lm_score = logprob + ALPHA lm_logprob + BETA len(tokens).  (The synthetic detector finds nothing on its own:
    the CLI's run_batch gets the planted det maps, as every pipeline test here hands them in.)"""
    import json
    from PIL import Image
    from retto_amd import cli, workload
    img = tmp_path / "img"
    img.mkdir()
    rects = []
    for i in range(2):
        page, r = workload.planted_page(160, 320, 2, seed=i)
        Image.fromarray(page).save(img / ("p%d.png" % i))
        rects.append(r)
    run_batch = retto_amd.RettoSession.run_batch

    def with_planted_maps(self, pages, det_map_override=None):
        lib, h = self._hd.lib, self._hd.h
        maps = []
        for r in rects[:len(pages)]:
            rh, rw, dh, dw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert lib.rt_resize_both_dims(h, 160, 320, C.byref(rh), C.byref(rw)) == 0
            assert lib.rt_det_input_dims(h, rh.value, rw.value, C.byref(dh), C.byref(dw)) == 0
            maps.append(workload.planted_map(dh.value, dw.value, 160, 320, r))
        return run_batch(self, pages, det_map_override=maps)

    monkeypatch.setattr(retto_amd.RettoSession, "run_batch", with_planted_maps)
    dic = session._dictionary()
    m = MR.random_model(5, len(dic), 2, per_level=50)
    (tmp_path / "m.arpa").write_bytes(MR.write_arpa(m, dic, unk=m.oov / MR.LN10).encode("utf-8"))   # (<unk> carries the model's oov)
    out = tmp_path / "out.jsonl"
    base = ["--images", str(img), "--synthetic", "--batch", "2", "--json", str(out)]
    assert cli.main(base + ["--rec-beam", "8,2"]) == 0
    plain = [json.loads(l) for l in open(out)]
    assert all(len(l["beams"]) == len(l["rec"]) for l in plain) and sum(len(l["rec"]) for l in plain) >= 1
    assert all(1 <= len(b) <= 2 and all(set(h) == {"text", "tokens", "logprob"} for h in b) for l in plain for b in l["beams"])
    assert cli.main(base + ["--rec-beam", "8,2", "--rec-lm", str(tmp_path / "m.arpa"), "--rec-lm-weights", "0.5,0.25"]) == 0
    fused = [json.loads(l) for l in open(out)]
    assert [l["rec"] for l in fused] == [l["rec"] for l in plain]
    for l in fused:
        for b in l["beams"]:
            for h in b:
                assert set(h) == {"text", "tokens", "logprob", "lm_logprob", "lm_score"}
                assert abs(h["lm_logprob"] - m.lm64(h["tokens"])) <= MR.TOL
                assert abs(h["lm_score"] - (h["logprob"] + 0.5 * h["lm_logprob"] + 0.25 * len(h["tokens"]))) <= MR.TOL
    with pytest.raises(SystemExit, match="--rec-lm needs --rec-beam"):
        cli.main(base + ["--rec-lm", str(tmp_path / "m.arpa")])
