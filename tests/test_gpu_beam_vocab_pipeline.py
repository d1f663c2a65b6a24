"""The rec vocabulary inside the pipeline on the MI355X (rt_vocab_create, rt_set_rec_beam_vocab, rt_results_rec_beam_vocab): on
test_gpu_beam_pipeline.py's page and session.  A vocabulary that is created but not attached changes nothing; attached -- and with
a charset, a lexicon with snap, a pattern and a keyword list on the lines as well -- every other result, the per-stage JSON
included, is what it is without it, bit for bit, and only the beams differ.  Every hypothesis' oov_words is the count by the
direct definition (ctc_vocab_ref.Vocab.count) over its tokens and vocab_score = logprob (with a model: lm_score) - gamma *
oov_words; the hypotheses of a line are the same from rt_run_batch, rt_submit_batch / rt_wait_batch and rt_run_regions; the Python
fields mirror the C results."""
import ctypes as C

import numpy as np
import pytest

import retto_amd

import crop_source_cases as CS
import ctc_lm_ref as MR
import ctc_vocab_ref as VR
from test_gpu_beam_pipeline import BEAM, NBEST, beam_bits, session   # noqa: F401  (the fixture)
from test_gpu_charset_pipeline import reference_rows
from test_gpu_keywords_pipeline import kw_bits, others, stage_json
from test_gpu_lexicon_pipeline import variants
from test_gpu_pattern_pipeline import exact_pattern, same_but_det_scores

pytestmark = pytest.mark.gpu

GAMMA = 6.0
ALPHA, BETA = 0.8, 0.6


def f32b(x):
    return None if x is None else np.float32(x).tobytes()


def vocab_bits(r):
    return [None if g.beams is None else [(h.tokens.tolist(), h.text, f32b(h.logprob), f32b(h.lm_logprob), f32b(h.lm_score),
                                           h.oov_words, f32b(h.vocab_score)) for h in g.beams] for g in r.rec_result]


@pytest.fixture(scope="module")
def vocab(session):
    """a vocabulary around what the beams-only search reads: of every line its LAST hypothesis whole (so that a string the plain
    search ranks low is free of charge while the ones above it are one run that is no entry) and the first three ids of its best
    one (a prefix: entries inside longer runs); one word goes in as UTF-8 text, the rest as ids; created once"""
    s, c = session, session.case
    dic = s._dictionary()
    s.set_rec_beam(BEAM, NBEST)
    try:
        plain = s.run_regions([c["page"]], [c["B"]])[0]
    finally:
        s.set_rec_beam(0)
    words = []
    for g in plain.rec_result:
        last, best = g.beams[-1].tokens.tolist(), g.beams[0].tokens.tolist()
        words += [tuple(last[i:i + VR.MAX_LEN]) for i in range(0, len(last), VR.MAX_LEN)]
        if len(best) >= 3:
            words.append(tuple(best[:3]))
    words = [w for w in words if w]
    assert words
    text_word = next((w for w in words if all(len(dic[t]) == 1 and dic.index(dic[t]) == t and not dic[t].isspace() for t in w)), None)
    ids = [w for w in words if w != text_word] + [words[0]]          # (one word twice)
    v = s.create_vocab(words=["".join(dic[t] for t in text_word)] if text_word else (), ids=ids)
    ref = VR.Vocab(len(dic), ([text_word] if text_word else []) + ids)
    assert v == 0 and s.vocab_info(v) == {"words": len(ref.entries), "nodes": len(ref.node), "word_classes": len(ref.word_classes), "variants_dropped": 0}
    assert s.vocab_info(1) is None and s.vocab_info(-1) is None
    return ref, v


def check_worded_line(s, g, ref, T, what, gamma=GAMMA, model=None):
    dic = s._dictionary()
    assert g.beams is not None and 1 <= len(g.beams) <= NBEST, what
    assert len({tuple(h.tokens.tolist()) for h in g.beams}) == len(g.beams), what
    for a, b in zip(g.beams, g.beams[1:]):
        assert a.vocab_score >= b.vocab_score, (what, a, b)
    g32 = float(np.float32(gamma))
    for h in g.beams:
        assert len(h.tokens) <= T and all(1 <= c < len(dic) for c in h.tokens) and h.logprob <= VR.TOL, (what, h)
        assert h.text == "".join(dic[c] for c in h.tokens), (what, h)
        assert h.oov_words == ref.count(h.tokens.tolist()), (what, h, ref.count(h.tokens.tolist()))
        assert (h.lm_score is None) == (model is None), (what, h)
        base = h.logprob if model is None else h.lm_score
        if model is not None:
            assert abs(h.lm_logprob - model.lm64(h.tokens.tolist())) <= MR.tol_of(T), (what, h)
            assert abs(h.lm_score - MR.fused64(h.logprob, h.lm_logprob, len(h.tokens), ALPHA, BETA)) <= MR.tol_of(T), (what, h)
        mine = base - g32 * h.oov_words
        assert abs(h.vocab_score - mine) <= 4e-7 * (abs(base) + g32 * h.oov_words + 1.0), (what, h, mine)


def test_a_vocabulary_that_is_not_attached_changes_nothing(session, vocab):
    s, c = session, session.case
    page, B3 = c["page"], c["B3"]
    lib = s._hd.lib
    _ref, v = vocab
    assert s.rec_beam_vocab() == (-1, 0.0)
    s.set_rec_beam(BEAM, NBEST)
    try:
        want = s.run_regions([page], [B3])[0]
        assert all(h.oov_words is None and h.vocab_score is None for g in want.rec_result for h in g.beams)
        s.set_rec_beam_vocab(v, GAMMA)
        assert s.rec_beam_vocab() == (v, np.float32(GAMMA))
        s.set_rec_beam_vocab(-1)
        assert s.rec_beam_vocab() == (-1, 0.0)
        again = s.run_regions([page], [B3])[0]
        assert vocab_bits(again) == vocab_bits(want) and others(again) == others(want)
        r = s.run_regions_raw([page], [page.shape[0]], [page.shape[1]], [B3])
        try:
            for k in range(3):
                p = C.POINTER(retto_amd._lib.BeamVocab)()
                assert lib.rt_results_rec_beams(r, 0, k, None) >= 1 and lib.rt_results_rec_beam_vocab(r, 0, k, C.byref(p)) == 0 and not p
        finally:
            lib.rt_results_free(r)
        for bad, g in ((1, 1.0), (-2, 1.0), (v, -0.1), (v, float("nan")), (v, float("inf"))):
            with pytest.raises(retto_amd.InvalidArgument, match="rt_set_rec_beam_vocab"):
                s.set_rec_beam_vocab(bad, g)
        assert s.rec_beam_vocab() == (-1, 0.0)
    finally:
        s.set_rec_beam(0)
    # legal while beam = 0, and without effect until a beam is set
    s.set_rec_beam_vocab(v)
    try:
        assert s.rec_beam_vocab() == (v, 4.0)
        off = s.run_regions([page], [B3])[0]
        assert others(off) == others(c["ref3"]) and beam_bits(off) == [None] * 3
    finally:
        s.set_rec_beam_vocab(-1)


def test_attached_only_the_beams_differ(session, vocab):
    s, c = session, session.case
    page, B3, ref3 = c["page"], c["B3"], c["ref3"]
    ref, v = vocab
    rows = reference_rows(s, page, B3)
    T = [len(p) for p in rows]
    try:
        s.set_rec_beam(BEAM, NBEST)
        plain = s.run_regions([page], [B3])[0]
        s.set_rec_beam_vocab(v, GAMMA)
        worded = s.run_regions([page], [B3])[0]
        assert others(worded) == others(plain) == others(ref3), CS.differing(CS.digest(worded), CS.digest(ref3))
        for k in range(3):
            check_worded_line(s, worded.rec_result[k], ref, T[k], ("worded", k))
        assert beam_bits(worded) != beam_bits(plain)       # (the vocabulary bites)
        assert any(h.oov_words > 0 for g in worded.rec_result for h in g.beams) and any(h.oov_words == 0 for g in worded.rec_result for h in g.beams)
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
        with_v = s.run_regions([page], [B3], **opts)[0]
        json_on = stage_json(s, page, B3, **opts)
        s.set_rec_beam_vocab(-1)
        without = s.run_regions([page], [B3], **opts)[0]
        assert others(with_v) == others(without), CS.differing(CS.digest(with_v), CS.digest(without))
        assert kw_bits(with_v) == kw_bits(without) and json_on == stage_json(s, page, B3, **opts)
        assert CS.digest(without) != CS.digest(ref3)      # (the other options bite)
        # the beam reads the model's own distribution: the other options on the line change neither form of it
        assert vocab_bits(with_v) == vocab_bits(worded) and vocab_bits(without) == vocab_bits(plain)
    finally:
        s.set_rec_beam_vocab(-1)
        s.set_rec_beam(0)


def test_the_same_hypotheses_from_every_entry_point_and_the_python_mirror(session, vocab):
    s, c = session, session.case
    page, mp, B = c["page"], c["map"], c["B"]
    lib = s._hd.lib
    ref, v = vocab
    plain = CS.digest(s.run_batch([page], det_map_override=[mp])[0])
    s.set_rec_beam(BEAM, NBEST)
    s.set_rec_beam_vocab(v, GAMMA)
    try:
        a = s.run_batch([page], det_map_override=[mp])[0]
        want, wd = vocab_bits(a), CS.digest(a)
        assert all(w is not None for w in want) and wd == plain
        for k in range(6):
            check_worded_line(s, a.rec_result[k], ref, c["T"][k], ("batch", k))
        t = s.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[mp])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.set_rec_beam_vocab(-1)
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.create_vocab(ids=[[1, 2]])
        w = s.wait_batch(t)[0]
        assert vocab_bits(w) == want and CS.digest(w) == wd
        reg = s.run_regions([page], [B])[0]
        assert vocab_bits(reg) == want and same_but_det_scores(CS.digest(reg), wd)
        two = s.run_regions([page, page], [B, B[c["three"]]])
        assert vocab_bits(two[0]) == want
        # (three of the lines in a call of their own: another chunk, so the logits GEMM may round differently)
        for g, k in zip(two[1].rec_result, c["three"]):
            assert [h.tokens.tolist() for h in g.beams] == [h.tokens.tolist() for h in a.rec_result[k].beams], k
            assert [h.oov_words for h in g.beams] == [h.oov_words for h in a.rec_result[k].beams], k
            assert max(abs(x.vocab_score - y.vocab_score) for x, y in zip(g.beams, a.rec_result[k].beams)) <= 2 * VR.tol_of(c["T"][k])
        # the Python fields against the C results
        r = s.run_regions_raw([page], [page.shape[0]], [page.shape[1]], [B])
        try:
            for k in range(6):
                bp = C.POINTER(retto_amd._lib.Beam)(); vp = C.POINTER(retto_amd._lib.BeamVocab)()
                n = lib.rt_results_rec_beams(r, 0, k, C.byref(bp))
                assert n == len(reg.rec_result[k].beams) == lib.rt_results_rec_beam_vocab(r, 0, k, C.byref(vp))
                assert lib.rt_results_rec_beam_lm(r, 0, k, None) == 0
                for q in range(n):
                    h = reg.rec_result[k].beams[q]
                    assert f32b(bp[q].logprob) == f32b(h.logprob) and vp[q].oov_words == h.oov_words and f32b(vp[q].score) == f32b(h.vocab_score)
            assert lib.rt_results_rec_beam_vocab(r, 0, 6, None) == 0 and lib.rt_results_rec_beam_vocab(r, 1, 0, None) == 0
        finally:
            lib.rt_results_free(r)
        # gamma = 0: the beams-only hypotheses with the counts beside them
        s.set_rec_beam_vocab(v, 0.0)
        zero = s.run_regions([page], [B])[0]
        s.set_rec_beam_vocab(-1)
        only = s.run_regions([page], [B])[0]
        assert beam_bits(zero) == beam_bits(only)
        assert all(f32b(h.vocab_score) == f32b(h.logprob) and h.oov_words == ref.count(h.tokens.tolist()) for g in zero.rec_result for h in g.beams)
        # beside a language model: the key is the fused score minus gamma per word; rt_beam_lm holds no gamma
        dic = s._dictionary()
        m = MR.random_model(78, len(dic), 3, [tuple(int(t) for t in g.tokens) for g in c["ref"].rec_result], per_level=300)
        lm = s.create_lm(MR.write_arpa(m, dic), oov_log10=m.oov / MR.LN10)
        s.set_rec_beam_lm(lm, ALPHA, BETA)
        s.set_rec_beam_vocab(v, GAMMA)
        both = s.run_regions([page], [B])[0]
        for k in range(6):
            check_worded_line(s, both.rec_result[k], ref, c["T"][k], ("both", k), model=m)
        s.set_rec_beam_vocab(v, 0.0)
        zero = s.run_regions([page], [B])[0]
        s.set_rec_beam_vocab(-1)
        lm_only = s.run_regions([page], [B])[0]
        strip = lambda r: [[x[:5] for x in g] for g in vocab_bits(r)]
        assert strip(zero) == strip(lm_only)
    finally:
        s.set_rec_beam_vocab(-1)
        s.set_rec_beam_lm(-1)
        s.set_rec_beam(0)
    after = s.run_batch([page], det_map_override=[mp])[0]
    assert CS.digest(after) == plain and all(g.beams is None for g in after.rec_result)


def test_the_session_holds_four_vocabularies(session, vocab):
    s = session
    with pytest.raises(retto_amd.InvalidArgument, match=r"rt_vocab_create: vocab: id word 1: the blank \(class 0\) is not a token"):
        s.create_vocab(ids=[[1, 2], [3, 0]])
    with pytest.raises(retto_amd.InvalidArgument, match="rt_vocab_create: vocab: no word at all"):
        s.create_vocab()
    while s.vocab_info(VR.MAX_VOCABS - 1) is None:
        s.create_vocab(ids=[[1, 2], [1]])
    with pytest.raises(retto_amd.CapacityError, match="RT_MAX_VOCABS"):
        s.create_vocab(ids=[[1, 2]])
    assert s.vocab_info(3) == {"words": 2, "nodes": 3, "word_classes": 2, "variants_dropped": 0}


def test_cli_vocab_flags(tmp_path, session, monkeypatch):
    """--rec-vocab FILE with --rec-beam gives every hypothesis oov_words and vocab_score = logprob - G oov_words, the count being
    the definition's over the words of the file and their case variants; --rec-vocab without --rec-beam exits with a message.
    (The synthetic detector finds nothing on its own: the CLI's run_batch gets the planted det maps, as every pipeline test here
    hands them in.)"""
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
    out = tmp_path / "out.jsonl"
    base = ["--images", str(img), "--synthetic", "--batch", "2", "--json", str(out)]
    assert cli.main(base + ["--rec-beam", "8,2"]) == 0
    plain = [json.loads(l) for l in open(out)]
    assert sum(len(l["rec"]) for l in plain) >= 1
    # the words of the file: the first three ids of every best hypothesis whose characters the compiler maps back to them
    ok = lambda t: len(dic[t]) == 1 and dic.index(dic[t]) == t and not dic[t].isspace()
    words = sorted({tuple(b[0]["tokens"][:3]) for l in plain for b in l["beams"] if len(b[0]["tokens"]) >= 3 and all(ok(t) for t in b[0]["tokens"][:3])})
    words = words or [tuple(t for t in range(1, len(dic)) if ok(t))[:2]]
    (tmp_path / "w.txt").write_bytes(("\n".join("".join(dic[t] for t in w) for w in words) + "\n").encode("utf-8"))
    assert cli.main(base + ["--rec-beam", "8,2", "--rec-vocab", str(tmp_path / "w.txt"), "--rec-vocab-gamma", "2.5"]) == 0
    worded = [json.loads(l) for l in open(out)]
    ref = VR.Vocab(len(dic), words)
    assert [l["rec"] for l in worded] == [l["rec"] for l in plain]
    for l in worded:
        for b in l["beams"]:
            for h in b:
                assert set(h) == {"text", "tokens", "logprob", "oov_words", "vocab_score"}
                assert h["oov_words"] == ref.count(h["tokens"]) and abs(h["vocab_score"] - (h["logprob"] - 2.5 * h["oov_words"])) <= 1e-4
    assert cli.main(base + ["--rec-beam", "8,2", "--rec-vocab", str(tmp_path / "w.txt"), "--rec-vocab-case-variants"]) == 0
    assert all("oov_words" in h for l in map(json.loads, open(out)) for b in l["beams"] for h in b)
    with pytest.raises(SystemExit, match="--rec-vocab needs --rec-beam"):
        cli.main(base + ["--rec-vocab", str(tmp_path / "w.txt")])
