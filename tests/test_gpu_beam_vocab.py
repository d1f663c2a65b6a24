"""The word-list constraint in the rec beam (retto_amd/csrc/ctc_vocab.h) on the MI355X: the device path (the row gather in chunks
of whole lines, the CTC FC GEMM, k_ctc_row_lse, k_ctc_beam_topc, k_ctc_beam_search's two vocabulary variants) through
rt_debug_ctc_beam_vocab against the fp64 restatement in ctc_vocab_ref.py, alone and with the order-3 model of ctc_lm_ref.
ctc_vocab_ref.check is ctc_lm_ref.check with the comparisons made on the closing score; it holds every hypothesis' oov_words to
the count by the direct definition, exactly.  test_beam_vocab_cpu.py runs the same checks on the host rule, measures the
tolerance there -- four times what the plain fp32 host loops deviate from fp64 on this grid (ctc_vocab_ref.MEASURED_HOST_*:
4.992e-4 up to 40 steps, 7.917e-4 on the line of 301 steps): TOL = 1.997e-3, TOL_LONG = 3.167e-3; the device is held to the same
figures, not measured on itself -- and asserts that at most 10 % of the ranks, and rank 0 on at most 5 % of the lines, are left
out of the string comparison (34 of 1602 ranks, no rank 0)."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lexicon_ref as LR
import ctc_lm_ref as MR
import ctc_vocab_ref as VR
from test_beam_vocab_cpu import check_prefix, check_rescue, check_ties, weights_of

pytestmark = pytest.mark.gpu
A, Bt, G = MR.ALPHA, MR.BETA, VR.GAMMA


def run_dev(sess, case, B, nbest, vocab, gamma=G, model=None, chunk=0, **kw):
    lib = _lib.load()
    rc, out = VR.call(lib.rt_debug_ctc_beam_vocab, sess._hd.h, *case, B, nbest, vocab, gamma, model, *weights_of(model), chunk=chunk, **kw)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_plain_dev(sess, case, B, nbest, chunk=0):
    lib = _lib.load()
    rc, out = BR.call(lib.rt_debug_ctc_beam, sess._hd.h, *case, B, nbest, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_lm_dev(sess, case, B, nbest, model, chunk=0):
    lib = _lib.load()
    rc, out = MR.call(lib.rt_debug_ctc_beam_lm, sess._hd.h, *case, B, nbest, model, A, Bt, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case, B, nbest, vocab, model=None):
    rc, out = VR.call(_lib.load().rt_debug_ctc_beam_vocab_host, None, *case, B, nbest, vocab, G, model, *weights_of(model))
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs, vocabulary and model per N; the fp64 rule per (N, model or not, beam) is computed on first use and shared
    by the chunkings"""
    g = {}
    for N in LR.GRID_N:
        case = BR.grid_case(N)
        g[N] = (case, VR.grid_vocab(N, case), MR.grid_model(N, VR.ORDER, case), {})
    return g


def ref_of(grid, N, fused, B):
    case, vocab, model, refs = grid[N]
    if (fused, B) not in refs:
        m = model if fused else None
        refs[(fused, B)] = VR.reference(*case, B, vocab, G, m, *weights_of(m))
    return refs[(fused, B)]


@pytest.mark.parametrize("chunk", [0, 1], ids=["default_chunks", "one_line_chunks"])
@pytest.mark.parametrize("B,nbest", BR.GRID_BEAMS)
@pytest.mark.parametrize("fused", [False, True], ids=["alone", "with_model"])
@pytest.mark.parametrize("N", LR.GRID_N)
def test_device_rule_against_fp64(hip_session, grid, N, fused, B, nbest, chunk):
    """chunk_rows = 1: every chunk takes its first line and no other"""
    case, vocab, model, _ = grid[N]
    tpl = case[3]
    m = model if fused else None
    out = run_dev(hip_session, case, B, nbest, vocab, model=m, chunk=chunk)
    st = VR.check(out, ref_of(grid, N, fused, B), tpl, N, B, nbest, VR.tol_of, vocab, G, m, *weights_of(m), what=(N, fused, B, nbest, chunk))
    print("N=%d model=%s beam=%d/%d chunk=%d: worst deviation %.3e up to 40 steps, %.3e on the long line; %d of %d ranks left out"
          % ((N, fused, B, nbest, chunk) + BR.worst_short_long(st) + (st["skipped"], st["ranks"])))
    assert st["lines"] == len(tpl) and out["n"].max() == nbest


@pytest.mark.parametrize("N", [5, 65])
def test_gamma_zero_is_the_device_beam_bit_for_bit(hip_session, grid, N):
    """gamma = 0 with any vocabulary: counts, tokens and logprob are rt_debug_ctc_beam's bytes and, with the model, those and the
    lm records rt_debug_ctc_beam_lm's"""
    case, vocab, model, _ = grid[N]
    for B, n in BR.GRID_BEAMS:
        for chunk in (0, 1):
            a = run_dev(hip_session, case, B, n, vocab, 0.0, chunk=chunk)
            p = run_plain_dev(hip_session, case, B, n, chunk=chunk)
            for k in ("n", "beams", "tokens"):
                assert a[k].tobytes() == p[k].tobytes(), (N, B, n, chunk, k)
            a = run_dev(hip_session, case, B, n, vocab, 0.0, model, chunk=chunk)
            p = run_lm_dev(hip_session, case, B, n, model, chunk=chunk)
            for k in ("n", "beams", "tokens", "lm"):
                assert a[k].tobytes() == p[k].tobytes(), (N, B, n, chunk, k, "model")


def test_rescue_case(hip_session):
    case, vocab = VR.rescue_case()
    out = run_dev(hip_session, case, 8, 4, vocab)
    check_rescue(run_plain_dev(hip_session, case, 8, 4), out, case)
    VR.check(out, VR.reference(*case, 8, vocab, G), case[3], VR.RESCUE_N, 8, 4, VR.tol_of, vocab, G)


def test_an_open_word_on_the_trie_is_not_counted(hip_session):
    case, vocab = VR.prefix_case()
    out = run_dev(hip_session, case, 1, 1, vocab)
    check_prefix(out, case, vocab)
    VR.check(out, VR.reference(*case, 1, vocab, G), case[3], 5, 1, 1, VR.tol_of, vocab, G)


@pytest.mark.parametrize("B", [2, 4])
def test_exact_ties_take_the_lower_id(hip_session, B):
    """classes bit-identical in the head and interchangeable in the trie (and identical in the model): the device's strings are
    the host rule's and the fp64 rule's with the same tie order, exactly"""
    case, vocab = BR.tie_case(), VR.tie_vocab()
    tpl = case[3]
    for m in (None, MR.tie_model()):
        ref = VR.reference(*case, B, vocab, G, m, *weights_of(m))
        host = VR.hyps_of(run_host(case, B, B, vocab, m), tpl, B, m is not None)
        for chunk in (0, 1):
            out = run_dev(hip_session, case, B, B, vocab, model=m, chunk=chunk)
            check_ties(out, ref, tpl, B, m is not None)
            dev = VR.hyps_of(out, tpl, B, m is not None)
            assert [[h[0] for h in hs] for hs in dev] == [[h[0] for h in hs] for hs in host]
            assert sum(h[k][5].tobytes() == h[k + 1][5].tobytes() for h in dev for k in range(len(h) - 1)) >= 2   # (ties are there)


@pytest.mark.parametrize("T", [1, 2, 7])
def test_words_longer_than_the_line(hip_session, T):
    """every entry is longer than the line, so every hypothesis that ends in a word class is open at the end -- on the trie or off
    it: the counts are the closing phase's; beams 1 and 32 at N = 5"""
    N = 5
    rng = np.random.default_rng(700 + T)
    W, b = BR.weights(rng, N)
    paths = [(T, LR.alignment(LR.random_entry(rng, N, max(1, T // 2), T), T)) for _ in range(4)] + [(T, None)] * 2
    z = LR.planted_features(rng, W.astype(np.float64), paths, gain=3.0, noise=1.5)
    case = (z, W, b, [T] * len(paths))
    texts = [R[0][0] for _lp, R in BR.reference(*case, 4) if R[0][0]]
    words = [tuple(c for c in s if c != 4) + tuple(int(x) for x in rng.integers(1, 4, T + 1)) for s in texts]
    words.append(tuple(int(x) for x in rng.integers(1, 4, T + 3)))
    vocab = VR.Vocab(N, words)
    assert min(len(w) for w in vocab.entries) > T and 4 not in vocab.word_classes
    closed_here = 0
    for B, n in ((1, 1), (4, 4), (32, 8)):
        ref = VR.reference(*case, B, vocab, G)
        closed_here += sum(r[4] > vocab.count(r[0], closed=False) for _lp, R in ref for r in R[:n])
        for chunk in (0, 1):
            VR.check(run_dev(hip_session, case, B, n, vocab, chunk=chunk), ref, case[3], N, B, n, VR.tol_of, vocab, G, what=(T, B, chunk))
    assert closed_here > 0      # (the line end closed words that were still on the trie)


def test_a_line_alone_and_nothing_at_all(hip_session, grid):
    case, vocab, model, _ = grid[65]
    z, W, b, tpl = case
    B, n = 16, 8
    out = VR.hyps_of(run_dev(hip_session, case, B, n, vocab, model=model), tpl, n, True)
    offs = np.concatenate([[0], np.cumsum(tpl)])
    for i in (tpl.index(40), tpl.index(7), len(tpl) - 1):
        alone = VR.hyps_of(run_dev(hip_session, (z[offs[i]:offs[i + 1]], W, b, [tpl[i]]), B, n, vocab, model=model), [tpl[i]], n, True)[0]
        assert [h[0] for h in alone] == [h[0] for h in out[i]], i
        assert max(abs(float(a[5]) - float(c[5])) for a, c in zip(alone, out[i])) <= 2 * VR.tol_of(tpl[i])
        assert [int(a[4]) for a in alone] == [int(c[4]) for c in out[i]]      # (the count depends on the string alone)
    for tp, beam in ((tpl, 0), ([], 4)):
        off = run_dev(hip_session, (z, W, b, tp), beam, 1, vocab, model=model)
        assert (off["n"] == BR.CANARY_N).all() and (off["beams"]["n_tokens"] == BR.CANARY_N).all() and (off["tokens"] == BR.CANARY_TOK).all()
        assert (off["lm"]["lm"] == MR.CANARY_LM).all() and (off["vocab"]["oov_words"] == VR.CANARY_OOV).all()
    for m in (None, model):
        none = run_dev(hip_session, (z, W, b, [0, 7, 0]), 4, 2, vocab, model=m)
        assert none["n"].tolist() == [0, 2, 0]
        VR.hyps_of(none, [0, 7, 0], 2, m is not None)
    none = run_dev(hip_session, (z, W, b, [0, 7, 0]), 4, 2, vocab, lm_null=True)      # (no model: lm_out may be NULL)
    assert none["n"].tolist() == [0, 2, 0]


def test_bad_arguments_are_rejected_before_any_launch(hip_session):
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f, h = lib.rt_debug_ctc_beam_vocab, hip_session._hd.h
    m = MR.Model(5, {(1,): (-1.0, -0.5), (2,): (-1.0, -0.5), (1, 2): (-0.5, 0.0)}, -9.0)
    v = VR.Vocab(5, [(1, 2), (3,)])
    wids, wlens = v.id_form()
    for kw, msg in ((dict(gamma=-0.5), b"gamma is not a finite number at least 0"), (dict(gamma=float("nan")), b"gamma is not"),
                    (dict(alpha=-0.5), b"alpha is not a finite number at least 0"),
                    (dict(word_form=(np.array([1, 0, 3]), wlens)), b"word 0: the blank (class 0) is not a token"),
                    (dict(word_form=(np.array([1, 2, 9]), wlens)), b"word 1: class id 9 is outside [1, 5)"),
                    (dict(word_form=(np.zeros(0, np.int32), np.zeros(0, np.int32))), b"no word at all"),
                    (dict(model=m, lm_null=True), b"a required pointer is null"),
                    (dict(B=33), b"beam = 33 is outside [0, RT_MAX_BEAM]"), (dict(n=5), b"nbest = 5 is outside"),
                    (dict(chunk=-1), b"chunk_rows is negative")):
        a = dict(B=4, n=2, gamma=1.0, alpha=0.0, model=None, word_form=None, lm_null=False, chunk=0)
        a.update(kw)
        if a["model"] is not None and a["alpha"] == 0.0:
            a["alpha"] = 0.5
        rc, out = VR.call(f, h, z, W, b, [4], a["B"], a["n"], v, a["gamma"], a["model"], a["alpha"], 0.0, chunk=a["chunk"],
                          word_form=a["word_form"], lm_null=a["lm_null"])
        assert rc == 8 and msg in lib.rt_last_error(h) and lib.rt_last_error(h).startswith(b"rt_debug_ctc_beam_vocab: "), (kw, lib.rt_last_error(h))
        assert (out["n"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all() and (out["vocab"]["oov_words"] == VR.CANARY_OOV).all()
