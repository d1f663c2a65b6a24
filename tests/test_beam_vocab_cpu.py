"""The word-list constraint in the rec beam (retto_amd/csrc/ctc_vocab.h, ctc_beam.h) without a GPU: the host rule in plain fp32
loops (rt_debug_ctc_beam_vocab_host) against the fp64 restatement of ctc_vocab_ref.py on the grid of test_gpu_beam_vocab.py, alone
and with the order-3 model, by that test's own checker -- this is where the tolerance is measured; gamma = 0 as the plain and the
fused beam's bytes; the rescue case, the open-prefix case, the exact tie case; the checker against the mutants it must refuse;
and what the arguments are held to."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lexicon_ref as LR
import ctc_lm_ref as MR
import ctc_vocab_ref as VR

A, Bt, G = MR.ALPHA, MR.BETA, VR.GAMMA


def run_host(case, B, nbest, vocab, gamma=G, model=None, alpha=None, beta=None, **kw):
    alpha, beta = ((A, Bt) if model is not None else (0.0, 0.0)) if alpha is None else (alpha, beta)
    rc, out = VR.call(_lib.load().rt_debug_ctc_beam_vocab_host, None, *case, B, nbest, vocab, gamma, model, alpha, beta, **kw)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


def run_plain(case, B, nbest):
    rc, out = BR.call(_lib.load().rt_debug_ctc_beam_host, None, *case, B, nbest)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


def run_lm(case, B, nbest, model, alpha=A, beta=Bt):
    rc, out = MR.call(_lib.load().rt_debug_ctc_beam_lm_host, None, *case, B, nbest, model, alpha, beta)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


def weights_of(m):
    return (A, Bt) if m is not None else (0.0, 0.0)


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs, its vocabulary and its model per N and the fp64 rule per (N, with the model or not, beam), computed once"""
    g = {}
    for N in LR.GRID_N:
        case = BR.grid_case(N)
        vocab, model = VR.grid_vocab(N, case), MR.grid_model(N, VR.ORDER, case)
        g[N] = (case, vocab, model, {(fused, B): VR.reference(*case, B, vocab, G, model if fused else None, *weights_of(model if fused else None))
                                     for fused in (False, True) for B, _ in BR.GRID_BEAMS})
    return g


# ---------------------------------------------------------------- the rule
def test_host_rule_on_the_grid_against_fp64(grid):
    """every check of the GPU test on the host rule; the figures the tolerances are four times of are measured here again; and
    the condition on the ranks left out of the string comparison is asserted on the fp64 rule's own gaps (check() decides what
    is left out from the reference alone), merged over the grid as the plain beam's test merges it"""
    stats = []
    for N in LR.GRID_N:
        case, vocab, model, refs = grid[N]
        tpl = case[3]
        assert all(not VR.is_grid_separator(c) for c in vocab.word_classes)
        for fused in (False, True):
            m = model if fused else None
            for B, n in BR.GRID_BEAMS:
                out = run_host(case, B, n, vocab, model=m)
                st = VR.check(out, refs[(fused, B)], tpl, N, B, n, VR.tol_of, vocab, G, m, *weights_of(m), what=("host", N, fused, B, n))
                print("host fp32 against fp64, N = %d, model %s, beam %d / %d: %.3e up to 40 steps, %.3e on the long line; %d of %d ranks left out"
                      % ((N, fused, B, n) + BR.worst_short_long(st) + (st["skipped"], st["ranks"])))
                stats.append(st)
    st = BR.merge_stats(stats)
    short, long_ = BR.worst_short_long(st)
    print("merged: %.4e, %.4e; %d of %d ranks left out, rank 0 on %d of %d lines" % (short, long_, st["skipped"], st["ranks"], st["rank0_skipped"], st["lines"]))
    assert short <= VR.MEASURED_HOST_SHORT * 1.001 and long_ <= VR.MEASURED_HOST_LONG * 1.001, (short, long_)
    assert VR.TOL == 4 * VR.MEASURED_HOST_SHORT and VR.TOL_LONG == 4 * VR.MEASURED_HOST_LONG
    assert BR.condition_holds(st), st
    assert st["ranks"] > 1200 and st["lines"] == 2 * 3 * 4 * 13


def test_the_vocabulary_changes_the_grid_and_reaches_every_row_of_the_step_table(grid):
    """the grid is no plain beam in disguise: at N = 65 the fp64 rule's best string differs from the plain rule's on several lines, and its
    hypotheses hold entries, words that are none, separators, and last words that the line end closes"""
    closed_by_end = 0
    for N in (5, 65, 6625):
        case, vocab, _model, refs = grid[N]
        plain = BR.reference(*case, 16)
        R = refs[(False, 16)]
        if N == 65:   # (at N = 5 and 6625 the lines' best strings stand too clear of the rest for gamma to move them)
            assert sum(1 for (_l, a), (_l2, p) in zip(R, plain) if a and a[0][0] != p[0][0]) >= 2, N
        entries = nonwords = seps = 0
        for _lp, hyps in R:
            for s, _v, _lm, _f, closed, _sc in hyps[:8]:
                runs, open_ = vocab.runs(s)
                entries += sum(r in vocab.entries for r in runs)
                nonwords += sum(r not in vocab.entries for r in runs)
                seps += sum(c not in vocab.word_classes for c in s)
                closed_by_end += open_ and closed > vocab.count(s, closed=False)
        assert entries > 0 and nonwords > 0 and seps > 0, (N, entries, nonwords, seps)
    assert closed_by_end > 0


def test_gamma_zero_is_the_plain_and_the_fused_beam_bit_for_bit(grid):
    """gamma = 0 with any vocabulary: counts, tokens, logprob (and, with a model, lm and its score) equal rt_debug_ctc_beam_host's
    and rt_debug_ctc_beam_lm_host's bytes; oov_words is still the definition's and score the fused score"""
    for N in (5, 65):
        case, vocab, model, _refs = grid[N]
        tpl = case[3]
        for B, n in BR.GRID_BEAMS:
            for m in (None, model):
                a = run_host(case, B, n, vocab, 0.0, m)
                p = run_plain(case, B, n) if m is None else run_lm(case, B, n, m)
                for k in ("n", "beams", "tokens") + (("lm",) if m is not None else ()):
                    assert a[k].tobytes() == p[k].tobytes(), (N, B, n, k, m is not None)
                for H in VR.hyps_of(a, tpl, n, m is not None):
                    for s, v, _lm, lsc, oov, sc in H:
                        assert int(oov) == vocab.count(s) and sc.tobytes() == (v if m is None else lsc).tobytes()


def check_rescue(plain_out, vocab_out, case):
    tpl = case[3]
    assert BR.hyps_of(plain_out, tpl, 4)[0][0][0] == VR.RESCUE_WRONG
    H = VR.hyps_of(vocab_out, tpl, 4, False)[0]
    assert H[0][0] == VR.RESCUE_WORD and int(H[0][4]) == 0
    wrong = [h for h in H if h[0] == VR.RESCUE_WRONG]
    assert not wrong or int(wrong[0][4]) == 1


def test_rescue_case():
    """the evidence alone reads a non-word one class away from an entry; the vocabulary's rank 0 is the entry; both gaps stand
    clear in fp64"""
    case, vocab = VR.rescue_case()
    P = BR.reference(*case, 8)[0][1]
    assert P[0][0] == VR.RESCUE_WRONG and P[1][0] == VR.RESCUE_WORD and P[0][1] - P[1][1] > 100 * BR.TOL
    assert vocab.count(VR.RESCUE_WRONG) == 1 and vocab.count(VR.RESCUE_WORD) == 0
    R = VR.reference(*case, 8, vocab, G)[0][1]
    assert R[0][0] == VR.RESCUE_WORD and R[0][5] - R[1][5] > 100 * VR.TOL
    out = run_host(case, 8, 4, vocab)
    check_rescue(run_plain(case, 8, 4), out, case)
    VR.check(out, VR.reference(*case, 8, vocab, G), case[3], VR.RESCUE_N, 8, 4, VR.tol_of, vocab, G)


def check_prefix(out, case, vocab):
    H = VR.hyps_of(out, case[3], 1, False)[0]
    assert H[0][0] == (1, 2) and int(H[0][4]) == 0, H


def test_an_open_word_on_the_trie_is_not_counted():
    """beam 1: the open prefix (1) must survive the separator that stands 0.5 below it, or the entry (1, 2) is never read"""
    case, vocab = VR.prefix_case()
    R = VR.reference(*case, 1, vocab, G)[0][1]
    assert R[0][0] == (1, 2) and R[0][4] == 0
    out = run_host(case, 1, 1, vocab)
    check_prefix(out, case, vocab)
    VR.check(out, VR.reference(*case, 1, vocab, G), case[3], 5, 1, 1, VR.tol_of, vocab, G)


def check_ties(out, ref, tpl, nbest, fused):
    """the exact tie rule: every string is the fp64 rule's with the same tie order"""
    H = VR.hyps_of(out, tpl, nbest, fused)
    assert [[h[0] for h in hs] for hs in H] == [[r[0] for r in R[:nbest]] for _lp, R in ref]


@pytest.mark.parametrize("B", [2, 4])
def test_exact_ties_take_the_lower_id(B):
    """classes that are bit-identical in the head AND interchangeable in the trie still resolve to the lower id, alone and with a
    model in which they are identical too"""
    case, vocab = BR.tie_case(), VR.tie_vocab()
    tpl = case[3]
    for lo, hi in BR.TIE_PAIRS:
        swap = lambda w: tuple(hi if c == lo else lo if c == hi else c for c in w)
        assert all(swap(w) in vocab.entries for w in vocab.entries)
    for m in (None, MR.tie_model()):
        out = run_host(case, B, B, vocab, model=m)
        check_ties(out, VR.reference(*case, B, vocab, G, m, *weights_of(m)), tpl, B, m is not None)
        n_ties = 0
        for h in VR.hyps_of(out, tpl, B, m is not None):
            for k in range(len(h) - 1):
                if h[k][5].tobytes() == h[k + 1][5].tobytes():    # (bit-equal scores: the lower id first)
                    assert h[k][0] < h[k + 1][0] and int(h[k][4]) == int(h[k + 1][4]), h
                    n_ties += 1
        assert n_ties >= 2, (B, m is not None, n_ties)


def test_stand_in_is_the_rule_and_every_mutant_is_caught(grid):
    res, resv = VR.rescue_case()
    pre, prev = VR.prefix_case()
    small, sv, _sm, small_refs = grid[5]
    mid, mv, mm, mid_refs = grid[65]
    cases = [(lambda o: check_rescue(run_plain(res, 8, 4), o, res), (res, 8, 4, resv, None)),
             (lambda o: check_prefix(o, pre, prev), (pre, 1, 1, prev, None)),
             (lambda o: VR.check(o, small_refs[(False, 16)], small[3], 5, 16, 8, VR.tol_of, sv, G), (small, 16, 8, sv, None)),
             (lambda o: VR.check(o, mid_refs[(True, 4)], mid[3], 65, 4, 4, VR.tol_of, mv, G, mm, A, Bt), (mid, 4, 4, mv, mm))]
    for chk, (case, B, n, v, m) in cases:
        chk(VR.stand_in(*case, B, n, v, G, m, *weights_of(m)))
    caught_by = {}
    for mut in VR.MUTANTS:
        for k, (chk, (case, B, n, v, m)) in enumerate(cases):
            try:
                chk(VR.stand_in(*case, B, n, v, G, m, *weights_of(m), mutant=mut))
            except AssertionError:
                caught_by.setdefault(mut, []).append(k)
        assert caught_by.get(mut), mut
    # ... and, the open-word mutant aside (only its own case prunes the entry's prefix away), by the grid cases, whose checker is
    # the GPU test's
    for mut in VR.MUTANTS:
        assert mut == "open_word_counted" or any(k >= 2 for k in caught_by[mut]), (mut, caught_by[mut])


def test_checker_refuses_a_wrong_count_a_wrong_score_and_a_written_canary(grid):
    case, vocab, _model, refs = grid[65]
    tpl = case[3]
    good = run_host(case, 4, 4, vocab)
    i = tpl.index(40)
    rec = good["vocab"][i][0]
    assert good["n"][i] == 4
    for key, at, val in (("vocab", (i, 0), (rec["oov_words"] + 1, rec["score"])), ("vocab", (i, 0), (rec["oov_words"], np.float32(rec["score"] + 0.05))),
                         ("lm", (i, 0), (np.float32(0.0), np.float32(0.0))), ("n", i, 3)):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][at] = val
        with pytest.raises(AssertionError):
            VR.check(bad, refs[(False, 4)], tpl, 65, 4, 4, VR.tol_of, vocab, G)


# ---------------------------------------------------------------- arguments
def test_host_entry_rejects_bad_arguments_and_off_writes_nothing():
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f = lib.rt_debug_ctc_beam_vocab_host
    m = MR.Model(5, {(1,): (-1.0, -0.5), (2,): (-1.0, -0.5), (1, 2): (-0.5, 0.0)}, -9.0)
    v = VR.Vocab(5, [(1, 2), (3,)])
    wids, wlens = v.id_form()
    untouched = lambda out: ((out["n"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all() and (out["lm"]["lm"] == MR.CANARY_LM).all() and
                             (out["beams"]["n_tokens"] == BR.CANARY_N).all() and (out["vocab"]["oov_words"] == VR.CANARY_OOV).all())
    for kw, msg in ((dict(gamma=-0.5), b"gamma is not a finite number at least 0"), (dict(gamma=float("nan")), b"gamma is not"),
                    (dict(gamma=float("inf")), b"gamma is not"), (dict(alpha=-0.5), b"alpha is not a finite number at least 0"),
                    (dict(beta=float("nan")), b"beta is not finite"),
                    (dict(word_form=(np.array([1, 0, 3]), wlens)), b"word 0: the blank (class 0) is not a token"),
                    (dict(word_form=(np.array([1, 2, 5]), wlens)), b"word 1: class id 5 is outside [1, 5)"),
                    (dict(word_form=(wids, np.array([3, 0]))), b"word 1 is empty"),
                    (dict(word_form=(np.ones(64, np.int32), np.array([64]))), b"word 0 has 64 ids, more than RT_VOCAB_MAX_LEN (63)"),
                    (dict(word_form=(np.zeros(0, np.int32), np.zeros(0, np.int32))), b"no word at all"),
                    (dict(model=m, lm_null=True), b"a required pointer is null"),
                    (dict(B=33), b"beam = 33 is outside [0, RT_MAX_BEAM]"), (dict(n=5), b"nbest = 5 is outside"),
                    (dict(tpl=[-4]), b"line 0 has a negative number of time steps")):
        a = dict(tpl=[4], B=4, n=2, gamma=1.0, alpha=0.0, beta=0.0, model=None, word_form=None, lm_null=False)
        a.update(kw)
        if a["model"] is not None and a["alpha"] == 0.0:
            a["alpha"] = 0.5
        rc, out = VR.call(f, None, z, W, b, a["tpl"], a["B"], a["n"], v, a["gamma"], a["model"], a["alpha"], a["beta"], word_form=a["word_form"],
                          lm_null=a["lm_null"])
        assert rc == 8 and msg in lib.rt_last_error(None) and lib.rt_last_error(None).startswith(b"rt_debug_ctc_beam_vocab_host: "), (kw, lib.rt_last_error(None))
        assert untouched(out)
    rc, out = VR.call(f, None, z, W, b, [4], 0, 3, v, 1.0)           # beam = 0: off
    assert rc == 0 and untouched(out)
    rc, out = VR.call(f, None, z, W, b, [], 4, 2, v, 1.0)            # no line
    assert rc == 0 and untouched(out)
    rc, out = VR.call(f, None, z, W, b, [0, 4, 0], 4, 2, v, 1.0)     # lines without a time step report no hypothesis
    assert rc == 0 and out["n"].tolist() == [0, 2, 0]
    VR.hyps_of(out, [0, 4, 0], 2, False)
    rc, out = VR.call(f, None, z, W, b, [4], 4, 2, v, 1.0, lm_null=True)   # no model: lm_out may be NULL
    assert rc == 0 and out["n"].tolist() == [2]
    for s, _v, _lm, _lsc, oov, _sc in VR.hyps_of(out, [4], 2, False)[0]:
        assert int(oov) == v.count(s)
