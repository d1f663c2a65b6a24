"""Language-model fusion in the rec beam (retto_amd/csrc/ctc_lm.h, ctc_beam.h) without a GPU: the host rule in plain fp32 loops
(rt_debug_ctc_beam_lm_host) against the fused fp64 restatement of ctc_lm_ref.py on the grid of test_gpu_beam_lm.py, by that
test's own checker -- this is where the tolerance is measured; alpha = beta = 0 as the plain beam's bytes; the exhaustive case,
the exact tie case, the rescue case; the checker against the mutants it must refuse; and what the arguments are held to."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lexicon_ref as LR
import ctc_lm_ref as MR


def run_host(case, B, nbest, model, alpha=MR.ALPHA, beta=MR.BETA):
    rc, out = MR.call(_lib.load().rt_debug_ctc_beam_lm_host, None, *case, B, nbest, model, alpha, beta)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


def run_plain(case, B, nbest):
    rc, out = BR.call(_lib.load().rt_debug_ctc_beam_host, None, *case, B, nbest)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs, its two models per N and the fused fp64 rule per (N, order, beam), computed once"""
    g = {}
    for N in LR.GRID_N:
        case = BR.grid_case(N)
        models = {order: MR.grid_model(N, order, case) for order in MR.ORDERS}
        g[N] = (case, models, {(order, B): MR.reference(*case, B, models[order], MR.ALPHA, MR.BETA) for order in MR.ORDERS for B, _ in BR.GRID_BEAMS})
    return g


# ---------------------------------------------------------------- the rule
def test_host_rule_on_the_grid_against_fp64(grid):
    """every check of the GPU test on the host rule; the figures the tolerances are four times of are measured here again; and
    the condition on the ranks left out of the string comparison is asserted on the fp64 rule's own fused gaps (check() decides
    what is left out from the reference alone), merged over the grid as the plain beam's test merges it"""
    stats = []
    for N in LR.GRID_N:
        case, models, refs = grid[N]
        tpl = case[3]
        for order in MR.ORDERS:
            m = models[order]
            assert m.order == order and any((c,) not in m.ngrams for c in range(1, N))
            for B, n in BR.GRID_BEAMS:
                st = MR.check(run_host(case, B, n, m), refs[(order, B)], tpl, N, B, n, MR.tol_of, m, MR.ALPHA, MR.BETA, what=("host", N, order, B, n))
                print("host fp32 against fp64, N = %d, order %d, beam %d / %d: %.3e up to 40 steps, %.3e on the long line; %d of %d ranks left out"
                      % ((N, order, B, n) + BR.worst_short_long(st) + (st["skipped"], st["ranks"])))
                stats.append(st)
    st = BR.merge_stats(stats)
    short, long_ = BR.worst_short_long(st)
    print("merged: %.4e, %.4e; %d of %d ranks left out, rank 0 on %d of %d lines" % (short, long_, st["skipped"], st["ranks"], st["rank0_skipped"], st["lines"]))
    assert short <= MR.MEASURED_HOST_SHORT * 1.001 and long_ <= MR.MEASURED_HOST_LONG * 1.001, (short, long_)
    assert MR.TOL == 4 * MR.MEASURED_HOST_SHORT and MR.TOL_LONG == 4 * MR.MEASURED_HOST_LONG
    assert BR.condition_holds(st), st
    assert st["ranks"] > 1200 and st["lines"] == 2 * 3 * 4 * 13


def test_fusion_changes_the_grid_and_reaches_the_model(grid):
    """the grid is no plain beam in disguise: on most lines the fused fp64 rule's best string is not the plain rule's, its
    hypotheses hold classes without a unigram, and their tokens were scored at every back-off depth of both orders"""
    for N in (65, 6625):
        case, models, refs = grid[N]
        plain = BR.reference(*case, 16)
        for order in MR.ORDERS:
            m, R = models[order], refs[(order, 16)]
            assert sum(1 for (_l, a), (_l2, p) in zip(R, plain) if a and a[0][0] != p[0][0]) >= 3
            depth, oov = set(), 0
            for _lp, hyps in R:
                for s, _v, _lm, _f in hyps[:8]:
                    h = (m.bos,) + s
                    for i in range(1, len(h)):
                        ctx = h[max(i - (order - 1), 0):i]
                        k = 0
                        while ctx + (h[i],) not in m.ngrams and ctx:
                            ctx = ctx[1:]; k += 1
                        depth.add(k)
                        oov += (h[i],) not in m.ngrams
            assert depth == set(range(order)) and oov > 0, (N, order, depth, oov)


def test_zero_weights_are_the_plain_beam_bit_for_bit(grid):
    """alpha = beta = 0 with any model: counts, tokens and logprob equal rt_debug_ctc_beam_host's bytes; lm is still the model's"""
    for N in (5, 65):
        case, models, _refs = grid[N]
        tpl = case[3]
        for order in MR.ORDERS:
            for B, n in BR.GRID_BEAMS:
                a, p = run_host(case, B, n, models[order], 0.0, 0.0), run_plain(case, B, n)
                for k in ("n", "beams", "tokens"):
                    assert a[k].tobytes() == p[k].tobytes(), (N, order, B, n, k)
                for H in MR.hyps_of(a, tpl, n):
                    for s, v, lm, sc in H:
                        assert sc.tobytes() == v.tobytes() and abs(float(lm) - models[order].lm64(s)) <= MR.TOL


EXHAUSTIVE_SEED = 0      # chosen so that the fused top-8 gaps exceed 100 tol (asserted first)


def exhaustive_inputs(seed=EXHAUSTIVE_SEED):
    case = BR.exhaustive_case(seed)
    return case, MR.random_model(900 + seed, 3, 3, texts=[(1, 2, 2, 1), (2, 1)])


def exhaustive_order(case, m):
    z, W, b, _tpl = case
    lp = LR.logp64(LR.logits64(z, W, b))
    strings = BR.all_strings(2, 4)
    ll = {s: BR.loglik64(lp, s) for s in strings}
    fused = {s: MR.fused64(ll[s], m.lm64(s), len(s), MR.ALPHA, MR.BETA) for s in strings if ll[s] > -np.inf}
    return ll, fused, sorted(fused, key=lambda s: -fused[s])


def check_exhaustive(out, case, m):
    ll, fused, order = exhaustive_order(case, m)
    H = MR.hyps_of(out, case[3], 8)[0]
    assert [h[0] for h in H] == order[:8], (H, order[:8])
    for s, v, lm, sc in H:
        assert abs(float(v) - ll[s]) <= MR.TOL and abs(float(sc) - fused[s]) <= MR.TOL and abs(float(lm) - m.lm64(s)) <= MR.TOL


def test_exhaustive_case_is_the_sort_of_the_fused_full_likelihoods():
    """classes = 3, T = 4, beam 32: the beam holds every string that has an alignment, so the result is the sort of (full
    likelihood + alpha lm + beta len) over all 31 strings, whatever the order the selection saw them in"""
    case, m = exhaustive_inputs()
    ll, fused, order = exhaustive_order(case, m)
    assert len(ll) == 31 <= BR.MAX_BEAM
    gaps = [fused[order[k]] - fused[order[k + 1]] for k in range(BR.MAX_NBEST)]
    assert min(gaps) > 100 * MR.TOL, gaps
    plain = sorted(fused, key=lambda s: -ll[s])
    assert plain[:8] != order[:8]                       # (the model changes the answer)
    out = run_host(case, 32, 8, m)
    check_exhaustive(out, case, m)
    MR.check(out, MR.reference(*case, 32, m, MR.ALPHA, MR.BETA), case[3], 3, 32, 8, MR.tol_of, m, MR.ALPHA, MR.BETA)
    # the fused fp64 restatement itself, against the definition
    R = {s: (v, f) for s, v, _lm, f in MR.beam_lm64(LR.logits64(*case[:3]), 32, m, MR.ALPHA, MR.BETA)}
    assert set(R) == set(fused) and max(abs(R[s][1] - fused[s]) for s in R) < 1e-9


def check_ties(out, ref, tpl, nbest):
    """the exact tie rule: every string is the fused fp64 rule's with the same tie order"""
    H = MR.hyps_of(out, tpl, nbest)
    assert [[h[0] for h in hs] for hs in H] == [[r[0] for r in R[:nbest]] for _lp, R in ref]


@pytest.mark.parametrize("B", [2, 4])
def test_exact_ties_take_the_lower_id(B):
    """classes that are bit-identical in the head AND in the model still resolve to the lower id"""
    case, m = BR.tie_case(), MR.tie_model()
    tpl = case[3]
    for lo, hi in BR.TIE_PAIRS:
        assert m.ngrams[(lo,)] == m.ngrams[(hi,)]
        assert all(m.ngrams.get((a, lo)) == m.ngrams.get((a, hi)) and m.ngrams.get((lo, a)) == m.ngrams.get((hi, a)) for a in range(1, 10))
    out = run_host(case, B, B, m)
    check_ties(out, MR.reference(*case, B, m, MR.ALPHA, MR.BETA), tpl, B)
    n_ties = 0
    for h in MR.hyps_of(out, tpl, B):
        for k in range(len(h) - 1):
            if h[k][3].tobytes() == h[k + 1][3].tobytes():    # (bit-equal fused scores: the lower id first)
                assert h[k][0] < h[k + 1][0] and h[k][2].tobytes() == h[k + 1][2].tobytes(), h
                n_ties += 1
    assert n_ties >= 2


def check_rescue(plain_out, fused_out, case, m):
    tpl = case[3]
    assert BR.hyps_of(plain_out, tpl, 4)[0][0][0] == MR.RESCUE_WRONG
    assert MR.hyps_of(fused_out, tpl, 4)[0][0][0] == MR.RESCUE_STRING


def test_rescue_case():
    """the acoustic evidence puts a wrong class narrowly first at one step: the plain beam reads the wrong string, the beam with a
    model built from the planted string reads the planted one; both gaps stand clear in fp64"""
    case, m = MR.rescue_case()
    P = BR.reference(*case, 8)[0][1]
    assert P[0][0] == MR.RESCUE_WRONG and P[1][0] == MR.RESCUE_STRING and P[0][1] - P[1][1] > 100 * BR.TOL
    R = MR.reference(*case, 8, m, MR.ALPHA, MR.BETA)[0][1]
    assert R[0][0] == MR.RESCUE_STRING and R[0][3] - R[1][3] > 100 * MR.TOL
    wrong = [r for r in R if r[0] == MR.RESCUE_WRONG]
    assert not wrong or R[0][3] - wrong[0][3] > 100 * MR.TOL
    check_rescue(run_plain(case, 8, 4), run_host(case, 8, 4, m), case, m)
    MR.check(run_host(case, 8, 4, m), MR.reference(*case, 8, m, MR.ALPHA, MR.BETA), case[3], MR.RESCUE_N, 8, 4, MR.tol_of, m, MR.ALPHA, MR.BETA)


def test_stand_in_is_the_rule_and_every_mutant_is_caught(grid):
    ex, exm = exhaustive_inputs()
    tie, tiem = BR.tie_case(), MR.tie_model()
    small, models, small_refs = grid[5]
    mid, mid_models, mid_refs = grid[65]
    A, Bt = MR.ALPHA, MR.BETA
    cases = [(lambda o: check_exhaustive(o, ex, exm), (ex, 32, 8, exm)),
             (lambda o: check_ties(o, MR.reference(*tie, 4, tiem, A, Bt), tie[3], 4), (tie, 4, 4, tiem)),
             (lambda o: MR.check(o, small_refs[(5, 16)], small[3], 5, 16, 8, MR.tol_of, models[5], A, Bt), (small, 16, 8, models[5])),
             (lambda o: MR.check(o, mid_refs[(3, 4)], mid[3], 65, 4, 4, MR.tol_of, mid_models[3], A, Bt), (mid, 4, 4, mid_models[3]))]
    for chk, (case, B, n, m) in cases:
        chk(MR.stand_in(*case, B, n, m, A, Bt))
    for mut in MR.MUTANTS:
        caught = 0
        for chk, (case, B, n, m) in cases:
            try:
                chk(MR.stand_in(*case, B, n, m, A, Bt, mutant=mut))
            except AssertionError:
                caught += 1
        assert caught >= 1, mut
    # ... and by the grid cases, whose checker is the GPU test's
    for mut in MR.MUTANTS:
        hit = 0
        for chk, (case, B, n, m) in cases[2:]:
            try:
                chk(MR.stand_in(*case, B, n, m, A, Bt, mutant=mut))
            except AssertionError:
                hit += 1
        assert hit >= 1, mut


def test_checker_refuses_a_wrong_lm_a_wrong_score_and_a_written_canary(grid):
    case, models, refs = grid[65]
    tpl = case[3]
    m = models[3]
    good = run_host(case, 4, 4, m)
    i = tpl.index(40)
    rec = good["lm"][i][0]
    assert good["n"][i] == 4
    for key, at, val in (("lm", (i, 0), (np.float32(rec["lm"] + 0.05), rec["score"])), ("lm", (i, 0), (rec["lm"], np.float32(rec["score"] + 0.05))),
                         ("lm", (i + 1, 3), (np.float32(0.0), np.float32(0.0))) if good["n"][i + 1] < 4 else ("n", i, 3), ("n", i, 3)):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][at] = val
        with pytest.raises(AssertionError):
            MR.check(bad, refs[(3, 4)], tpl, 65, 4, 4, MR.tol_of, m, MR.ALPHA, MR.BETA)


# ---------------------------------------------------------------- arguments
def test_host_entry_rejects_bad_arguments_and_off_writes_nothing():
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f = lib.rt_debug_ctc_beam_lm_host
    m = MR.Model(5, {(1,): (-1.0, -0.5), (2,): (-1.0, -0.5), (1, 2): (-0.5, 0.0)}, -9.0)
    ids, lens, logp, bo = m.id_form()
    untouched = lambda out: ((out["n"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all() and (out["lm"]["lm"] == MR.CANARY_LM).all() and
                             (out["beams"]["n_tokens"] == BR.CANARY_N).all())
    for kw, msg in ((dict(alpha=-0.5), b"alpha is not a finite number at least 0"), (dict(alpha=float("nan")), b"alpha is not"),
                    (dict(alpha=float("inf")), b"alpha is not"), (dict(beta=float("nan")), b"beta is not finite"),
                    (dict(beta=float("-inf")), b"beta is not finite"), (dict(oov=1.0), b"oov is not a finite number at most 0"),
                    (dict(id_form=(np.array([1, 0, 1, 2]), lens, logp, bo)), b"n-gram 1: the blank (class 0) is not a token"),
                    (dict(id_form=(np.array([1, 2, 4, 2]), lens, logp, bo)), b"n-gram 2: the n-gram's context"),
                    (dict(B=33), b"beam = 33 is outside [0, RT_MAX_BEAM]"), (dict(n=5), b"nbest = 5 is outside"),
                    (dict(tpl=[-4]), b"line 0 has a negative number of time steps")):
        a = dict(tpl=[4], B=4, n=2, alpha=0.5, beta=0.5, id_form=None, oov=None)
        a.update(kw)
        rc, out = MR.call(f, None, z, W, b, a["tpl"], a["B"], a["n"], m, a["alpha"], a["beta"], id_form=a["id_form"], oov=a["oov"])
        assert rc == 8 and msg in lib.rt_last_error(None) and lib.rt_last_error(None).startswith(b"rt_debug_ctc_beam_lm_host: "), lib.rt_last_error(None)
        assert untouched(out)
    rc, out = MR.call(f, None, z, W, b, [4], 0, 3, m, 0.5, 0.5)      # beam = 0: off
    assert rc == 0 and untouched(out)
    rc, out = MR.call(f, None, z, W, b, [], 4, 2, m, 0.5, 0.5)       # no line
    assert rc == 0 and untouched(out)
    rc, out = MR.call(f, None, z, W, b, [0, 4, 0], 4, 2, m, 0.5, 0.5)   # lines without a time step report no hypothesis
    assert rc == 0 and out["n"].tolist() == [0, 2, 0]
    MR.hyps_of(out, [0, 4, 0], 2)
    empty = MR.Model(5, {}, -3.0)                                       # a model without an n-gram: every class is OOV
    rc, out = MR.call(f, None, z, W, b, [4], 4, 2, empty, 1.0, 0.0)
    assert rc == 0
    for s, _v, lm, _sc in MR.hyps_of(out, [4], 2)[0]:
        assert abs(float(lm) + 3.0 * len(s)) < 1e-6
