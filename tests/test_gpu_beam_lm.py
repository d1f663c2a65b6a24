"""Language-model fusion in the rec beam (retto_amd/csrc/ctc_lm.h) on the MI355X: the device path (the row gather in chunks of
whole lines, the CTC FC GEMM, k_ctc_row_lse, k_ctc_beam_topc, k_ctc_beam_search's fused variant) through rt_debug_ctc_beam_lm
against the fused fp64 restatement in ctc_lm_ref.py.  ctc_lm_ref.check is ctc_beam_ref.check with the comparisons made on the fused
score, and holds every hypothesis' lm to the model's direct definition.  test_beam_lm_cpu.py runs the same checks on the host
rule, measures the tolerance there -- four times what the plain fp32 host loops deviate from fp64 on this grid
(ctc_lm_ref.MEASURED_HOST_*: 4.951e-4 up to 40 steps, 8.321e-4 on the line of 301 steps): TOL = 1.980e-3, TOL_LONG = 3.328e-3;
the device is held to the same figures, not measured on itself -- and asserts that at most 10 % of the ranks, and rank 0 on at
most 5 % of the lines, are left out of the string comparison.

Seen on an MI355X over the grid of test_device_rule_against_fp64 (both chunkings give the same figures), worst |score - fused fp64
rule| over every rank: up to 40 steps 1.5e-5 at N = 5, 2.5e-5 at N = 65 and 6.5e-5 at N = 6625, on the line of 301 steps 3.5e-5,
1.9e-5 and 8.0e-5; at most 4 of a case's 104 ranks are left out of the string comparison."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lexicon_ref as LR
import ctc_lm_ref as MR
from test_beam_lm_cpu import check_exhaustive, check_rescue, check_ties, exhaustive_inputs

pytestmark = pytest.mark.gpu
A, Bt = MR.ALPHA, MR.BETA


def run_dev(sess, case, B, nbest, model, alpha=A, beta=Bt, chunk=0):
    lib = _lib.load()
    rc, out = MR.call(lib.rt_debug_ctc_beam_lm, sess._hd.h, *case, B, nbest, model, alpha, beta, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_plain_dev(sess, case, B, nbest, chunk=0):
    lib = _lib.load()
    rc, out = BR.call(lib.rt_debug_ctc_beam, sess._hd.h, *case, B, nbest, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case, B, nbest, model, alpha=A, beta=Bt):
    rc, out = MR.call(_lib.load().rt_debug_ctc_beam_lm_host, None, *case, B, nbest, model, alpha, beta)
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs and models per N; the fused fp64 rule per (N, order, beam) is computed on first use and shared by the chunkings"""
    g = {}
    for N in LR.GRID_N:
        case = BR.grid_case(N)
        g[N] = (case, {order: MR.grid_model(N, order, case) for order in MR.ORDERS}, {})
    return g


def ref_of(grid, N, order, B):
    case, models, refs = grid[N]
    if (order, B) not in refs:
        refs[(order, B)] = MR.reference(*case, B, models[order], A, Bt)
    return refs[(order, B)]


@pytest.mark.parametrize("chunk", [0, 1], ids=["default_chunks", "one_line_chunks"])
@pytest.mark.parametrize("B,nbest", BR.GRID_BEAMS)
@pytest.mark.parametrize("order", MR.ORDERS)
@pytest.mark.parametrize("N", LR.GRID_N)
def test_device_rule_against_fp64(hip_session, grid, N, order, B, nbest, chunk):
    """chunk_rows = 1: every chunk takes its first line and no other"""
    case, models, _ = grid[N]
    tpl = case[3]
    out = run_dev(hip_session, case, B, nbest, models[order], chunk=chunk)
    st = MR.check(out, ref_of(grid, N, order, B), tpl, N, B, nbest, MR.tol_of, models[order], A, Bt, what=(N, order, B, nbest, chunk))
    print("N=%d order=%d beam=%d/%d chunk=%d: worst deviation %.3e up to 40 steps, %.3e on the long line; %d of %d ranks left out"
          % ((N, order, B, nbest, chunk) + BR.worst_short_long(st) + (st["skipped"], st["ranks"])))
    assert st["lines"] == len(tpl) and out["n"].max() == nbest


@pytest.mark.parametrize("N", [5, 65])
def test_zero_weights_are_the_plain_device_beam_bit_for_bit(hip_session, grid, N):
    """alpha = beta = 0 with any model: counts, tokens and logprob are rt_debug_ctc_beam's bytes"""
    case, models, _ = grid[N]
    for order in MR.ORDERS:
        for B, n in BR.GRID_BEAMS:
            for chunk in (0, 1):
                a = run_dev(hip_session, case, B, n, models[order], 0.0, 0.0, chunk=chunk)
                p = run_plain_dev(hip_session, case, B, n, chunk=chunk)
                for k in ("n", "beams", "tokens"):
                    assert a[k].tobytes() == p[k].tobytes(), (N, order, B, n, chunk, k)


def test_exhaustive_case(hip_session):
    case, m = exhaustive_inputs()
    for chunk in (0, 1):
        check_exhaustive(run_dev(hip_session, case, 32, 8, m, chunk=chunk), case, m)


@pytest.mark.parametrize("B", [2, 4])
def test_exact_ties_take_the_lower_id(hip_session, B):
    """classes bit-identical in the head and in the model: the device's strings are the host rule's and the fused fp64 rule's
    with the same tie order, exactly"""
    case, m = BR.tie_case(), MR.tie_model()
    tpl = case[3]
    ref = MR.reference(*case, B, m, A, Bt)
    host = MR.hyps_of(run_host(case, B, B, m), tpl, B)
    for chunk in (0, 1):
        out = run_dev(hip_session, case, B, B, m, chunk=chunk)
        check_ties(out, ref, tpl, B)
        dev = MR.hyps_of(out, tpl, B)
        assert [[h[0] for h in hs] for hs in dev] == [[h[0] for h in hs] for hs in host]
        assert sum(h[k][3].tobytes() == h[k + 1][3].tobytes() for h in dev for k in range(len(h) - 1)) >= 2   # (ties are there)


def test_rescue_case(hip_session):
    case, m = MR.rescue_case()
    fused = run_dev(hip_session, case, 8, 4, m)
    check_rescue(run_plain_dev(hip_session, case, 8, 4), fused, case, m)
    MR.check(fused, MR.reference(*case, 8, m, A, Bt), case[3], MR.RESCUE_N, 8, 4, MR.tol_of, m, A, Bt)


@pytest.mark.parametrize("T", [1, 2, 7])
def test_order_5_on_lines_shorter_than_the_order(hip_session, T):
    """hypotheses shorter than the order: the start state and every back-off depth are reached while the context is still growing"""
    N = 9
    rng = np.random.default_rng(600 + T)
    W, b = BR.weights(rng, N)
    paths = [(T, LR.alignment(LR.random_entry(rng, N, max(1, T // 2), T), T)) for _ in range(4)] + [(T, None)] * 2
    z = LR.planted_features(rng, W.astype(np.float64), paths, gain=3.0, noise=1.5)
    case = (z, W, b, [T] * len(paths))
    texts = [R[0][0] for _lp, R in BR.reference(*case, 4)]
    m = MR.random_model(640 + T, N, 5, texts, per_level=40)
    assert m.order == 5 and (N,) in m.state_index
    for B, n in ((4, 4), (32, 8)):
        ref = MR.reference(*case, B, m, A, Bt)
        for chunk in (0, 1):
            MR.check(run_dev(hip_session, case, B, n, m, chunk=chunk), ref, case[3], N, B, n, MR.tol_of, m, A, Bt, what=(T, B, chunk))
    first = {s[0] for _lp, R in MR.reference(*case, 32, m, A, Bt) for s, *_ in R if s}
    assert any((N, c) in m.ngrams for c in first) and any((N, c) not in m.ngrams for c in first)   # (<s> c hit and backed off)


def test_a_line_alone_and_nothing_at_all(hip_session, grid):
    case, models, _ = grid[65]
    z, W, b, tpl = case
    m = models[3]
    B, n = 16, 8
    out = MR.hyps_of(run_dev(hip_session, case, B, n, m), tpl, n)
    offs = np.concatenate([[0], np.cumsum(tpl)])
    for i in (tpl.index(40), tpl.index(7), len(tpl) - 1):
        alone = MR.hyps_of(run_dev(hip_session, (z[offs[i]:offs[i + 1]], W, b, [tpl[i]]), B, n, m), [tpl[i]], n)[0]
        assert [h[0] for h in alone] == [h[0] for h in out[i]], i
        assert max(abs(float(a[3]) - float(c[3])) for a, c in zip(alone, out[i])) <= 2 * MR.tol_of(tpl[i])
        assert [a[2].tobytes() for a in alone] == [c[2].tobytes() for c in out[i]]      # (lm depends on the string alone)
    for tp, beam in ((tpl, 0), ([], 4)):
        off = run_dev(hip_session, (z, W, b, tp), beam, 1, m)
        assert (off["n"] == BR.CANARY_N).all() and (off["beams"]["n_tokens"] == BR.CANARY_N).all() and (off["tokens"] == BR.CANARY_TOK).all()
        assert (off["lm"]["lm"] == MR.CANARY_LM).all()
    none = run_dev(hip_session, (z, W, b, [0, 7, 0]), 4, 2, m)
    assert none["n"].tolist() == [0, 2, 0]
    MR.hyps_of(none, [0, 7, 0], 2)


def test_bad_arguments_are_rejected_before_any_launch(hip_session):
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f, h = lib.rt_debug_ctc_beam_lm, hip_session._hd.h
    m = MR.Model(5, {(1,): (-1.0, -0.5), (2,): (-1.0, -0.5), (1, 2): (-0.5, 0.0)}, -9.0)
    _ids, lens, logp, bo = m.id_form()
    for kw, msg in ((dict(alpha=-0.5), b"alpha is not a finite number at least 0"), (dict(beta=float("nan")), b"beta is not finite"),
                    (dict(oov=1.0), b"oov is not a finite number at most 0"),
                    (dict(id_form=(np.array([1, 0, 1, 2]), lens, logp, bo)), b"n-gram 1: the blank (class 0) is not a token"),
                    (dict(id_form=(np.array([1, 2, 1, 9]), lens, logp, bo)), b"n-gram 2: token id 9 is outside [1, 5]"),
                    (dict(B=33), b"beam = 33 is outside [0, RT_MAX_BEAM]"), (dict(n=5), b"nbest = 5 is outside"),
                    (dict(chunk=-1), b"chunk_rows is negative")):
        a = dict(B=4, n=2, alpha=0.5, beta=0.5, id_form=None, oov=None, chunk=0)
        a.update(kw)
        rc, out = MR.call(f, h, z, W, b, [4], a["B"], a["n"], m, a["alpha"], a["beta"], chunk=a["chunk"], id_form=a["id_form"], oov=a["oov"])
        assert rc == 8 and msg in lib.rt_last_error(h) and lib.rt_last_error(h).startswith(b"rt_debug_ctc_beam_lm: "), lib.rt_last_error(h)
        assert (out["n"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all() and (out["lm"]["lm"] == MR.CANARY_LM).all()
