"""Rec beams (retto_amd/csrc/ctc_beam.h) on the MI355X: the device path (the row gather in chunks of whole lines, the CTC FC GEMM,
k_ctc_row_lse, k_ctc_beam_topc, k_ctc_beam_search) through rt_debug_ctc_beam against the fp64 restatement in ctc_beam_ref.py.
ctc_beam_ref.check is margin-free on every line and every hypothesis (count, distinct strings without a blank, order, canaries,
logprob <= the string's full CTC likelihood + tol) and compares with the fp64 rule rank by rank: the logprob at every rank, the
string wherever the fp64 rule's own neighbours are more than 2 tol away.  test_beam_cpu.py runs the same checks on the host rule
and asserts that on these seeds at most 10 % of the ranks, and rank 0 on at most 5 % of the lines, are left out of the string
comparison.

The tolerances are four times what the plain fp32 host loops deviate from fp64 on the same grid (ctc_beam_ref.MEASURED_HOST_*:
4.951e-4 up to 40 steps, 7.667e-4 on the line of 301 steps, both at N = 6625, where the host adds the 6625 terms of a row's lse
one after the other): TOL = 1.980e-3, TOL_LONG = 3.067e-3.

Measured on an MI355X over the grid of test_device_rule_against_fp64 (N in 5, 65, 6625; three lines each of 1, 2, 7 and 40 steps
and one of 301, every third pure noise; beams (1, 1), (4, 4), (16, 8), (32, 8); both chunkings give the same figures), worst
|logprob - fp64 rule| over every rank: on the lines of up to 40 steps 9.332e-6 at N = 5, 7.957e-6 at N = 65, 9.906e-6 at N = 6625;
on the line of 301 steps 3.431e-5, 1.089e-5, 2.663e-5.  The device is well inside a quarter of either tolerance: k_ctc_row_lse
adds a row's terms in 64 lanes and a butterfly, not one after the other.  Of the 801 ranks of a chunking 36 are left out of the
string comparison (the fp64 rule's own neighbours within 2 tol), rank 0 on none of the 156 lines."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lexicon_ref as LR

pytestmark = pytest.mark.gpu


def run_dev(sess, case, B, nbest, chunk=0):
    lib = _lib.load()
    rc, out = BR.call(lib.rt_debug_ctc_beam, sess._hd.h, *case, B, nbest, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case, B, nbest):
    rc, out = BR.call(_lib.load().rt_debug_ctc_beam_host, None, *case, B, nbest)
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs per N; the fp64 rule per (N, beam) is computed on first use and shared by the chunkings"""
    return {N: (BR.grid_case(N), {}) for N in LR.GRID_N}


def ref_of(grid, N, B):
    case, refs = grid[N]
    if B not in refs:
        refs[B] = BR.reference(*case, B)
    return refs[B]


@pytest.mark.parametrize("chunk", [0, 1], ids=["default_chunks", "one_line_chunks"])
@pytest.mark.parametrize("B,nbest", BR.GRID_BEAMS)
@pytest.mark.parametrize("N", LR.GRID_N)
def test_device_rule_against_fp64(hip_session, grid, N, B, nbest, chunk):
    """chunk_rows = 1: every chunk takes its first line and no other"""
    case = grid[N][0]
    tpl = case[3]
    assert max(tpl) == BR.GRID_LONG and set(BR.GRID_T) <= set(tpl)
    out = run_dev(hip_session, case, B, nbest, chunk=chunk)
    st = BR.check(out, ref_of(grid, N, B), tpl, N, B, nbest, BR.tol_of, what=(N, B, nbest, chunk))
    print("N=%d beam=%d/%d chunk=%d: worst deviation %.3e up to 40 steps, %.3e on the long line; %d of %d ranks left out"
          % ((N, B, nbest, chunk) + BR.worst_short_long(st) + (st["skipped"], st["ranks"])))
    assert st["lines"] == len(tpl) and out["n"].max() == nbest


@pytest.mark.parametrize("B", [2, 4])
def test_exact_ties_take_the_lower_id(hip_session, B):
    """W has duplicated columns and a duplicated bias: the two extensions carry bit-equal totals on any device, and the lower
    candidate index wins.  The device's strings are the host rule's and the fp64 rule's with the same tie order, exactly."""
    case = BR.tie_case()
    tpl = case[3]
    ref = BR.reference(*case, B)
    host = BR.hyps_of(run_host(case, B, B), tpl, B)
    for chunk in (0, 1):
        dev = BR.hyps_of(run_dev(hip_session, case, B, B, chunk=chunk), tpl, B)
        assert [[s for s, _ in h] for h in dev] == [[s for s, _ in h] for h in host], (chunk, dev, host)
        assert [[s for s, _ in h] for h in dev] == [[s for s, _ in r[1][:B]] for r in ref], chunk
        assert sum(h[k][1].tobytes() == h[k + 1][1].tobytes() for h in dev for k in range(len(h) - 1)) >= 2   # (ties are there)


@pytest.mark.parametrize("N", [65, 6625])
def test_planted_line(hip_session, N):
    """a string planted with gain 4.0 into noise is rank 0; its logprob lies between the log-probability of the planted path and the
    string's full CTC likelihood"""
    z, W, b, tpl, entries, paths = BR.planted_case(N)
    assert [len(e) for e in entries] == list(BR.PLANTED_LENS) and set(tpl) == {BR.PLANTED_T}
    lp = LR.logp64(LR.logits64(z, W, b))
    tol = BR.tol_of(BR.PLANTED_T)
    for B, n in ((16, 4), (4, 4)):
        H = BR.hyps_of(run_dev(hip_session, (z, W, b, tpl), B, n), tpl, n)
        for i, (e, path) in enumerate(zip(entries, paths)):
            l = lp[i * BR.PLANTED_T:(i + 1) * BR.PLANTED_T]
            assert H[i][0][0] == tuple(e), (N, B, i, H[i][0], e)
            path_lp = float(l[np.arange(BR.PLANTED_T), path].sum())
            assert path_lp - tol <= float(H[i][0][1]) <= BR.loglik64(l, tuple(e)) + tol, (N, B, i, path_lp, H[i][0][1])


def test_a_line_alone_and_nothing_at_all(hip_session, grid):
    """a line's values do not depend on what else is in the call beyond the logits GEMM's rounding; beam = 0 and a call without a
    line write nothing at all"""
    case = grid[65][0]
    z, W, b, tpl = case
    B, n = 16, 8
    out = BR.hyps_of(run_dev(hip_session, case, B, n), tpl, n)
    offs = np.concatenate([[0], np.cumsum(tpl)])
    for i in (tpl.index(40), tpl.index(7), len(tpl) - 1):
        alone = BR.hyps_of(run_dev(hip_session, (z[offs[i]:offs[i + 1]], W, b, [tpl[i]]), B, n), [tpl[i]], n)[0]
        assert [s for s, _ in alone] == [s for s, _ in out[i]], i
        assert max(abs(float(a[1]) - float(c[1])) for a, c in zip(alone, out[i])) <= 2 * BR.tol_of(tpl[i])
    for tp, beam in ((tpl, 0), ([], 4)):
        off = run_dev(hip_session, (z, W, b, tp), beam, 1)
        assert (off["n"] == BR.CANARY_N).all() and (off["beams"]["n_tokens"] == BR.CANARY_N).all() and (off["tokens"] == BR.CANARY_TOK).all()
    none = run_dev(hip_session, (z, W, b, [0, 7, 0]), 4, 2)
    assert none["n"].tolist() == [0, 2, 0]
    BR.hyps_of(none, [0, 7, 0], 2)


def test_bad_arguments_are_rejected(hip_session):
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f, h = lib.rt_debug_ctc_beam, hip_session._hd.h
    for B, n, chunk, msg in ((33, 1, 0, b"beam = 33 is outside [0, RT_MAX_BEAM]"), (4, 0, 0, b"nbest = 0 is outside [1, min(beam, RT_MAX_NBEST)]"),
                             (4, 5, 0, b"nbest = 5 is outside"), (32, 9, 0, b"nbest = 9 is outside"), (4, 1, -1, b"chunk_rows is negative")):
        rc, out = BR.call(f, h, z, W, b, [4], B, n, chunk=chunk)
        assert rc == 8 and msg in lib.rt_last_error(h), lib.rt_last_error(h)
        assert (out["n"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all()
