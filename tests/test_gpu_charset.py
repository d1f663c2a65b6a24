"""Rec charsets (retto_amd/csrc/ctc_charset.h) on the MI355X: the device path (the row gather, the CTC FC GEMM,
k_ctc_charset_argmax, then pp::ctc_decode and the masked k_ctc_topk) through rt_debug_ctc_charset against the fp64 restatement in
ctc_charset_ref.py.  The checks are margin-free and leave no row out (ctc_charset_ref.check_outputs).

Measured on an MI355X over the grid of test_device_rule_against_fp64 (N in 5 .. 6625, K in 0, 1, 5; 241 restricted rows each, fp64
reference on the same features): worst |p - q| = 4.30e-6 (N = 6625, K = 5, a rank >= 1 entry; 3.72e-6 over the rows' own prob
at N = 6625, 2.43e-6 at N = 65, 7.2e-7 at N = 5).  On these inputs the fp64 gap between the two best allowed logits is at
least 6e-4 on every row (test_charset_cpu.test_grid_inputs_have_a_clear_winner_on_every_row), so idx is in practice the fp64
argmax itself, which test_device_rule_against_fp64 asserts as well."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_candidates_ref as R
import ctc_charset_ref as CR

pytestmark = pytest.mark.gpu

# 4 x the worst |p - q| measured on the MI355X over the N x K grid below (test_gpu_candidates.py's convention; that file's
# PIPE_TOL = 2e-4 is the cap)
MEASURED_WORST = 4.30e-6
HOOK_TOL = 4 * MEASURED_WORST
assert HOOK_TOL <= 2e-4


def run_dev(sess, case, K, chunk=0):
    lib = _lib.load()
    rc, out = CR.call(lib.rt_debug_ctc_charset, sess._hd.h, *case, K, chunk=chunk)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case, K):
    rc, out = CR.call(_lib.load().rt_debug_ctc_charset_host, None, *case, K)
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs, generated once"""
    return {N: CR.grid_case(N) for N in (5, 37, 64, 65, 6625)}


@pytest.mark.parametrize("K", [0, 1, 5])
@pytest.mark.parametrize("N", [5, 37, 64, 65, 6625])
def test_device_rule_against_fp64(hip_session, grid, N, K):
    case = grid[N]
    out = run_dev(hip_session, case, K)
    worst = CR.check_outputs(out, *case, K, HOOK_TOL, (N, K))
    print("worst |p - q| N=%d K=%d: %.3e" % (N, K, worst))
    assert out["ntok"].sum() > 0
    # the fp64 argmax itself (the inputs have a clear winner on every row)
    z, W, b, _, _, tpl, ls, masks = case
    l = CR.logits64(z, W, b)
    o = 0
    for T, s in zip(tpl, ls):
        if s > 0:
            S = np.array(CR.members(masks[s - 1], N))
            assert np.array_equal(out["idx"][o:o + T], S[np.argmax(l[o:o + T][:, S], axis=1)]), (N, K, s)
        o += T


def _zero_case(N, bias, ids, idx0=1):
    T = 8
    z, W, b = CR.zero_feature_case(N, bias, T)
    return z, W, b, np.full(T, idx0, np.int32), np.full(T, 0.5, np.float32), [T], [1], np.stack([CR.mask_of(ids, N)])


def test_tied_allowed_classes_come_out_by_id(hip_session):
    """all-zero features: the logits are the biases, bit for bit"""
    N = 37
    bias = np.full(N, -2.0, np.float32); bias[[3, 9, 20, 36]] = 1.5
    case = _zero_case(N, bias, [9, 20, 36, 5])    # 3 is outside: 9, 20 and 36 tie
    out = run_dev(hip_session, case, 8)
    assert list(out["idx"]) == [9] * 8 and out["ntok"][0] == 1 and out["tokens"][0] == 9
    assert list(out["cands"]["id"][0]) == [9, 20, 36, 0, 5, -1, -1, -1]
    p = out["cands"]["prob"][0]
    assert p[0].tobytes() == p[1].tobytes() == p[2].tobytes() and p[3].tobytes() == p[4].tobytes()
    assert list(p[5:]) == [0.0, 0.0, 0.0]          # |S| = 5 < K = 8: the (-1, 0.0f) fill
    CR.check_outputs(out, *case, 8, HOOK_TOL)


def test_the_largest_bias_outside_the_set_is_never_chosen(hip_session):
    N = 65
    bias = np.linspace(-1.0, 1.0, N).astype(np.float32); bias[64] = 9.0; bias[33] = 8.0
    case = _zero_case(N, bias, [2, 31, 32, 63])
    out = run_dev(hip_session, case, 5)
    assert list(out["idx"]) == [63] * 8
    assert 64 not in out["cands"]["id"][0] and 33 not in out["cands"]["id"][0]
    assert list(out["cands"]["id"][0]) == [63, 32, 31, 2, 0]
    CR.check_outputs(out, *case, 5, HOOK_TOL)


@pytest.mark.parametrize("N", [37, 65, 6625])
def test_pad_columns_take_no_part(hip_session, N):
    """negative biases: a pad column of the logits GEMM (weights and bias zero: logit 0) would win the maximum and join the sum"""
    rng = np.random.default_rng(N)
    bias = (-1.0 - 3.0 * rng.random(N)).astype(np.float32)
    case = _zero_case(N, bias, [N - 1, N - 2, N - 3, 1])
    out = run_dev(hip_session, case, 5)
    assert out["idx"].max() < N and out["cands"]["id"][:1].max() < N
    CR.check_outputs(out, *case, 5, HOOK_TOL)
    host = run_host(case, 5)
    assert np.array_equal(out["idx"], host["idx"])


def test_blank_only_set_gives_no_token_and_probability_one(hip_session):
    N = 6625
    bias = np.random.default_rng(1).normal(0, 1, N).astype(np.float32)
    case = _zero_case(N, bias, [])
    out = run_dev(hip_session, case, 3)
    assert list(out["idx"]) == [0] * 8 and out["ntok"][0] == 0 and np.isnan(out["scores"][0])
    assert out["prob"].tobytes() == np.ones(8, np.float32).tobytes()
    CR.check_outputs(out, *case, 3, HOOK_TOL)


@pytest.mark.parametrize("restricted", [0, 1, 16, 17, 33])
def test_logits_chunks(hip_session, restricted):
    """chunk_rows = 16: no restricted row, one, exactly one chunk, one chunk and a row, two chunks and a row"""
    rng = np.random.default_rng(restricted)
    first = min(restricted, 5)
    tpl = [9, max(first, 1), 12, max(restricted - first, 1)]
    ls = [0, 1 if first else 0, 0, 2 if restricted - first else 0]
    z, W, b, idx, prob = R.make_case(rng, 6625, tpl)
    case = (z, W, b, idx, prob, tpl, ls, CR.grid_sets(rng, 6625)[1:])
    assert sum(T for T, s in zip(tpl, ls) if s) == restricted
    out = run_dev(hip_session, case, 4, chunk=16)
    CR.check_outputs(out, *case, 4, HOOK_TOL, restricted)


def test_line_lengths_around_the_wave(hip_session):
    """lines of 1, 63, 64, 65 and 129 time steps, every one restricted"""
    rng = np.random.default_rng(64)
    tpl = [1, 63, 64, 65, 129]
    z, W, b, idx, prob = R.make_case(rng, 65, tpl, blank_share=0.05, repeat_share=0.05)
    case = (z, W, b, idx, prob, tpl, [3, 2, 1, 3, 2], CR.grid_sets(rng, 65))
    out = run_dev(hip_session, case, 3)
    assert out["ntok"][4] > 20
    CR.check_outputs(out, *case, 3, HOOK_TOL)


def test_large_logits_stay_finite(hip_session):
    """logits out to about +-80: the maximum over the set is subtracted before exp"""
    rng = np.random.default_rng(80)
    N, K, tpl = 6625, 5, [60]
    z = np.clip(rng.normal(0.0, 6.0, (60, R.D)), -20.0, 20.0).astype(np.float32)
    W = (rng.normal(0.0, 1.0, (R.D, N)) * 0.27).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    l = CR.logits64(z, W, b)
    assert l.max() > 60 and l.min() < -60
    masks = CR.grid_sets(rng, N)[2:]
    case = (z, W, b, np.zeros(60, np.int32), np.full(60, 0.5, np.float32), tpl, [1], masks)
    out = run_dev(hip_session, case, K)
    S = set(CR.members(masks[0], N))
    assert np.isfinite(out["prob"]).all() and (out["prob"] > 0).all() and (out["prob"] <= 1.0).all()
    assert set(out["idx"].tolist()) <= S and out["ntok"][0] > 30
    c = out["cands"][:out["ntok"][0]]
    assert np.isfinite(c["prob"]).all() and (c["prob"] >= 0).all() and set(c["id"].ravel().tolist()) <= S
    assert (c["prob"].astype(np.float64).sum(axis=1) <= 1.0 + K * HOOK_TOL).all()


def test_unrestricted_lines_equal_the_candidates_hook(hip_session, grid):
    """line_set all 0: idx / prob untouched, and the candidates are what rt_debug_ctc_candidates returns, bit for bit"""
    import ctypes as C
    z, W, b, idx, prob, tpl, _, masks = grid[65]
    case = (z, W, b, idx, prob, tpl, [0] * len(tpl), masks)
    out = run_dev(hip_session, case, 5)
    assert out["idx"].tobytes() == np.asarray(idx, np.int32).tobytes() and out["prob"].tobytes() == np.asarray(prob, np.float32).tobytes()
    lib = _lib.load()
    cands, cols = R.new_outputs(sum(tpl), 5)
    ntok = np.full(len(tpl), -1, np.int32)
    keep, a = R.call_args(z, W, b, idx, prob, tpl)
    assert lib.rt_debug_ctc_candidates(hip_session._hd.h, a[0], a[1], a[2], 65, a[3], a[4], a[5], len(tpl), 5, 0,
                                       cands.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p),
                                       ntok.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(ntok, out["ntok"]) and cols.tobytes() == out["cols"].tobytes() and cands.tobytes() == out["cands"].tobytes()
