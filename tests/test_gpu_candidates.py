"""Token candidates (rt_config.rec_return_candidates) on the MI355X: the device path (k_ctc_kept_rows, the row gather, the CTC
FC GEMM, k_ctc_topk) through rt_debug_ctc_candidates against the fp64 restatement in ctc_candidates_ref.py, and inside the
pipeline teacher-forced by the oracle session running the HIP workers.

Measured on an MI355X over the grid of test_device_rule_against_fp64 (N in 5 .. 6625, K in 1 .. 8, 113 .. 165 kept rows each, fp64
reference on the same features): worst |p - q| = 3.91e-6 (N = 65, K = 5; 3.38e-6 at N = 6625); the same rule in plain fp32 loops
on the CPU: 5.09e-6."""
import ctypes as C

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, synth, workload
from oracle import ref_lib as OR
import ctc_candidates_ref as R

pytestmark = pytest.mark.gpu

# Hook tests: 4 x the worst |p - q| measured on the MI355X over the N x K grid below (see the module docstring; the worst case grows
# slowly with the row count, and the tests use few rows); far below the 2e-4 test_rec_net holds the same softmax to.
HOOK_TOL = 4 * 3.92e-6
# Pipeline tests compare with the probability rows the same session's rt_rec returns: the project's bar for that softmax.
PIPE_TOL = 2e-4


def run_dev(sess, z, W, b, idx, prob, tpl, K, chunk=0):
    lib = _lib.load()
    rows = int(sum(tpl))
    cands, cols = R.new_outputs(rows, K)
    ntok = np.full(len(tpl), -1, np.int32)
    keep, a = R.call_args(z, W, b, idx, prob, tpl)
    rc = lib.rt_debug_ctc_candidates(sess._hd.h, a[0], a[1], a[2], W.shape[1], a[3], a[4], a[5], len(tpl), K, chunk,
                                     cands.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p),
                                     ntok.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return cands, cols, ntok


def run_host(z, W, b, idx, prob, tpl, K):
    lib = _lib.load()
    cands, cols = R.new_outputs(int(sum(tpl)), K)
    ntok = np.full(len(tpl), -1, np.int32)
    keep, a = R.call_args(z, W, b, idx, prob, tpl)
    assert lib.rt_debug_ctc_candidates_host(a[0], a[1], a[2], W.shape[1], a[3], a[4], a[5], len(tpl), K,
                                            cands.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p),
                                            ntok.ctypes.data_as(C.c_void_p)) == 0
    return cands, cols, ntok


# ---------------------------------------------------------------- the device path on host arrays
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("N", [5, 37, 64, 65, 6625])
def test_device_rule_against_fp64(hip_session, N, K):
    rng = np.random.default_rng(1000 * N + K)
    tpl = [40, 1, 80, 7, 33, 120]
    z, W, b, idx, prob = R.make_case(rng, N, tpl)
    cands, cols, ntok = run_dev(hip_session, z, W, b, idx, prob, tpl, K)
    assert 0 < ntok.sum() < sum(tpl)
    worst = R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, tpl, K, HOOK_TOL, (N, K))
    print("worst |p - q| N=%d K=%d kept=%d: %.3e" % (N, K, ntok.sum(), worst))
    # the device against the same rule in plain fp32 loops on the CPU: same columns and rank 0; a class both return agrees within
    # the tolerance, a class only the device returns sat at the CPU list's edge
    hc, hcols, hntok = run_host(z, W, b, idx, prob, tpl, K)
    assert np.array_equal(ntok, hntok) and np.array_equal(cols, hcols)
    assert np.ascontiguousarray(cands[:, 0]).tobytes() == np.ascontiguousarray(hc[:, 0]).tobytes()
    o = 0
    for li, T in enumerate(tpl):
        for j in range(ntok[li]):
            d, h = cands[o + j][1:], hc[o + j][1:]
            host = {int(i): float(p) for i, p in zip(h["id"], h["prob"])}
            for i, p in zip(d["id"], d["prob"]):
                if int(i) in host:
                    assert abs(float(p) - host[int(i)]) <= HOOK_TOL, (N, K, li, j)
                else:
                    assert float(p) <= min(host.values()) + 2 * HOOK_TOL, (N, K, li, j)
        o += T


def test_exact_ties_are_ordered_by_id(hip_session):
    """All-zero features: every logit is exactly its bias; tied classes come out in id order with bit-equal probabilities."""
    N, K, T = 37, 8, 6
    b = np.array([0.5, 2.0, 1.0] * 12 + [2.0], np.float32)
    z = np.zeros((T, R.D), np.float32)
    W = np.random.default_rng(3).normal(0, 1, (R.D, N)).astype(np.float32)
    idx = np.array([4, 0, 1, 1, 36, 2], np.int32)
    prob = np.full(T, 0.25, np.float32)
    cands, cols, ntok = run_dev(hip_session, z, W, b, idx, prob, [T], K)
    assert ntok[0] == 4 and list(cols[:4]) == [0, 2, 4, 5]
    top = [i for i in range(N) if b[i] == 2.0]
    for j, tok in enumerate([4, 1, 36, 2]):
        assert list(cands["id"][j][1:]) == [i for i in top if i != tok][:K - 1], (j, cands["id"][j])
        assert len(set(cands["prob"][j][1:].tobytes()[4 * k:4 * k + 4] for k in range(K - 1))) == 1
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, [T], K, HOOK_TOL)


@pytest.mark.parametrize("N", [37, 65, 6625])
def test_pad_columns_are_excluded(hip_session, N):
    """The logits GEMM writes the pad columns up to round_up(N, 4), where weights and bias are zero: with zero features and
    negative biases a pad logit of 0 would beat every class."""
    rng = np.random.default_rng(N)
    T, K = 9, 5
    z = np.zeros((T, R.D), np.float32)
    W = rng.normal(0, 1, (R.D, N)).astype(np.float32)
    b = (-1.0 - 3.0 * rng.random(N)).astype(np.float32)
    idx = np.array([N - 1, 1, 0, N - 2, N - 2, 3, 0, 2, N - 1], np.int32)
    prob = np.full(T, 0.5, np.float32)
    cands, cols, ntok = run_dev(hip_session, z, W, b, idx, prob, [T], K)
    assert ntok[0] == 6
    assert cands["id"][:6].max() < N
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, [T], K, HOOK_TOL)


def test_ballot_chunk_edges(hip_session):
    """Lines of 1, 63, 64, 65 and 129 time steps: the 64-step ballot chunks of k_ctc_kept_rows, nearly every step kept."""
    rng = np.random.default_rng(64)
    tpl = [1, 63, 64, 65, 129]
    z, W, b, idx, prob = R.make_case(rng, 65, tpl, blank_share=0.05, repeat_share=0.05)
    cands, cols, ntok = run_dev(hip_session, z, W, b, idx, prob, tpl, 3)
    assert ntok[2] > 40 and ntok[4] > 80
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, tpl, 3, HOOK_TOL)


@pytest.mark.parametrize("kept", [0, 1, 16, 17, 33])
def test_logits_chunks(hip_session, kept):
    """chunk_rows = 16: no chunk, one row, exactly one chunk, one chunk and a row, two chunks and a row."""
    rng = np.random.default_rng(kept)
    tpl = [30, 40]
    z, W, b, _, _ = R.make_case(rng, 6625, tpl)
    idx = np.zeros(70, np.int32)
    first = min(kept, 12)
    idx[0:2 * first:2] = 7 + np.arange(first)            # line 0: `first` kept steps, blanks between them
    idx[30:30 + kept - first] = 100 + np.arange(kept - first)   # line 1: the rest, consecutive and distinct
    q = R.softmax64(z, W, b)
    prob = q[np.arange(70), idx].astype(np.float32)
    cands, cols, ntok = run_dev(hip_session, z, W, b, idx, prob, tpl, 4, chunk=16)
    assert ntok.sum() == kept
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, tpl, 4, HOOK_TOL)


def test_large_logits_stay_finite(hip_session):
    """Logits out to about +-80: the maximum is subtracted before exp, so no inf or NaN, and what a row returns sums to <= 1."""
    rng = np.random.default_rng(80)
    N, K, tpl = 6625, 8, [60]
    z = np.clip(rng.normal(0.0, 6.0, (60, R.D)), -20.0, 20.0).astype(np.float32)
    W = (rng.normal(0.0, 1.0, (R.D, N)) * 0.27).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    l = z.astype(np.float64) @ W.astype(np.float64) + b
    assert l.max() > 60 and l.min() < -60
    q = R.softmax64(z, W, b)
    idx = q.argmax(axis=1).astype(np.int32)
    prob = q[np.arange(60), idx].astype(np.float32)
    cands, cols, ntok = run_dev(hip_session, z, W, b, idx, prob, tpl, K)
    assert ntok[0] > 30
    c = cands[:ntok[0]]
    assert np.isfinite(c["prob"]).all() and (c["prob"] >= 0).all()
    assert (c["prob"].astype(np.float64).sum(axis=1) <= 1.0 + K * HOOK_TOL).all()
    for row in c["id"]:
        assert len(set(row.tolist())) == K and row.min() >= 0 and row.max() < N


# ---------------------------------------------------------------- inside the pipeline
def _cfg(k: int, **kw):
    cfg = retto_amd.synthetic_session_config(0, **kw)
    cfg.rec_processor_config.return_candidates = k
    return cfg


@pytest.fixture(scope="module")
def k5_session():
    s = retto_amd.RettoSession(_cfg(5))
    yield s
    s.close()


def _planted_for(page_h, page_w, lines, seed):
    page, rects = workload.planted_page(page_h, page_w, lines, seed)
    plan = OR.resize_both_plan(page_h, page_w)
    ah, aw = plan[-1] if plan else (page_h, page_w)
    dh, dw = OR.resize_either_dims(ah, aw)
    return page, workload.planted_map(dh, dw, page_h, page_w, rects)


def _tall_page():
    """test_gpu_word_boxes' page: lines of h / w >= 1.5 (crops rotated by 270 degrees) beside a line over 1500 px wide"""
    h, w = 400, 1984
    page = np.zeros((h, w, 3), np.uint8)
    rng = np.random.default_rng(3)
    rects = [(20, 30, 1930, 55), (40, 120, 300, 126), (600, 100, 640, 380), (700, 90, 760, 330), (900, 200, 1500, 240)]
    for x0, y0, x1, y1 in rects:
        page[y0:y1, x0:x1] = rng.integers(100, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    plan = OR.resize_both_plan(h, w)
    ah, aw = plan[-1] if plan else (h, w)
    dh, dw = OR.resize_either_dims(ah, aw)
    return page, workload.planted_map(dh, dw, h, w, rects, shrink=0.05)


def _oracle(session):
    """the oracle session running the HIP workers; rec_worker records the same session's rt_rec probability rows"""
    from oracle.pipeline import OracleSession
    det, cls, rec, dic = synth.synth_models(0)
    o = OracleSession(det, cls, rec, dic)
    o.det_worker, o.cls_worker = session.worker.det, session.worker.cls
    o.calls = []

    def rec_worker(t):
        p = session.worker.rec(t)
        o.calls.append(p)
        return p
    o.rec_worker = rec_worker
    return o


def _teacher_forced(session, pages, maps, K):
    """every line of every page: columns, rank 0 and ranks >= 1 against the recorded probability rows; returns the token count"""
    res = session.run_batch(pages, det_map_override=maps)
    o = _oracle(session)
    total = 0
    for page, m, r in zip(pages, maps, res):
        o.calls = []
        ores = o.run(page, det_map_override=m)
        n = len(ores.crops)
        dims = [c.shape[:2] for c in ores.crops]
        order = sorted(range(n), key=lambda i: -(float(dims[i][0]) / float(dims[i][1])))
        probs = [None] * n
        for bi, p in enumerate(o.calls):
            for j, i in enumerate(order[6 * bi:6 * bi + 6]):
                probs[i] = p[j]
        assert len(r.rec_result) == n
        for i, g in enumerate(r.rec_result):
            q = probs[i].astype(np.float64)
            am = np.argmax(probs[i], axis=-1)
            kc = R.kept_cols(am)
            assert [int(c) for c in g.token_cols] == kc, f"line {i}: kept columns differ"
            assert len(g.candidates) == len(g.tokens) == len(kc)
            for j, (t, cand) in enumerate(zip(kc, g.candidates)):
                assert len(cand) == K
                assert cand[0][0] == int(g.tokens[j]) == int(am[t])
                assert cand[0][1] == o.dict[cand[0][0]]
                assert abs(cand[0][2] - q[t, am[t]]) <= PIPE_TOL
                R.check_token(int(am[t]), [c[0] for c in cand[1:]], [c[2] for c in cand[1:]], q[t], PIPE_TOL, (i, j))
            if len(kc):   # rank 0 is what the score averages
                assert abs(np.mean([c[0][2] for c in g.candidates]) - g.score) <= 1e-6
            total += len(kc)
    return res, total


def _sig(results):
    """everything the option returns, bit for bit"""
    return [([int(c) for c in g.token_cols], [[(i, np.float32(p).tobytes()) for i, _, p in tok] for tok in g.candidates])
            for r in results for g in r.rec_result]


def _same_but_candidates(a, b):
    for x, y in zip(a, b):
        assert [d.boxes.as_array().tolist() for d in x.det_result] == [d.boxes.as_array().tolist() for d in y.det_result]
        assert np.array_equal(np.array([d.score for d in x.det_result], np.float32), np.array([d.score for d in y.det_result], np.float32))
        assert [(c.label.label, c.label.score) for c in x.cls_result] == [(c.label.label, c.label.score) for c in y.cls_result]
        for g, h in zip(x.rec_result, y.rec_result):
            assert np.array_equal(g.tokens, h.tokens) and g.text == h.text
            assert np.array_equal(np.float32(g.score).view(np.uint32), np.float32(h.score).view(np.uint32))


def test_on_changes_nothing_else(k5_session, hip_session):
    pages, maps = zip(*[_planted_for(960, 960, 32, s) for s in (101, 102)])
    a = k5_session.run_batch(list(pages), det_map_override=list(maps))
    b = hip_session.run_batch(list(pages), det_map_override=list(maps))
    assert k5_session.last_det_checksum == hip_session.last_det_checksum
    _same_but_candidates(a, b)
    assert all(g.candidates is not None and h.candidates is None and h.token_cols is None
               for x, y in zip(a, b) for g, h in zip(x.rec_result, y.rec_result))
    lib = _lib.load()
    for sess, want in ((hip_session, 0), (k5_session, 5)):   # the C accessor: 0 on the off session
        r = sess.run_batch_raw([pages[0]], [960], [960], det_map_override=[maps[0]])
        try:
            cp = C.POINTER(_lib.Candidate)(); colp = C.POINTER(C.c_int32)()
            assert lib.rt_results_count(r, 0) > 0
            assert lib.rt_results_rec_candidates(r, 0, 0, C.byref(cp), C.byref(colp)) == want
            assert lib.rt_results_rec_candidates(r, 0, 10 ** 6, None, None) == 0
        finally:
            lib.rt_results_free(r)


def test_teacher_forced_pages(k5_session):
    pages, maps = zip(*[_planted_for(480, 640, 6, 31), _planted_for(960, 960, 32, 201)])
    _, total = _teacher_forced(k5_session, list(pages), list(maps), 5)
    assert total > 50


def test_tall_and_widest_lines_teacher_forced():
    s = retto_amd.RettoSession(_cfg(2))
    try:
        page, m = _tall_page()
        res, total = _teacher_forced(s, [page], [m], 2)
        assert total > 0
        assert max(int(max(g.token_cols)) for g in res[0].rec_result if len(g.token_cols)) >= 64   # a line past one ballot chunk
    finally:
        s.close()


CAND_FAMILIES = ("ctc_gather_rows", "gemm_cand_fc", "ctc_topk")


def test_k1_runs_no_logits_recompute(k5_session, hip_session):
    pages, maps = zip(*[_planted_for(960, 960, 32, s) for s in (101, 102)])
    s = retto_amd.RettoSession(_cfg(1))
    try:
        profs = []
        for sess in (s, k5_session, hip_session):
            sess.profile_enable(True)
            try:
                out = sess.run_batch(list(pages), det_map_override=list(maps))
                profs.append(sess.profile_get())
            finally:
                sess.profile_enable(False)
            if sess is s:
                res = out
        k1, k5, off = profs
        assert "ctc_kept_rows" in k1 and not any(f in k1 for f in CAND_FAMILIES), sorted(k1)
        assert "ctc_kept_rows" in k5 and all(f in k5 for f in CAND_FAMILIES), sorted(k5)
        assert "ctc_kept_rows" not in off and not any(f in off for f in CAND_FAMILIES), sorted(off)
        _same_but_candidates(res, hip_session.run_batch(list(pages), det_map_override=list(maps)))
        n = 0
        for r in res:
            for g in r.rec_result:
                assert len(g.candidates) == len(g.tokens) == len(g.token_cols)
                assert all(len(c) == 1 and c[0][0] == int(t) for c, t in zip(g.candidates, g.tokens))
                n += len(g.tokens)
        assert n > 0
        lib = _lib.load()
        r = s.run_batch_raw([pages[0]], [960], [960], det_map_override=[maps[0]])
        try:
            assert lib.rt_results_rec_candidates(r, 0, 0, None, None) == 1
        finally:
            lib.rt_results_free(r)
    finally:
        s.close()


def test_repeatable_and_submit_wait_equals_run_batch(k5_session):
    pages, maps = zip(*[_planted_for(960, 960, 32, s) for s in (301, 302, 303, 304)])
    pages, maps = list(pages), list(maps)
    a = k5_session.run_batch(pages, det_map_override=maps)
    assert _sig(k5_session.run_batch(pages, det_map_override=maps)) == _sig(a)
    t1 = k5_session.submit_batch_raw(pages, [960] * 4, [960] * 4, det_map_override=maps)
    t2 = k5_session.submit_batch_raw(pages, [960] * 4, [960] * 4, det_map_override=maps)
    for t in (t1, t2):
        r = k5_session.wait_batch_raw(t)
        try:
            got = [k5_session._collect(r, i) for i in range(4)]
        finally:
            k5_session._hd.lib.rt_results_free(r)
        assert _sig(got) == _sig(a)
    assert sum(len(g.tokens) for r in a for g in r.rec_result) > 0


def test_encoded_entry_equals_decoded(k5_session):
    pages = [workload.planted_page(960, 960, 32, seed=s)[0] for s in (401, 402)]
    files = [b"P6\n%d %d\n255\n" % (p.shape[1], p.shape[0]) + p.tobytes() for p in pages]
    a = k5_session.run_batch(pages)
    assert sum(len(g.tokens) for r in a for g in r.rec_result) > 0
    b = k5_session.run_encoded_batch(files)
    _same_but_candidates(a, b)
    assert _sig(b) == _sig(a)
    c = k5_session.wait_batch(k5_session.submit_encoded_batch(files))
    assert _sig(c) == _sig(a)


def test_fp16_server_session():
    """the PP-OCRv4 server graphs in fp16: same tokens with the option on and off; candidates consistent with them"""
    pages, maps = zip(*[_planted_for(960, 960, 16, s) for s in (401, 402)])
    outs = []
    for k in (5, 0):
        s = retto_amd.RettoSession(_cfg(k, server=True, dtype="f16"))
        try:
            outs.append(s.run_batch(list(pages), det_map_override=list(maps)))
        finally:
            s.close()
    n_classes = len(retto_amd.parse_dictionary(synth.synth_models(0)[3]))
    total = 0
    for r, q in zip(*outs):
        for g, h in zip(r.rec_result, q.rec_result):
            assert np.array_equal(g.tokens, h.tokens) and g.text == h.text and h.candidates is None
            assert len(g.candidates) == len(g.tokens)
            cols = [int(c) for c in g.token_cols]
            assert cols == sorted(set(cols))
            for t, cand in zip(g.tokens, g.candidates):
                ids = [c[0] for c in cand]; ps = [c[2] for c in cand]
                assert ids[0] == int(t) and len(set(ids)) == 5 and min(ids) >= 0 and max(ids) < n_classes
                assert all(0.0 <= p <= 1.0 for p in ps)
                assert all(ps[k + 1] <= ps[k] + PIPE_TOL for k in range(1, 4))
            total += len(g.tokens)
    assert total > 0
