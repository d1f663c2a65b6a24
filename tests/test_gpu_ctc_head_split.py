"""The split-bf16 CTC head (k_ctc_head_split, GemmKernel::argmax_split) on the MI355X: one launch per case of tests/ctc_head_ref.py
through rt_debug_gemm(variant = 40, ctc = 0), held to the same fp64 reference, tie rule and TOL_PROB as the fp32 forms
(test_gpu_ctc_head.py), and one page through the pipeline with the head switched on (rt_debug_set_variants flag bit 13).  The
device's worst |prob / ref - 1| per case is printed (-s)."""
import numpy as np
import pytest

import ctc_head_ref as R
from retto_amd import workload
from test_gpu_ops import AMN, CANARY, NONE, _up4, dev, run_gemm   # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

AMS = AMN + 1   # nn::GemmKernel::argmax_split


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_split_head_against_fp64(dev, case_id):
    c = R.case(case_id)
    out, plan, idx, prob = run_gemm(dev, c.A, R.K, c.W, c.bias, NONE, ctc=0, ldc=_up4(c.N), variant=40)
    assert plan[0] == AMS, plan
    assert (out.view(np.uint32) == CANARY).all(), "the logits reached the output buffer"
    print("%s: worst |prob / ref - 1| %.3g (TOL_PROB %.3g)" % (case_id, R.deviation(c, prob), R.TOL_PROB))
    R.check(c, idx, prob)
    if c.planted:   # bit-equal columns are bit-equal logits in both kernels: the tie rule decides alone
        _, plan0, idx0, _ = run_gemm(dev, c.A, R.K, c.W, c.bias, NONE, ctc=0, ldc=_up4(c.N), variant=0)
        assert plan0[0] == AMN, plan0
        differ = np.flatnonzero(idx != idx0)
        assert not len(differ), "the split head and form 0 differ on rows %s" % differ[:8]


def test_pipeline_split_head_equals_fp32_head(hip_session):
    """One 960 x 960 page of 8 planted lines with flags 0 and with 4096 | 8192: boxes, labels and token ids identical, line scores
    within 1e-5 (the bar of test_pipeline_split_bf16_equals_fp32_mfma_pipeline), at least one score another bit pattern -- at this
    size the wide layers stay on fp32, so only the head can have moved it."""
    lib, h = hip_session._hd.lib, hip_session._hd.h
    page, rects = workload.planted_page(960, 960, 8, seed=640)
    pmap = workload.planted_map(960, 960, 960, 960, rects)
    lib.rt_set_lanes(h, 1)
    try:
        base = hip_session.run_batch([page], det_map_override=[pmap])[0]
        lib.rt_debug_set_variants(0, 0, 4096 | 8192)
        got = hip_session.run_batch([page], det_map_override=[pmap])[0]
    finally:
        lib.rt_debug_set_variants(0, 0, 0)
        lib.rt_set_lanes(h, 1 << 20)
    assert len(base.det_result) == len(got.det_result) == 8
    assert np.array_equal(np.stack([d.boxes.as_array() for d in base.det_result]), np.stack([d.boxes.as_array() for d in got.det_result]))
    assert [c.label.label for c in base.cls_result] == [c.label.label for c in got.cls_result]
    scores = []
    for x, y in zip(base.rec_result, got.rec_result):
        assert np.array_equal(x.tokens, y.tokens) and x.text == y.text
        if x.score == x.score:
            scores.append((x.score, y.score))
    assert scores and max(abs(a - b) for a, b in scores) <= 1e-5, scores
    assert any(a != b for a, b in scores), "the split head did not run"
