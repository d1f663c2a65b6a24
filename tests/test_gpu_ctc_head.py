"""The fused CTC head on the MI355X, one launch at a time through rt_debug_gemm with ctc = 0, 1, 2 (k_gemm<8, 1>, the 256 x 240 and
the 128 x 128 wide tile with EPIM, each followed by k_argmax_merge), held to the fp64 reference of tests/ctc_head_ref.py: class
counts from 1 to 18385, row counts around the row tiles, planted ties at every stage that has to let the lowest column win, rows
of equal logits, rows of negative logits (a pad column holding 0 would win), large logits.  test_ctc_head_checks_cpu.py shows
that these cases refuse each wrong restatement of the head.  The device's worst |prob / ref - 1| per case is printed (-s)."""
import numpy as np
import pytest

import ctc_head_ref as R
from test_gpu_ops import AM128, AM256, AMN, CANARY, NONE, _up4, dev, run_gemm   # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

FORMS = ((0, AMN), (1, AM256), (2, AM128))


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_head_against_fp64(dev, case_id):
    c = R.case(case_id)
    got, worst = [], 0.0
    for form, kern in FORMS:
        out, plan, idx, prob = run_gemm(dev, c.A, R.K, c.W, c.bias, NONE, ctc=form, ldc=_up4(c.N))
        assert plan[0] == kern, (form, plan)
        assert (out.view(np.uint32) == CANARY).all(), "form %d: the logits reached the output buffer" % form
        got.append((form, idx, prob))
        worst = max(worst, R.deviation(c, prob))
    print("%s: worst |prob / ref - 1| %.3g (TOL_PROB %.3g)" % (case_id, worst, R.TOL_PROB))
    for form, idx, prob in got:
        try:
            R.check(c, idx, prob)
        except AssertionError as e:
            raise AssertionError("form %d: %s" % (form, e)) from None
    if c.planted:   # bit-equal columns are bit-equal logits in every kernel: the tie rule decides alone
        for form, idx, _ in got[1:]:
            differ = np.flatnonzero(idx != got[0][1])
            assert not len(differ), "form %d and form 0 differ on rows %s" % (form, differ[:8])
