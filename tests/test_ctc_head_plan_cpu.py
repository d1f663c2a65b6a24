"""nn::gemm_plan() on the CTC head's shape with the split switch at 2 (the head joins the split path) and at 1 (it stays on the
fp32 narrow kernel, as before the split head existed).  Through tests/native/gemm_plan_driver.cpp, whose kernel_name() prints
`?` for GemmKernel::argmax_split.  No GPU."""
import pytest

import plan_driver
from test_gemm_plan_cpu import plan_query

HEAD = dict(M=5000, K=120, N=6625, am=1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return plan_driver.build(tmp_path_factory)


@pytest.mark.parametrize("what,kw,want", [
    ("split = 2: the split head, one workgroup per 128 rows", dict(split=2), "? 0 0 0 0 40 1 gemm_ctc_fc"),
    ("variant 40 forces it", dict(variant=40), "? 0 0 0 0 40 1 gemm_ctc_fc"),
    ("split = 1 keeps its meaning", dict(split=1), "argmax_narrow 8 0 1 0 40 52 gemm_ctc_fc"),
    ("K = 128 has no channel left for the bias", dict(split=2, K=128), "argmax_narrow 8 0 1 0 40 52 gemm_ctc_fc"),
    ("the wide fp32 forms stay what they are", dict(split=2, amw=2), "argmax_128x128 0 0 0 0 40 52 gemm_ctc_fc"),
])
def test_head_plan(driver, what, kw, want):
    assert plan_driver.run(driver, [plan_query(**{**HEAD, **kw})]) == [want], what
