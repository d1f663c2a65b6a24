"""Kernel-level numerics of the fp32 depthwise kernels (k_dwconv_rows, k_dwconv_sweep: one launch through rt_debug_dwconv) and of
the wide LCNetV3 blocks run_lc builds from them (depthwise, squeeze-excite from the depthwise kernel's partial sums, pointwise GEMM
with the scales folded into its A rows, or run_se in place: rt_debug_lc_wide) against the fp64 references of tests/dw_kernel_ref.py
(its docstring derives every bound; tests/test_dw_kernel_checks_cpu.py proves on the CPU that the checks refuse nineteen plausible
errors, that a float32 torch computation passes them, and that the case table reaches what the plan picks).

Every launch writes into buffers filled with RT_DEBUG_CANARY with 64 spare rows, and every element of every returned buffer is
checked: against the reference inside the op's output, bit for bit against the canary outside it (the rows past the last image, the
partial-sum slots of blocks an image does not own, the block output's columns past cout), +0 in the pad channels (the input's pad
channels hold noise).  One exception: the partial sums and the means of a pooled depthwise launch come back without spare rows
(run_dw below), so past their last row nothing is checked; inside them every slot is.  The rms rule: a kernel's rms error per
buffer is within twice that of the float32 torch form on the CPU.

Cases (dw_kernel_ref.CASE_IDS; what ran is asserted from rt_debug_dw_plan and from rt_debug_lc_wide's report, never restated):
  det-* / rec-*      one depthwise launch per kernel instance the networks reach, with the layer's real epilogue, on a ragged batch
                     of five images (68 / 33 / 7 / 1 pixels wide, a partial last strip, images below a strip, 1 x 1; on 6-row maps
                     a 4 x 68 image, whose strip count depends on the plan's 3-row strips); -pool: with
                     the squeeze-excite partial sums and the means k_se_fc reads from them; -x8: eight images, so that
                     k_dwconv_rows takes its XCD remap (asserted from the plan's grid); -rows: the same operands with the sweep off
  blk-*              the 13 wide block shapes of DET_SPEC / REC_SPEC on a small ragged batch (squeeze-excite: run_se in place), and
                     the four squeeze-excite blocks folded: -fold128 / -fold240 at the first M at which gemm_plan() takes the
                     128 x 128 / 128 x 240 "+se" tile (neighbouring images of 130 .. 138 pixels, in the rec batches a 4-row
                     line among them, then one large image), -minpix the same size with one image of 126 pixels (the fold
                     is refused: run_se)
  twins              a case that runs the sweep and its -rows twin return the same bits in every buffer
  repeatability      every case twice, bit for bit

What was measured (docs/HISTORY.md, "the depthwise kernels and the wide LCNetV3 blocks against fp64", has the tables).  On an
MI355X, on the unmodified kernels, all 104 tests passing; worst err / bound with the torch float32
figure in brackets, rms ratio = kernel / torch float32:
  depthwise, rows / sweep    0.10 ... 0.25 (0.092 ... 0.26), y 0.87 ... 1.06; partial sums 0.20 ... 0.33, means 0.78 ... 1.04
  blocks, small batches      0.011 ... 0.25 (0.015 ... 0.34), y 0.93 ... 1.60 (rising with the GEMM's K), y1 0.67 ... 1.03, scales 0.50 ... 0.69
  folded 128 x 128 / 240     0.13 ... 0.16 (0.13 ... 0.15), y 1.00 ... 1.53, y1 0.99 ... 1.06, scales 0.56 ... 0.85
  fold refused (126 pixels)  0.021, 0.028 (0.015, 0.020), y 1.2, 1.33"""
import ctypes as C

import numpy as np
import pytest

import dw_kernel_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_session):
    return hip_session._hd.lib, hip_session._hd.h


def P(a):
    return None if a is None else a.ctypes.data


def canary(shape):
    return np.full(shape, R.CANARY, np.uint32).view(np.float32)


def dw_plan(lib, c):
    plan = (C.c_int * 8)()
    assert lib.rt_debug_dw_plan(c.K, c.sh, c.sw, c.Cp, c.maxHo, c.maxWo, int(c.pooled), c.form, plan) == 0
    return tuple(plan)


def run_dw(dev, c):
    lib, h = dev
    refs = c.reference()
    hs, ws = (np.array(v, np.int32) for v in zip(*c.imgs))
    x, w, b = (np.ascontiguousarray(a, np.float32) for a in (c.x, c.w, c.b))
    out = np.zeros(refs[0].shape, np.float32)
    # rt_debug_dwconv returns the partial sums and the means without spare rows.  The 64 canary rows check() expects past them are
    # written here on the host and never reach the device: they check nothing.  What the device's canary does hold in `part` are the
    # slots inside [image][chunks] that an image does not own; a write past the end of either device buffer would go unseen.
    part = canary(refs[1].shape) if c.pooled else None
    mean = canary(refs[2].shape) if c.pooled else None
    info = (C.c_int * 4)()
    la, lc = c.lab if c.lab else (1.0, 0.0)
    rc = lib.rt_debug_dwconv(h, P(x), P(hs), P(ws), len(c.imgs), c.C, c.Cp, c.K, c.sh, c.sw, P(w), P(b), c.act, 1 if c.lab else 0, la, lc,
                             int(c.pooled), c.form, P(out), P(part), 0 if part is None else part.size - 64 * c.Cp, P(mean), info)
    assert rc == 0, lib.rt_last_error(h)
    return [out] + ([part, mean] if c.pooled else []), tuple(info)


def run_lc(dev, c):
    lib, h = dev
    refs = c.reference()
    hs, ws = (np.array(v, np.int32) for v in zip(*c.imgs))
    ops = [np.ascontiguousarray(a, np.float32) for a in (c.x, c.dw_w, c.dw_b, c.pw_w, c.pw_b)]
    fc = [np.ascontiguousarray(a, np.float32) for a in c.fc] if c.se else [None] * 4
    out, y1 = np.zeros(refs[0].shape, np.float32), np.zeros(refs[1].shape, np.float32)
    scale = np.zeros(refs[2].shape, np.float32) if c.se else None
    info = (C.c_int * 16)()
    la, lc = c.lab if c.lab else (1.0, 0.0)
    rc = lib.rt_debug_lc_wide(h, P(ops[0]), P(hs), P(ws), len(c.imgs), c.K, c.cin, c.cout, c.sh, c.sw, P(ops[1]), P(ops[2]), P(ops[3]),
                              P(ops[4]), c.act, 1 if c.lab else 0, la, lc, 1, R.LAB_PW[0], R.LAB_PW[1], P(fc[0]), P(fc[1]), P(fc[2]),
                              P(fc[3]), c.form, P(out), out.size, P(y1), y1.size, P(scale), 0 if scale is None else scale.size, info)
    assert rc == 0, lib.rt_last_error(h)
    return [out, y1] + ([scale] if c.se else []), tuple(info)


def report(case_id, fig, extra=""):
    print("FIG %s %s%s" % (case_id, extra, " ".join("%s=%.4g" % kv for kv in sorted(fig.items()))))


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("case_id", R.DW_IDS)
def test_depthwise_against_fp64(dev, case_id):
    c = R.case(case_id)
    plan = dw_plan(dev[0], c)
    assert plan == c.plan, "%s: the plan is %s, the case was built for %s" % (c.name, plan, c.plan)
    assert R.instance_name(plan, c.K, c.sh, c.sw, c.pooled) == c.instance
    remap = R.takes_xcd_remap(plan, len(c.imgs))
    assert remap == c.remap and (remap or "-x8" not in case_id)
    outs, info = run_dw(dev, c)
    assert info[3] == (1 if plan[0] == R.SWEEP else 0)
    assert not c.pooled or info[:3] == (plan[5], plan[2], plan[4])
    report(case_id, R.check(c, outs), "instance=[%s] remap=%d " % (c.instance, remap))
    again, info2 = run_dw(dev, c)
    assert info2 == info and same_bits(outs, again), "%s: two runs differ" % c.name


@pytest.mark.parametrize("case_id", R.BLOCK_IDS)
def test_wide_block_against_fp64(dev, case_id):
    c = R.case(case_id)
    outs, info = run_lc(dev, c)
    assert info[0] == 0, "%s took the fused route %d" % (c.name, info[0])
    assert info[1:9] == c.plan, "%s: depthwise plan %s, the case was built for %s" % (c.name, info[1:9], c.plan)
    gemm = R.GEMM_KERNELS[info[10]] if info[10] < len(R.GEMM_KERNELS) else str(info[10])
    if c.scaled == "fold":      # the scales folded into the register-staged "+se" tile the case is named for, 2-int table
        assert info[9] == 128 and info[11] == 1 and info[12] == 1, info
        assert gemm == ("wide_128x240" if "fold240" in case_id else "wide_128x128"), gemm
    else:
        assert info[9] == 0 and info[11] == 0 and info[12] == (2 if c.se else 0), info
    report(case_id, R.check(c, outs), "dw=[%s] gemm=%s se_rows=%d " % (R.instance_name(info[1:9], c.K, c.sh, c.sw, c.scaled == "fold"), gemm, info[9]))
    again, info2 = run_lc(dev, c)
    assert info2 == info and same_bits(outs, again), "%s: two runs differ" % c.name


@pytest.mark.parametrize("pair", R.TWINS, ids=[a for a, _ in R.TWINS])
def test_sweep_equals_rows_bit_for_bit(dev, pair):
    a, b = (R.case(i) for i in pair)
    run = run_lc if a.family == "block" else run_dw
    (oa, ia), (ob, ib) = run(dev, a), run(dev, b)
    if a.family == "block":
        assert ia[1] == R.SWEEP and ib[1] != R.SWEEP, (ia, ib)
    else:
        assert ia[3] == 1 and ib[3] == 0, (ia, ib)
    names = ("y", "y1", "scale") if a.family == "block" else ("y", "partial", "mean")
    assert len(oa) == len(ob)
    for name, x, y in zip(names, oa, ob):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: the sweep differs from the row kernel in %s" % (a.name, name)
