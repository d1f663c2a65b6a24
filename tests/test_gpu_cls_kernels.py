"""Kernel-level numerics of the classifier's blocks, the three stems and the fp32 squeeze-excite / pooling / softmax glue, one
launch (or one launch series) at a time through rt_debug_cls_block, rt_debug_stem and rt_debug_glue32 against the fp64 references
of tests/cls_kernel_ref.py (its docstring derives every bound; tests/test_cls_kernel_checks_cpu.py proves on the CPU that the
checks refuse twenty plausible errors and that a float32 torch computation passes them).

Operands are uniform(-1, 1) float32 with full significands, 1x1 weights scaled by 4 / sqrt(K), every bias random per channel,
squeeze-excite weights scaled so that the hard-sigmoid reaches both clamps and its linear part.  Every launch writes into buffers
filled with RT_DEBUG_CANARY with 64 spare rows, and every element of every returned buffer is checked: against the reference
inside the op's output, bit for bit against the canary outside it, +0 in the scales and scaled pixels past C.  The rms rule: a
kernel's rms error is within twice that of the float32 torch form on the CPU.

Cases (cls_kernel_ref.CASE_IDS; the instance that ran is asserted from the entry's report):
  blk0 .. blk10     the eleven CLS_SPEC blocks at their production shapes (3 crops of 24x96 -> 12x96 -> 6x96 -> 6x96 -> 3x96 ... ->
                    2x96, crop 1 scaled by 0.05), each as the launch series (f0) and as k_cls_block (f1)
  edge-*            form 1: one and two tile columns, odd height at stride 2, H = 1 with k = 5 and at stride 2, 40 / 41 row tiles
                    on the padded layout (MAXU 5 / 9), 72 tiles on the swizzled one, both sides of the 96 KB switch
  refused-*         form 1 on W = 24, 73 row tiles, cin = 36, mid = 520: the series must run and meet the bound
  stem8 / 16 / 16-u8   k_stem<8>, k_stem_mfma<0>, k_stem_mfma<1> on one ragged list with full and partial 8 x 32 tiles, odd and even
                    extents and images below the window; the U8 output also equals the tensor path's bit for bit
  se-c*-r*-a*       se_scale at C = 8 / 48 / 88 / 200 / 480 (scalar and vector FC2, 256 and 1024 threads, pitch 224, slope 1/6) on
                    images of 1, 127, 128, 129 and 300 pixels, residual 0 / 1, with and without scale_channels in place
  gmean, maxpool, avgpool, softmax / argmax_prob / argmax at C = 2 (ld 4), 257, 6625 with ties, an equal row, a last-index maximum
  repeatability     every block case twice, bit for bit

What was measured (worst err / bound with the torch float32 figure beside it in brackets; rms ratio = kernel / torch float32).
On an MI355X, the first run of this file on the unmodified kernels, all cases passing:
  blocks, series (f0)       5.7e-5 ... 0.016 (4.1e-5 ... 0.011), rms ratio 0.99 ... 1.24
  blocks, k_cls_block (f1)  4.8e-5 ... 0.016 (4.1e-5 ... 0.011), 1.00 ... 1.26; blk0, blk1 ran swizzle / MAXU 9, blk2 .. 10 padded / MAXU 5
  edge shapes               1.3e-4 ... 0.023 (1.4e-4 ... 0.017), 0.97 ... 1.14; -w16, -w32, -h5-s2, -h1-k5, -h1-s2, -40tiles-pad5: padded /
                            MAXU 5; -41tiles-pad9-k3, -k5se, -s2 and -96k-below: padded / MAXU 9; -72tiles-swz-k5se, -k3, -swz-k5-s2
                            and -96k-above: swizzle / MAXU 9
  refused shapes            1.1e-5 ... 0.012 (6.5e-6 ... 0.011), 1.03 ... 1.38, all on the launch series
  stem8 / 16 / 16-u8        0.084 / 0.127 / 0.096 (0.071 / 0.085 / 0.086), 1.18 / 1.06 / 0.99
  se_scale                  9.2e-5 ... 0.060 (1.3e-4 ... 0.051), scales 0.56 ... 1.10, scaled x 0.79 ... 1.20
  global_mean, avgpool      0.019 (0.016), 1.14; 0.344 (0.344), 1.00
  softmax 2 / 257 / 6625    0.49 / 0.18 / 0.011 (0.28 / 0.11 / 0.0051), 1.00 / 0.91 / 1.33
  argmax_prob 2 / 257 / 6625   0.096 / 0.0038 / 2.5e-4, 1.00 / 0.80 / 0.83;  maxpool, argmax, every index: equal
The blocks sit at 1e-4 ... 2e-2 of their composed bounds: each stage's worst case is carried through sum |w| of the next.  That
margin is recorded, not tuned; the rms rule is the tight check.  From the CPU stand-in alone (no GPU): the mutant figures of
tests/test_cls_kernel_checks_cpu.py.  docs/HISTORY.md has the tables."""
import ctypes as C

import numpy as np
import pytest

import cls_kernel_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_session):
    return hip_session._hd.lib, hip_session._hd.h


def P(a):
    return None if a is None else a.ctypes.data


def run_block(dev, c, form=None):
    lib, h = dev
    f = [np.ascontiguousarray(a, np.float32) for a in (c.fc if c.se else ())] or [None] * 4
    ops = [np.ascontiguousarray(a, np.float32) for a in (c.x, c.exp_w, c.exp_b, c.dw_w, c.dw_b, c.lin_w, c.lin_b)]
    out = np.zeros(c.reference()[0].shape, np.float32)
    info = (C.c_int * 4)()
    rc = lib.rt_debug_cls_block(h, P(ops[0]), c.n, c.H, c.W, c.cin, c.mid, c.cout, c.k, c.sh, c.act, int(c.se), P(ops[1]), P(ops[2]),
                                P(ops[3]), P(ops[4]), P(f[0]), P(f[1]), P(f[2]), P(f[3]), P(ops[5]), P(ops[6]),
                                c.form if form is None else form, P(out), info)
    assert rc == 0, lib.rt_last_error(h)
    return [out], tuple(info)


def run_stem(dev, c, x4=None):
    """x4: run the tensor path on these floats instead of the case's own input"""
    lib, h = dev
    hs, ws = (np.array(v, np.int32) for v in zip(*c.imgs))
    w, b = np.ascontiguousarray(c.w, np.float32), np.ascontiguousarray(c.b, np.float32)
    out = np.zeros(c.reference()[0].shape, np.float32)
    mean, std = np.array(R.DET_MEAN, np.float32), np.array(R.DET_STD, np.float32)
    u8 = c.u8 and x4 is None
    src = np.ascontiguousarray(c.rgb) if u8 else np.ascontiguousarray(c.x4 if x4 is None else x4, np.float32)
    rc = lib.rt_debug_stem(h, None if u8 else P(src), P(src) if u8 else None, P(hs), P(ws), len(c.imgs), c.cout, P(w), P(b), c.act,
                           R.DET_SCALE, P(mean), P(std), P(out), out.size)
    assert rc == 0, lib.rt_last_error(h)
    return [out]


def run_glue(dev, c):
    lib, h = dev
    refs = c.reference()
    ip = np.zeros(8, np.int32); ip[:len(c.ip)] = c.ip   # noqa: E702
    fp = np.zeros(4, np.float32); fp[:len(c.fp)] = c.fp   # noqa: E702
    rows_op = c.imgs is None
    hs, ws = (None, None) if rows_op else (np.array(v, np.int32) for v in zip(*c.imgs))
    x = np.ascontiguousarray(c.x, np.float32)
    wts = [np.ascontiguousarray(a, np.float32) for a in c.w] if c.w is not None else []
    wp = (C.c_void_p * 4)(*[a.ctypes.data for a in wts]) if wts else None
    out = np.zeros(refs[0].shape, np.float32)
    second = refs[1] if len(refs) > 1 else None
    out2 = np.zeros(second.shape, np.float32) if second is not None and second.kind != "index" else None
    idx = np.zeros(second.shape, np.int32) if second is not None and second.kind == "index" else None
    rc = lib.rt_debug_glue32(h, R.GLUE_OPS.index(c.op), P(ip), P(fp), P(hs), P(ws), c.rows if rows_op else len(c.imgs), P(x), x.size, wp,
                             P(out), out.size, P(out2), 0 if out2 is None else out2.size, P(idx))
    assert rc == 0, lib.rt_last_error(h)
    return [out] + [a for a in (out2, idx) if a is not None]


def report(case_id, fig, extra=""):
    print("FIG %s %s%s" % (case_id, extra, " ".join("%s=%.4g" % kv for kv in sorted(fig.items()))))


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("case_id", R.BLOCK_IDS)
def test_cls_block_against_fp64(dev, case_id):
    c = R.case(case_id)
    outs, info = run_block(dev, c)
    assert info[:3] == c.info, "%s ran as %s" % (c.name, R.INSTANCE.get(info[:3], info))
    assert (info[3] > 0) == (c.info != R.SERIES) and info[3] <= 160 * 1024
    report(case_id, R.check(c, outs), "instance=[%s] lds=%d " % (R.INSTANCE[info[:3]], info[3]))
    again, info2 = run_block(dev, c)
    assert info2 == info and same_bits(outs, again), "%s: two runs differ" % c.name


def test_the_fused_cases_reach_every_workgroup_shape(dev):
    """over the reports of the entry: all three workgroup shapes, each with k 3 and 5, stride 1 and 2, squeeze-excite on and off"""
    seen = {}
    for case_id in R.BLOCK_IDS:
        c = R.case(case_id)
        if c.form and c.info != R.SERIES:
            _, info = run_block(dev, c)
            seen.setdefault(info[:3], set()).add((c.k, c.sh, c.se))
    assert set(seen) == {R.SWZ9, R.PAD9, R.PAD5}
    for inst, combos in seen.items():
        assert {k for k, _, _ in combos} == {3, 5} and {sh for _, sh, _ in combos} == {1, 2} and {se for _, _, se in combos} == {True, False}, (inst, combos)


@pytest.mark.parametrize("case_id", R.STEM_IDS)
def test_stem_against_fp64(dev, case_id):
    c = R.case(case_id)
    outs = run_stem(dev, c)
    report(case_id, R.check(c, outs))
    if c.u8:   # the page path stages the floats of k_det_normalize: the tensor path on those floats gives the same bits
        assert same_bits(outs, run_stem(dev, c, x4=c.x4))


@pytest.mark.parametrize("case_id", R.GLUE_IDS)
def test_glue_against_fp64(dev, case_id):
    c = R.case(case_id)
    outs = run_glue(dev, c)
    report(case_id, R.check(c, outs))
    if c.op == "se_scale":   # (the summation orders are fixed by the layer alone: repeatable)
        assert same_bits(outs, run_glue(dev, c))
