"""Kernel-level numerics of the fp16 family (nn_f16.hip, nn_f16_dma.hip) beyond the plain conv, one launch at a time against the
fp64 references of tests/f16_kernel_ref.py (plain numpy; tests/test_f16_kernel_checks_cpu.py proves on the CPU that its checks
refuse a dropped tap, a wrong pitch, a wrong phase order ... and that a float32 computation passes them): nh::conv16's epilogue
and addressing forms through rt_debug_conv16x, the fifteen glue kernels through rt_debug_glue16.

Operands: sign * uniform[1/16, 1] rounded to fp16 (no operand and no product is subnormal), weights scaled by 4 / sqrt(K) (K = the
summed terms: Cin * kh * kw, or K * K for the depthwise), bias random per channel, LAB (1.3, 0.07); the gates' inputs span both
clamps and hold the clamp points and their float32 neighbours; max-pool inputs have all-negative images; means are taken over
0.5 + N(0, 1).  Batches are ragged, Cp = 24 for the glue so that idx % C8 is not a mask, inputs and outputs are views of wider
buffers (pitch and channel offset) where the nets use them so.  Every launch writes into a buffer filled with RT_DEBUG_CANARY
with 64 spare rows; everything outside the op's output must come back bit for bit.

conv16x cases (the route is asserted from the entry's report, not restated):
  residual      the classifier's linear convs 88 -> 16 and 200 -> 32, flat, no activation, residual at pitch ldy + 8, M = 1 / 255 /
                4100 (k_conv16, the narrow store path)
  LAB + hswish  48 -> 96 flat M = 300 (k_conv16, Cin < 64), 240 -> 240 flat M = 4100 (k_gemm16p, ragged last 256-row tile)
  pad channels  96 -> 18 (into channels 8 .. 31 of pitch 40) and 192 -> 42 (pitch 56) flat M = 257: channels N .. pitch8(N) are +0,
                the canary survives beyond them
  concat        one buffer of pitch 96, 3x3 32 -> 32 relu reading channels 32 .. 63 and writing 64 .. 95 in place on the ragged
                batch [(26, 100), (13, 37), (1, 1), (5, 16), (24, 17), (7, 2)] (k_conv16v2); 1x1 flat 64 -> 64 relu from channels
                0 .. 63 into 64 .. 127 of a pitch-128 buffer, M = 4100 (k_gemm16p, ldx != Cin)
  3x3 stride 2  64 -> 64 on the same ragged batch (k_conv16v2)
  phase convs   PFHeadLocal: Cin = 80, 2x2, N = 64, relu, dot epilogue, the four phases (a, b) with pads (1 - a, 1 - b) in sequence
                on one uniform(0, 1) map over [(16, 16), (1, 1), (3, 40), (17, 5)] at half resolution (the k_conv16v2 dot
                instance); each launch may change the pixels of its phase only, bit for bit

Three kinds of check (f16_kernel_ref.check):
  exact    pixel_shuffle16, upsample_into16 without a scale, maxpool16, map_window16, f32x4_to_h8, h_to_f32, f32_to_h equal the
           numpy reference (with numpy's round-to-nearest-even to float16 where the kernel rounds) bit for bit; pad channels
           (conv16's N .. pitch8(N), gate16's C .. Cp, u8_to_h8's 3 .. 7, f32x4_to_h8's 4 .. 7) are +0.
  arith    |err| <= U (T + 8) S L + Hout |y| + 2^-25, U = 2^-24, Hout = 2^-11 for an fp16 store (2^-23 for the fp32 outputs of
           global_mean16 and the hard-sigmoid gate16: the two roundings behind the stored value), T summed terms, S = |bias| +
           sum |w| |x| (+ |residual|), L = 1, or 1.5 |lab_a| after hardswish; and the rms error within twice that of the same
           operation in float32 numpy rounded once to the output type.  global_mean16: T = the image's pixels, S = mean |x|.
  sigmoid  gate16 with the ESE gate, deconv_to_map16 and the dot epilogue: |err| <= f (y (1 - y) A + c U y) + E with y the sigmoid,
           A = the bound of its fp32 argument (0 for gate16, whose argument is its input; U (C + 9) (|b| + sum |w| |f|) for the
           deconv; U ((4 Cin + 9) + (N + 9)) (|dot_b| + sum_n |dot_w| S_n) for the dot), f = 1 and E = 0 except for the dot
           epilogue, which stores 0.5 * (map + sigmoid): f = 0.5, E = 2 U |stored| for the one rounding of the sum.  c is not
           taken from the kernel: per op it is twice the worst case measured over that op's own inputs of what |err| leaves
           after the other terms, as a fraction of the |v| + 8 that exp2(v log2 e) with a 1-ulp v_exp_f32, one add and one
           divide allow (SIGMOID_FRAC_MEASURED; a measured value below zero means the other terms alone cover every error, and
           c is then 0).  The rms rule is not applied to this kind: numpy's float32 sigmoid is good to an ulp, the bound
           deliberately allows __expf more.

Measured on an MI355X, worst err / bound (rms error / float32 numpy's): dwconv16 0.88 ... 0.99 over the 23 cases (1.00: an fp16
store fills H |y| by construction, the ratio near 1 is the rounding to half itself); global_mean16 0.09 ... 0.13 (0.65 ... 0.85);
gate16 hard-sigmoid 0.06 ... 0.09 (0.73 ... 1.06); scale_channels16 0.95 ... 0.98 (1.00); upsample_add16 0.99 ... 1.00 (1.00);
upsample_into16 with a scale 0.91 ... 0.96 (1.00); avgpool16 0.995 (1.00); u8_to_h8 0.93 (1.00).
conv16x, worst err / bound, rms ratio 1.00 in every case (the same rounding to half): residual 88 -> 16 at M = 1 / 255 / 4100 0.47 /
0.91 / 0.96, 200 -> 32 0.51 / 0.86 / 0.89 (k_conv16); LAB + hswish 48 -> 96 0.94 (k_conv16), 240 -> 240 0.80 (k_gemm16p); pad
channels 96 -> 18 0.91, 192 -> 42 0.88 (k_conv16), the pad channels +0; concat in place 3x3 ragged 0.83 (k_conv16v2), 1x1 flat
0.97 (k_gemm16p); ragged 3x3 stride 2 0.71 (k_conv16v2); the four phase convs with the dot epilogue 0.016 (the k_conv16v2
dot instance), every launch changing its own phase's pixels only.
The sigmoid constants, measured fraction of |v| + 8 left after the other terms of the bound: gate16 0.497 over its 220 inputs
(|v| <= 12; used 0.994, worst err / bound 0.50, and 0.97 with the + 1); deconv_to_map16 -0.386 (C = 24) and -0.407 (C = 64) over
276 map pixels each; the dot epilogue -6.197 over 1848 map pixels.  The last two are below zero -- the error of the fp32 argument
that the bound already allows covers __expf's -- so c = 0 there and the bound is y (1 - y) A (+ E) alone: worst err / bound
0.19 / 0.10 for the deconv."""
import numpy as np
import pytest

import f16_kernel_ref as R

pytestmark = pytest.mark.gpu

# c of the sigmoid bound as a fraction of |v| + 8, per op: the worst (|err| - the rest of the bound) / ((|v| + 8) U y) over that
# op's own inputs, measured on an MI355X; the tests use twice it
SIGMOID_FRAC_MEASURED = {"gate16": 0.497, "deconv_to_map16": -0.386, "conv16x": -6.197}


def sigmoid_frac(c):
    frac = 2 * max(SIGMOID_FRAC_MEASURED[c.name.split()[0]], 0.0)
    assert frac <= 1, "c above |v| + 8: __expf would be worse than a 1-ulp exp2 allows"
    return frac


@pytest.fixture(scope="module")
def dev(hip_session):
    return hip_session._hd.lib, hip_session._hd.h


def run(dev, c):
    lib, h = dev
    hs = [np.array(v, np.int32) for v in ([a for a, _ in c.src], [b for _, b in c.src], [a for a, _ in c.dst], [b for _, b in c.dst])]
    out = np.zeros((c.out_rows + 64) * c.out_ld, np.float32)
    arr = lambda a: (np.ascontiguousarray(a, np.float32), ) if a is not None else (None, )   # noqa: E731
    (x,), (x2,), (tab,) = arr(c.x), arr(c.x2), arr(c.tab)
    ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    n = lambda a: a.size if a is not None else 0   # noqa: E731
    rc = lib.rt_debug_glue16(h, c.op, c.ip.ctypes.data, c.fp.ctypes.data, hs[0].ctypes.data, hs[1].ctypes.data, hs[2].ctypes.data,
                             hs[3].ctypes.data, len(c.src), ptr(x), n(x), ptr(x2), n(x2), ptr(tab), n(tab), out.ctypes.data, out.size)
    assert rc == 0, lib.rt_last_error(h)
    return out


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_glue16_against_fp64(dev, case_id):
    c = R.case(case_id)
    out = run(dev, c)
    fig = R.check(c, out, sig_frac=sigmoid_frac(c) if c.kind == "sigmoid" else 1.0)
    print("FIG %s %s" % (case_id, " ".join("%s=%.4g" % kv for kv in sorted(fig.items()))))


def test_global_mean16_is_deterministic(dev):
    c = R.case("global_mean16-Cp200")
    assert np.array_equal(run(dev, c).view(np.uint32), run(dev, c).view(np.uint32))



def run_conv(dev, c, ip, w, b, out):
    """one rt_debug_conv16x launch; out goes in (the map of the dot epilogue) and comes back whole"""
    lib, h = dev
    hs, ws = np.array([a for a, _ in c.src], np.int32), np.array([a for _, a in c.src], np.int32)
    x, w, b = np.ascontiguousarray(c.x, np.float32), np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    res = np.ascontiguousarray(c.res, np.float32) if c.res is not None else None
    route = np.zeros(1, np.int32)
    rc = lib.rt_debug_conv16x(h, ip.ctypes.data, c.fp.ctypes.data, hs.ctypes.data, ws.ctypes.data, len(c.src), x.ctypes.data, x.size,
                              w.ctypes.data, w.size, b.ctypes.data, res.ctypes.data if res is not None else None,
                              res.size if res is not None else 0, c.dot_w.ctypes.data if c.dot_w is not None else None,
                              out.ctypes.data, out.size, route.ctypes.data)
    assert rc == 0, lib.rt_last_error(h)
    return int(route[0])


@pytest.mark.parametrize("case_id", [i for i in R.CONV_CASE_IDS if i != "conv16x-phase-dot"])
def test_conv16x_against_fp64(dev, case_id):
    c = R.case(case_id)
    out = np.zeros((c.out_rows + 64) * c.out_ld, np.float32)
    route = run_conv(dev, c, c.ip, c.w, c.b, out)
    assert route == c.route, "%s ran on %s, expected %s" % (c.name, R.ROUTE_NAMES.get(route, route), R.ROUTE_NAMES[c.route])
    fig = R.check(c, out)
    print("FIG %s route=%s %s" % (case_id, R.ROUTE_NAMES[route], " ".join("%s=%.4g" % kv for kv in sorted(fig.items()))))


def test_conv16x_phase_convs_with_the_dot_epilogue(dev):
    """the four PFHeadLocal phase convs in sequence on one map: each launch changes the pixels of its phase and nothing else, and
    after the four every pixel is 0.5 * (map + sigmoid) of its own phase's conv"""
    c = R.case("conv16x-phase-dot")
    m = np.concatenate([c.in_place, np.zeros(64, np.float32)])
    for a in range(2):
        for b in range(2):
            before = m.copy()
            route = run_conv(dev, c, c.ip_of(a, b), c.w[2 * a + b], c.b[2 * a + b], m)
            assert route == c.route, "phase (%d, %d) ran on %s" % (a, b, R.ROUTE_NAMES.get(route, route))
            if (a, b) == (0, 0):   # (the entry overwrites the 64 spare floats with the canary on its first launch)
                before[-64:] = m[-64:]
                assert (m[-64:].view(np.uint32) == R.CANARY).all()
            c.check_step(before, m, a, b, sig_frac=sigmoid_frac(c))
    fig = R.check(c, m, sig_frac=sigmoid_frac(c))
    print("FIG conv16x-phase-dot route=%s %s" % (R.ROUTE_NAMES[c.route], " ".join("%s=%.4g" % kv for kv in sorted(fig.items()))))
