"""The column-sweep depthwise kernel (k_dwconv_sweep) on the recognition net's strided and squeeze-excite layers, one launch at
a time through rt_debug_dwconv: ragged batches of 3 images, 7 / 33 / 100 pixels wide (no multiple of the 4-pixel column, one
narrower than a block).

(a) the sweep (form 1) equals the row-strip kernel (form 0) bit for bit: the outputs, the pooled partial sums as they lie in
    memory, and the channel means k_se_fc reads from them;
(b) the sweep is within 2^-24 (K K + 2) sum |w| |x| per output of an fp64 depthwise conv of the same data.  This run has no
    activation and a zero bias: the bound is that of the K K roundings of the tap sum, and has no term for the roundings a
    large bias would add.  The bias-first order is held by (a), with a random bias, hardswish and the learnable affine;
(c) two runs of the sweep are bit-identical.

The pooled means are also held to the fp64 mean of the launch's own outputs: (n + 2) 2^-24 mean |y| for n pixels, the bound of
an n-term fp32 sum in any order, the rounding of 1 / n and the product."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE, HSWISH = 0, 2
U = 2.0 ** -24
LAB = (1.3, 0.07)
WIDTHS = (7, 33, 100)

# (name, K, sh, sw, pooled, (C, Cp) ..., input heights, heights at which the layer has a sweep instance)
LAYERS = [
    ("s6.1", 5, 1, 1, 1, ((480, 480), (240, 256)), (12, 6), (6,)),          # pooled: 3-row strips (6-row maps) only
    ("s6.2", 5, 2, 1, 0, ((480, 480), (240, 256)), (12, 6), (12, 6)),
    ("s6.0", 5, 2, 1, 1, ((240, 256), (480, 480)), (12, 6), (12,)),         # 12 -> 6 rows: 3-row strips
    ("s5.0", 3, 1, 2, 0, ((128, 128),), (24, 12, 6), (24, 12)),             # 6-row maps: 32-channel slabs, row kernel
]
CASES = [(name, K, sh, sw, pooled, c, cp, (h, h, h), h in swept)
         for name, K, sh, sw, pooled, chans, heights, swept in LAYERS for c, cp in chans for h in heights]
# images of different heights in one batch: columns that cross one and two pooling strips
CASES += [("s6.1", 5, 1, 1, 1, 480, 480, (6, 4, 3), True), ("s6.0", 5, 2, 1, 1, 240, 256, (12, 11, 5), True),
          ("s6.2", 5, 2, 1, 0, 480, 480, (11, 12, 1), True), ("s5.0", 3, 1, 2, 0, 128, 128, (24, 13, 2), True)]


def _run(dev, x, heights, c, cp, K, sh, sw, w, bias, act, lab, pooled, form):
    lib, h = dev
    n = len(heights)
    hs = np.asarray(heights, np.int32)
    ws = np.asarray(WIDTHS, np.int32)
    pout = sum(((a + sh - 1) // sh) * ((b + sw - 1) // sw) for a, b in zip(heights, WIDTHS))
    out = np.empty((pout + 64, cp), np.float32)
    cap = 1 << 20
    part = np.zeros(cap, np.float32)
    mean = np.zeros((n, cp), np.float32)
    info = (C.c_int * 4)()
    la, lc = lab if lab else (1.0, 0.0)
    rc = lib.rt_debug_dwconv(h, x.ctypes.data, hs.ctypes.data, ws.ctypes.data, n, c, cp, K, sh, sw, w.ctypes.data, bias.ctypes.data,
                             act, 1 if lab else 0, la, lc, pooled, form, out.ctypes.data, part.ctypes.data, cap, mean.ctypes.data,
                             info)
    assert rc == 0, lib.rt_last_error(h)
    return out, part[:n * info[0] * cp].copy(), mean, tuple(info)


def _ref64(x, heights, c, cp, K, sh, sw, w):
    """fp64 depthwise conv ('same' padding K // 2) and sum |w| |x| per output, images concatenated as the kernel lays them out."""
    P = K // 2
    w64 = w.astype(np.float64).reshape(K, K, cp)
    refs, mags = [], []
    off = 0
    for hh, ww in zip(heights, WIDTHS):
        img = x[off:off + hh * ww].astype(np.float64).reshape(hh, ww, cp)
        off += hh * ww
        ho, wo = (hh + sh - 1) // sh, (ww + sw - 1) // sw
        pad = np.zeros((hh + 2 * P + sh, ww + 2 * P + sw, cp))
        pad[P:P + hh, P:P + ww] = img
        r = np.zeros((ho, wo, cp))
        m = np.zeros((ho, wo, cp))
        for dy in range(K):
            for dx in range(K):
                v = pad[dy:dy + (ho - 1) * sh + 1:sh, dx:dx + (wo - 1) * sw + 1:sw]
                r += v * w64[dy, dx]
                m += np.abs(v) * np.abs(w64[dy, dx])
        r[..., c:] = 0.0
        refs.append(r.reshape(-1, cp))
        mags.append(m.reshape(-1, cp))
    return np.concatenate(refs), np.concatenate(mags)


@pytest.fixture(scope="module")
def dev(hip_session):
    return hip_session._hd.lib, hip_session._hd.h


@pytest.mark.parametrize("name,K,sh,sw,pooled,c,cp,heights,swept", CASES,
                         ids=["%s-c%d-h%s" % (t[0], t[5], "_".join(map(str, t[7]))) for t in CASES])
def test_sweep_equals_rows_and_fp64(dev, name, K, sh, sw, pooled, c, cp, heights, swept):
    rng = np.random.default_rng(1000 * K + 100 * sh + 10 * sw + c + sum(heights))
    npix = sum(a * b for a, b in zip(heights, WIDTHS))
    x = np.zeros((npix, cp), np.float32)
    x[:, :c] = rng.uniform(-1, 1, (npix, c)).astype(np.float32)
    w = np.zeros((K * K, cp), np.float32)
    w[:, :c] = rng.uniform(-1, 1, (K * K, c)).astype(np.float32)
    bias = np.zeros(cp, np.float32)
    bias[:c] = rng.uniform(-1, 1, c).astype(np.float32)

    rows = _run(dev, x, heights, c, cp, K, sh, sw, w, bias, HSWISH, LAB, pooled, 0)
    sweep = _run(dev, x, heights, c, cp, K, sh, sw, w, bias, HSWISH, LAB, pooled, 1)
    again = _run(dev, x, heights, c, cp, K, sh, sw, w, bias, HSWISH, LAB, pooled, 1)
    assert sweep[3][3] == (1 if swept else 0), "the layer's route changed: info %s" % (sweep[3],)
    assert rows[3][3] == 0, "form 0 ran the sweep"
    pout = sweep[0].shape[0] - 64
    # (a) bit for bit, canary rows past the end and pitch padding included
    for i, what in enumerate(("outputs", "pooled partial sums", "pooled means")):
        assert np.array_equal(rows[i].view(np.uint32), sweep[i].view(np.uint32)), "%s: sweep differs from the row kernel in %s" % (name, what)
        assert np.array_equal(sweep[i].view(np.uint32), again[i].view(np.uint32)), "%s: two sweep runs differ in %s" % (name, what)   # (c)
    assert np.all(sweep[0][pout:].view(np.uint32) == 0x7FA5C3E1), "wrote past the last image"
    assert np.all(sweep[0][:pout, c:] == 0.0) and np.all(np.isfinite(sweep[0][:pout]))
    if pooled:
        y = sweep[0][:pout].astype(np.float64)
        off = 0
        for i, (hh, ww) in enumerate(zip(heights, WIDTHS)):
            n = ((hh + sh - 1) // sh) * ((ww + sw - 1) // sw)
            img = y[off:off + n]
            off += n
            err = np.abs(sweep[2][i].astype(np.float64) - img.mean(axis=0))
            assert np.all(err <= (n + 2) * U * np.abs(img).mean(axis=0)), "%s: pooled mean of image %d off by %g" % (name, i, err.max())

    # (b) fp64 reference of the linear layer
    zero = np.zeros(cp, np.float32)
    lin = _run(dev, x, heights, c, cp, K, sh, sw, w, zero, NONE, None, pooled, 1)[0][:pout].astype(np.float64)
    ref, mag = _ref64(x, heights, c, cp, K, sh, sw, w)
    assert ref.shape == lin.shape
    err = np.abs(lin - ref)
    bound = U * (K * K + 2) * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s C=%d h=%s: worst err / bound %.3f" % (name, c, heights, worst))
    assert np.all(err <= bound), "%s: %d outputs outside the fp64 bound, worst err / bound %.3g" % (name, int((err > bound).sum()), worst)
