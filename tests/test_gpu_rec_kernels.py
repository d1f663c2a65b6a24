"""Kernel-level numerics of three families on the recognition net's hot path, one launch at a time against fp64 references
computed with numpy on the host: the fused thin LCNetV3 blocks (rt_debug_lc_block: k_lc_lds, k_lc_wave, k_lc_thin, the unfused
pair), the SVTR neck's 1x3 token convs (rt_debug_conv13: k_conv13_flat, k_conv_sp<1, 3>) and k_add_layernorm
(rt_debug_layernorm).  Operands are uniform(-1, 1) float32 with full 24-bit significands, pointwise / conv weights scaled by
4 / sqrt(K), every bias random per channel, the two LAB pairs different from each other and from (1, 0).  U = 2^-24.  Every
launch writes into a buffer filled with a canary, with 64 rows past the last one.  Besides its element bound every kernel's
rms error must stay within twice that of the same operation in float32 by torch on the CPU.

(a) Thin blocks: the seven blocks of the two LCNetV3 backbones with the depthwise tails the nets give them, each with and
without the pointwise LAB, on one ragged batch of six images (49 / 28 tiles in the largest: several workgroups, a partial
last wave; a single pixel; an image narrower than a tile; odd and even stride-2 inputs).  The route that ran is asserted,
forms 1 and 3 equal form 0 bit for bit, and form 3 is within

    s = b_dw + sum_taps w x             S1 = |b_dw| + sum |w| |x|
    a = lab1(hswish(s))  (or s)         L1 = 1.5 |dw_a|  (or 1)
    da = U (9 + 2) S1 L1 + 4 U |a|      (second term only with a tail)
    S2 = sum_k |Wp_k| |a_k| + |b_pw|    L2 = 1.5 |pw_a|
    bound = L2 (sum_k |Wp_k| da_k + U (K + 8) S2) + 4 U |y|

of the fp64 block: the two stage bounds the suite already uses, composed.  da is the depthwise stage's (the 9-tap fp32 sum
in any order, through an activation of Lipschitz factor L1, plus the roundings of the tail itself); the pointwise stage sees
inputs off by da (first term, through |Wp|), adds the error of its own K-term sum and passes both through hardswish + LAB
(L2); 4 U |y| covers the roundings of that last epilogue.  A dropped or swapped tap moves an output by ~10^3 bounds.
Measured on an MI355X, worst err / bound over the batch (k_lc_lds; torch float32 on the CPU in brackets): 16->32 0.039 (0.043),
32->64 0.031 (0.028), 48->48 0.023 (0.025), 64->64 0.020 (0.018), 32->48 /2 0.041 (0.043), 48->96 /2 0.035 (0.038), 64->128
/(2, 1) 0.024 (0.020); rms error 1.00-1.05 x torch's.  Without the pointwise LAB the barrier-free kernels were one bit off form 0
(+0 for the -0 hardswish gives below -3: their LAB fma ran with a = 1, c = 0); lc_plan() leaves such a block to
k_lc_thin / the unfused pair, and the routes asserted here say so.

(b) 1x3 token convs, N = 60 with swish, cin = 480 (inside rows of pitch 960 whose upper half holds noise) and 960: form 1
(k_conv13_flat over the flat token list with RecNet's line flags) equals form 0 (k_conv_sp on one image per line) bit for bit
and is within U (3 cin + 8) S L + 4 U R of an fp64 zero-padded conv per line -- the bound of tests/test_gpu_ops.py for a sum of
3 cin terms: S = sum |w| |x| + |bias|, L = 1.1 (swish), R = |output|.  The line lists hold lines of 1 and 2 tokens, a line that
ends on token 127, one that straddles a 128-token tile edge and one longer than a tile, at totals of 1, 127 and 0 modulo 128;
two larger lists make conv13_flat() pick 2 and 4 column tiles per workgroup (its rule, asserted on the CU count it reports).
Both kernels close a partial sum every two 32-channel slabs (192 products) and add it to a running total: in one fp32
accumulator chain of 1440 / 2880 terms the rms error was 2.8 x / 3.8 x torch's (6.2e-7 ... 6.6e-7 and 8.8e-7 ... 8.9e-7 against
2.2e-7 ... 2.4e-7), which this file's rms check refused.  Measured on an MI355X (256 CUs: NT 1 on the small lists, 2 and 4 on the
large ones): worst err / bound 0.001 or below in all eight cases (torch float32: the same), rms error 2.2e-7 ... 2.4e-7,
0.99 - 1.00 x torch's.

(c) k_add_layernorm, C = 120, 1 / 5 / 4099 rows, with and without the residual, eps 1e-5 / 1e-6, on unit-normal rows, rows
of 50 + 0.05 N(0, 1) (a one-pass E[x^2] - mean^2 variance loses them) and rows of mixed offset and spread.  With v = x + r,
d = v - mean, s' = sqrt(var + eps):

    E = U ((C + 4) mean|v| + 2 |v|)
    rel = max_row(E) / s' + (C + 8) U
    bound = |g| / s' (E + |d| rel) + 4 U (|y| + |beta|)

E bounds the error of d (the rounding of x + r, the C-term sum behind the mean, the subtraction), rel the relative error of
1 / s' that follows from it (the variance is a C-term sum of squares of values off by at most max E) and the last term the
two roundings of the affine.  Rows of one repeated value must give beta exactly.  The kernel takes the mean of the centred values out of them again
(corrected two-pass): with the plain two-pass form a row of mean 10 and spread 1 carried the rounding of its mean, 3.3e-7 rms
against torch's 4.5e-8 on the single mixed row, which the rms check refused.  Measured on an MI355X: worst err / bound 0.073
(unit normal), 0.006 (offset), 0.070 (mixed); rms error at most 1.85 x torch's over the 36 (case, population) pairs, and 0.03 x
on the 4099 mixed rows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NONE, HSWISH, SWISH = 0, 2, 3
CANARY = 0x7FA5C3E1   # RT_DEBUG_CANARY
U = 2.0 ** -24
DW_LAB, PW_LAB = (1.3, 0.07), (0.8, -0.05)
UNFUSED, THIN, WAVE, LDS = 0, 1, 2, 3   # nn::LcRoute
ROUTE = {UNFUSED: "unfused pair", THIN: "k_lc_thin", WAVE: "k_lc_wave", LDS: "k_lc_lds"}


@pytest.fixture(scope="module")
def dev(hip_session):
    return hip_session._hd.lib, hip_session._hd.h


def _pitch(c):
    return (c + 31) // 32 * 32 if c >= 128 else (c + 3) // 4 * 4


def _hswish(v):
    return v * np.clip(v + 3.0, 0.0, 6.0) / 6.0


def _hswish32(v):
    return v * torch.clamp(v + 3.0, 0.0, 6.0) / 6.0


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


# ------------------------------------------------------------------------------------------------------------------------------
# (a) fused thin LCNetV3 blocks
BLOCKS = [(16, 32, 1, 1), (32, 64, 1, 1), (48, 48, 1, 1), (64, 64, 1, 1), (32, 48, 2, 2), (48, 96, 2, 2), (64, 128, 2, 1)]
IMAGES = [(26, 100), (13, 37), (1, 1), (5, 16), (24, 17), (7, 2)]


def _lc_run(dev, d, pw_lab, form):
    lib, h = dev
    cin, cout, sh, sw = d["block"]
    hs = np.array([a for a, _ in IMAGES], np.int32)
    ws = np.array([b for _, b in IMAGES], np.int32)
    out = np.empty((d["pout"] + 64, _pitch(cout)), np.float32)
    info = (C.c_int * 1)(-1)
    dw_lab = DW_LAB if d["tail"] else None
    rc = lib.rt_debug_lc_block(h, d["x"].ctypes.data, hs.ctypes.data, ws.ctypes.data, len(IMAGES), cin, cout, sh, sw,
                               d["dw_w"].ctypes.data, d["dw_b"].ctypes.data, d["pw_w"].ctypes.data, d["pw_b"].ctypes.data,
                               HSWISH if d["tail"] else NONE, 1 if dw_lab else 0, DW_LAB[0], DW_LAB[1],
                               1 if pw_lab else 0, PW_LAB[0], PW_LAB[1], form, out.ctypes.data, info)
    assert rc == 0, lib.rt_last_error(h)
    return out, info[0]


@functools.lru_cache(maxsize=None)
def _lc_data(cin, cout, sh, sw):
    """Operands of a block and everything of its references that does not depend on the pointwise LAB (computed once per block)."""
    rng = np.random.default_rng(1000 * cin + 10 * cout + 3 * sh + sw)
    tail = not (sh == 2 and sw == 2)   # LearnableRepLayer: hardswish + LAB, skipped at stride 2
    npix = sum(a * b for a, b in IMAGES)
    x = rng.uniform(-1, 1, (npix, cin)).astype(np.float32)
    dw_w = rng.uniform(-1, 1, (cin, 3, 3)).astype(np.float32)
    dw_b = rng.uniform(-1, 1, cin).astype(np.float32)
    pw_w = (rng.uniform(-1, 1, (cout, cin)) * (4.0 / np.sqrt(cin))).astype(np.float32)
    pw_b = rng.uniform(-1, 1, cout).astype(np.float32)
    w64, b64 = dw_w.astype(np.float64), dw_b.astype(np.float64)
    a_l, da_l, a32_l = [], [], []
    off = 0
    for hh, ww in IMAGES:
        img = x[off:off + hh * ww].reshape(hh, ww, cin)
        off += hh * ww
        ho, wo = (hh + sh - 1) // sh, (ww + sw - 1) // sw
        pad = np.zeros((hh + 2 + sh, ww + 2 + sw, cin))
        pad[1:1 + hh, 1:1 + ww] = img
        s = np.zeros((ho, wo, cin)) + b64
        S1 = np.zeros((ho, wo, cin)) + np.abs(b64)
        for dy in range(3):
            for dx in range(3):
                v = pad[dy:dy + (ho - 1) * sh + 1:sh, dx:dx + (wo - 1) * sw + 1:sw]
                s += v * w64[:, dy, dx]
                S1 += np.abs(v) * np.abs(w64[:, dy, dx])
        if tail:
            a = _hswish(s) * DW_LAB[0] + DW_LAB[1]
            da = U * (9 + 2) * S1 * 1.5 * abs(DW_LAB[0]) + 4 * U * np.abs(a)
        else:
            a, da = s, U * (9 + 2) * S1
        a_l.append(a.reshape(-1, cin))
        da_l.append(da.reshape(-1, cin))
        # the same stage in float32 on the CPU
        t = F.conv2d(torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))[None], torch.from_numpy(dw_w)[:, None],
                     torch.from_numpy(dw_b), stride=(sh, sw), padding=1, groups=cin)[0]
        assert tuple(t.shape) == (cin, ho, wo)
        if tail:
            t = _hswish32(t) * DW_LAB[0] + DW_LAB[1]
        a32_l.append(t.permute(1, 2, 0).reshape(-1, cin))
    a, da, a32 = np.concatenate(a_l), np.concatenate(da_l), torch.cat(a32_l)
    wp64 = pw_w.astype(np.float64).T
    return {"block": (cin, cout, sh, sw), "tail": tail, "x": x, "dw_w": dw_w, "dw_b": dw_b, "pw_w": pw_w, "pw_b": pw_b,
            "pout": a.shape[0],
            "pre": a @ wp64 + pw_b.astype(np.float64),
            "S2": np.abs(a) @ np.abs(wp64) + np.abs(pw_b.astype(np.float64)),
            "dpre": da @ np.abs(wp64),
            "pre32": a32 @ torch.from_numpy(pw_w).T + torch.from_numpy(pw_b)}


@pytest.mark.parametrize("pw_lab", [1, 0], ids=["lab", "nolab"])
@pytest.mark.parametrize("cin,cout,sh,sw", BLOCKS, ids=["%d-%d-s%d%d" % b for b in BLOCKS])
def test_thin_block_forms_against_fp64(dev, cin, cout, sh, sw, pw_lab):
    d = _lc_data(cin, cout, sh, sw)
    pout, ldy = d["pout"], _pitch(cout)
    assert ldy == cout
    name = "%d->%d /(%d, %d)%s" % (cin, cout, sh, sw, "" if pw_lab else " without the pointwise LAB")
    stride1 = sh == 1 and sw == 1
    f0, r0 = _lc_run(dev, d, pw_lab, 0)
    f3, r3 = _lc_run(dev, d, pw_lab, 3)
    again, _ = _lc_run(dev, d, pw_lab, 3)
    # 1. the routes (the barrier-free kernels always apply a pointwise LAB: a block without one stays on form 0's kernels)
    assert r0 == (UNFUSED if (sh, sw) == (2, 1) else THIN), "%s: form 0 ran %s" % (name, ROUTE.get(r0, r0))
    assert r3 == (LDS if pw_lab else r0), "%s: form 3 ran %s" % (name, ROUTE.get(r3, r3))
    # 2. bit for bit over the whole buffer
    if stride1:
        f1, r1 = _lc_run(dev, d, pw_lab, 1)
        assert r1 == (WAVE if pw_lab else r0), "%s: form 1 ran %s" % (name, ROUTE.get(r1, r1))
        assert np.array_equal(f1.view(np.uint32), f0.view(np.uint32)), "%s: k_lc_wave differs from form 0" % name
    assert np.array_equal(f3.view(np.uint32), f0.view(np.uint32)), "%s: form 3 (%s) differs from form 0 (%s)" % (name, ROUTE[r3], ROUTE[r0])
    assert np.array_equal(f3.view(np.uint32), again.view(np.uint32)), "%s: two runs of form 3 differ" % name
    # 3. canary rows, finite outputs
    assert (f3[pout:].view(np.uint32) == CANARY).all(), "%s: wrote past the last image" % name
    assert np.isfinite(f3[:pout]).all(), name
    # 4. element bound against the fp64 block
    pa, pc = PW_LAB if pw_lab else (1.0, 0.0)
    ref = _hswish(d["pre"]) * pa + pc
    bound = 1.5 * abs(pa) * (d["dpre"] + U * (cin + 8) * d["S2"]) + 4 * U * np.abs(ref)
    err = np.abs(f3[:pout].astype(np.float64) - ref)
    ratio = err / bound
    worst = float(ratio.max())
    # 5. rms against float32 on the CPU
    cpu = (_hswish32(d["pre32"]) * pa + pc).numpy().astype(np.float64)
    rms, rms_cpu, cpu_worst = _rms(err), _rms(cpu - ref), float((np.abs(cpu - ref) / bound).max())
    # 6.
    print("%s: worst err / bound %.3f (torch float32: %.3f), rms err %.3g (torch float32: %.3g)" % (name, worst, cpu_worst, rms, rms_cpu))
    if worst > 1.0:
        p, c = np.unravel_index(int(ratio.argmax()), ratio.shape)
        starts = np.cumsum([0] + [((a + sh - 1) // sh) * ((b + sw - 1) // sw) for a, b in IMAGES])
        img = int(np.searchsorted(starts, p, side="right") - 1)
        wo = (IMAGES[img][1] + sw - 1) // sw
        pytest.fail("%s: %d outputs outside the fp64 bound, worst err / bound %.3g at image %d pixel (%d, %d) channel %d (got %r ref %r)" % (
            name, int((ratio > 1).sum()), worst, img, (p - starts[img]) // wo, (p - starts[img]) % wo, c, f3[p, c], ref[p, c]))
    assert rms <= 2 * rms_cpu, "%s: rms err %.3g, torch float32 %.3g" % (name, rms, rms_cpu)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) 1x3 token convs
C13_N = 60
_HEAD = [1, 2, 50, 75, 100, 60, 130, 1, 2]   # 75 ends on token 127, 60 crosses token 256, 130 (two tiles of k_conv_sp) crosses 384; 421 tokens
SMALL_LISTS = {513: _HEAD + [40, 51, 1], 511: _HEAD + [60, 28, 2], 512: _HEAD + [89, 2]}
NT_SEEN = set()


def _large_list(total):
    rng = np.random.default_rng(total)
    lines = list(_HEAD)
    left = total - sum(lines)
    while left > 0:
        t = int(min(left, rng.integers(1, 101)))
        lines.append(t)
        left -= t
    return lines


def _check_list(lines, total):
    """The properties every line list of this file must have."""
    ends = np.cumsum(lines)
    starts = ends - np.asarray(lines)
    assert ends[-1] == total
    assert 1 in lines and 2 in lines and max(lines) > 128
    assert 128 in ends and 128 in starts                                                  # a line ends on token 127, the next starts on 128
    assert any(s // 128 != (e - 1) // 128 and t <= 128 for s, e, t in zip(starts, ends, lines))   # a line (no longer than a tile) across a tile edge


def _flags(lines):
    f = np.zeros(int(np.sum(lines)), np.uint8)
    ends = np.cumsum(lines)
    f[ends - np.asarray(lines)] |= 1
    f[ends - 1] |= 2
    return f


def _c13_run(dev, x, lines, cin, w, bias, form):
    lib, h = dev
    rows, ldx = x.shape
    toks = np.asarray(lines, np.int32)
    out = np.empty((rows + 64, _pitch(C13_N)), np.float32)
    info = (C.c_int * 2)(-1, -1)
    rc = lib.rt_debug_conv13(h, x.ctypes.data, rows, ldx, toks.ctypes.data, len(lines), cin, w.ctypes.data, C13_N, bias.ctypes.data,
                             SWISH, form, out.ctypes.data, info)
    assert rc == 0, lib.rt_last_error(h)
    return out, tuple(info)


def _nt_rule(rows, cus):
    """conv13_flat(): 4 column tiles of 16 channels per workgroup, halved until there is a workgroup per CU."""
    tiles, nt = (rows + 127) // 128, 4
    while nt > 1 and tiles * ((4 + nt - 1) // nt) < cus:
        nt = (nt + 1) // 2
    return nt


def _c13_check(dev, name, total, lines, cin, ldx, expect_nt=None):
    _check_list(lines, total)
    rng = np.random.default_rng(7 * total + cin + ldx)
    x = rng.uniform(-1, 1, (total, ldx)).astype(np.float32)   # (cin < ldx: the channels past cin are noise the conv must not read)
    K = 3 * cin
    w = (rng.uniform(-1, 1, (C13_N, cin, 1, 3)) * (4.0 / np.sqrt(K))).astype(np.float32)
    bias = rng.uniform(-1, 1, C13_N).astype(np.float32)
    sp, info0 = _c13_run(dev, x, lines, cin, w, bias, 0)
    flat, info1 = _c13_run(dev, x, lines, cin, w, bias, 1)
    # the column tiles per workgroup, by conv13_flat()'s rule on the CU count it used
    assert info0[0] == 0 and info1[1] > 0
    assert info1[0] == _nt_rule(total, info1[1]), "%s: NT %d on %d CUs" % (name, info1[0], info1[1])
    if expect_nt is not None and info1[1] == 256:
        assert info1[0] == expect_nt, "%s: NT %d, expected %d on 256 CUs" % (name, info1[0], expect_nt)
    NT_SEEN.add(info1[0])
    # 1. / 2. bit for bit, canary rows intact
    assert np.array_equal(flat.view(np.uint32), sp.view(np.uint32)), "%s: k_conv13_flat differs from k_conv_sp" % name
    assert (flat[total:].view(np.uint32) == CANARY).all(), "%s: wrote past the last token" % name
    # rows to compare: all, or the first and the last two tiles plus every 61st row
    if total <= 20000:
        rows = np.arange(total)
    else:
        last = ((total + 127) // 128 - 2) * 128
        rows = np.unique(np.concatenate([np.arange(256), np.arange(last, total), np.arange(0, total, 61)]))
        assert len(rows) >= 0.02 * total
        f = _flags(lines)
        in_tiles = np.concatenate([np.arange(256), np.arange(last, total)])
        assert np.isin(in_tiles[f[in_tiles] != 0], rows).all()
    # fp64: a zero-padded conv per line -- the neighbours of a token inside its own line, zeros beyond its ends
    left, right = np.full(total, -1), np.full(total, -1)
    o = 0
    for t in lines:
        left[o + 1:o + t] = np.arange(o, o + t - 1)
        right[o:o + t - 1] = np.arange(o + 1, o + t)
        o += t
    x32 = np.concatenate([x[:, :cin], np.zeros((1, cin), np.float32)])   # (index -1: the zero row)
    a32 = np.concatenate([x32[left[rows]], x32[rows], x32[right[rows]]], axis=1)
    w2 = np.ascontiguousarray(w[:, :, 0, :].transpose(2, 1, 0).reshape(K, C13_N))   # [tap][cin] x [cout]
    a64, w64, b64 = a32.astype(np.float64), w2.astype(np.float64), bias.astype(np.float64)
    acc = a64 @ w64 + b64
    S = np.abs(a64) @ np.abs(w64) + np.abs(b64)
    ref = acc / (1.0 + np.exp(-acc))
    bound = U * (K + 8) * S * 1.1 + 4 * U * np.abs(ref)
    got = flat[rows, :C13_N].astype(np.float64)
    assert np.isfinite(got).all(), name
    err = np.abs(got - ref)
    ratio = err / bound
    worst = float(ratio.max())
    t = torch.from_numpy(a32) @ torch.from_numpy(w2) + torch.from_numpy(bias)
    cpu = (t * torch.sigmoid(t)).numpy().astype(np.float64)
    rms, rms_cpu = _rms(err), _rms(cpu - ref)
    print("%s: NT %d on %d CUs, worst err / bound %.3f (torch float32: %.3f), rms err %.3g (torch float32: %.3g)" % (
        name, info1[0], info1[1], worst, float((np.abs(cpu - ref) / bound).max()), rms, rms_cpu))
    if worst > 1.0:
        i, c = np.unravel_index(int(ratio.argmax()), ratio.shape)
        pytest.fail("%s: %d outputs outside the fp64 bound, worst err / bound %.3g at token %d (flags %d) channel %d (got %r ref %r)" % (
            name, int((ratio > 1).sum()), worst, rows[i], _flags(lines)[rows[i]], c, got[i, c], ref[i, c]))
    assert rms <= 2 * rms_cpu, "%s: rms err %.3g, torch float32 %.3g" % (name, rms, rms_cpu)


@pytest.mark.parametrize("total", sorted(SMALL_LISTS))
@pytest.mark.parametrize("cin,ldx", [(480, 960), (960, 960)])
def test_token_conv_forms_against_fp64(dev, cin, ldx, total):
    _c13_check(dev, "conv1x3 %d -> 60 (pitch %d), %d tokens" % (cin, ldx, total), total, SMALL_LISTS[total], cin, ldx, expect_nt=1)


# 129 tiles of 128 tokens (>= 128: two column tiles per workgroup on 256 CUs) and 256 tiles (> 255: four)
@pytest.mark.parametrize("total,nt", [(128 * 128 + 1, 2), (255 * 128 + 1, 4)])
def test_token_conv_column_tiles_per_workgroup(dev, total, nt):
    _c13_check(dev, "conv1x3 480 -> 60, %d tokens" % total, total, _large_list(total), 480, 480, expect_nt=nt)


def test_token_conv_every_instance_ran():
    """k_conv13_flat<1>, <2> and <4> (the tests above, on the 256 CUs of an MI355X)."""
    assert NT_SEEN == {1, 2, 4}, "column tiles per workgroup that ran: %s" % sorted(NT_SEEN)


# ------------------------------------------------------------------------------------------------------------------------------
# (c) add + layernorm
LN_C = 120


def _ln_run(dev, x, r, g, beta, eps):
    lib, h = dev
    rows = x.shape[0]
    out = np.empty((rows + 64, LN_C), np.float32)
    rc = lib.rt_debug_layernorm(h, x.ctypes.data, None if r is None else r.ctypes.data, rows, LN_C, g.ctypes.data, beta.ctypes.data,
                                eps, out.ctypes.data)
    assert rc == 0, lib.rt_last_error(h)
    assert (out[rows:].view(np.uint32) == CANARY).all(), "wrote past the last row"
    return out[:rows]


def _ln_rows(kind, rows, rng):
    n = rng.standard_normal((rows, LN_C))
    if kind == "normal":
        return n
    if kind == "offset":
        return 50.0 + 0.05 * n
    return rng.uniform(-10, 10, (rows, 1)) + rng.uniform(0.01, 3.0, (rows, 1)) * n   # mixed


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("residual", [0, 1], ids=["x", "x+r"])
@pytest.mark.parametrize("rows", [1, 5, 4099])
def test_add_layernorm_against_fp64(dev, rows, residual, eps):
    rng = np.random.default_rng(100 * rows + 10 * residual + (1 if eps < 5e-6 else 0))
    g = rng.uniform(-1.5, 1.5, LN_C).astype(np.float32)
    beta = rng.uniform(-1, 1, LN_C).astype(np.float32)
    g64, b64 = g.astype(np.float64), beta.astype(np.float64)
    for kind in ("normal", "offset", "mixed"):
        v0 = _ln_rows(kind, rows, rng)
        if residual:   # x + r has the population's statistics
            r = rng.uniform(-1, 1, (rows, LN_C)).astype(np.float32)
            x = (v0 - r).astype(np.float32)
        else:
            r, x = None, v0.astype(np.float32)
        got = _ln_run(dev, x, r, g, beta, eps).astype(np.float64)
        assert np.isfinite(got).all()
        v = x.astype(np.float64) + (0.0 if r is None else r.astype(np.float64))
        mean = v.mean(axis=1, keepdims=True)
        d = v - mean
        sd = np.sqrt((d * d).mean(axis=1, keepdims=True) + eps)
        ref = d / sd * g64 + b64
        E = U * ((LN_C + 4) * np.abs(v).mean(axis=1, keepdims=True) + 2 * np.abs(v))
        rel = E.max(axis=1, keepdims=True) / sd + (LN_C + 8) * U
        bound = np.abs(g64) / sd * (E + np.abs(d) * rel) + 4 * U * (np.abs(ref) + np.abs(b64))
        err = np.abs(got - ref)
        worst = float((err / bound).max())
        v32 = torch.from_numpy(x) if r is None else torch.from_numpy(x) + torch.from_numpy(r)
        cpu = F.layer_norm(v32, (LN_C,), torch.from_numpy(g), torch.from_numpy(beta), eps).numpy().astype(np.float64)
        rms, rms_cpu = _rms(err), _rms(cpu - ref)
        print("layernorm %d rows%s eps %g, %s: worst err / bound %.3f (torch float32: %.3f), rms err %.3g (torch float32: %.3g)" % (
            rows, " + r" if residual else "", eps, kind, worst, float((np.abs(cpu - ref) / bound).max()), rms, rms_cpu))
        if worst > 1.0:
            i, c = np.unravel_index(int((err / bound).argmax()), err.shape)
            pytest.fail("%s rows: err / bound %.3g at row %d channel %d (got %r ref %r)" % (kind, worst, i, c, got[i, c], ref[i, c]))
        assert rms <= 2 * rms_cpu, "%s rows: rms err %.3g, torch float32 %.3g" % (kind, rms, rms_cpu)


@pytest.mark.parametrize("residual", [0, 1], ids=["x", "x+r"])
def test_add_layernorm_of_constant_rows_is_beta(dev, residual):
    """Values of at most 8 significant bits: every partial sum of the 120 (7 more bits) is exact in any order, so the mean is the
    value itself, the centred row and the variance are zero, and the output is beta whatever 1 / sqrt(eps) is."""
    rng = np.random.default_rng(5)
    vals = np.array([0.0, 1.0, -3.0, 50.0, -0.625, 96.0, 2.0 ** -20, -1000.0], np.float32)
    g = rng.uniform(-1.5, 1.5, LN_C).astype(np.float32)
    beta = rng.uniform(-1, 1, LN_C).astype(np.float32)
    x = np.repeat(vals[:, None], LN_C, axis=1)
    r = None
    if residual:   # x + r exact: r = the value again (2 v has the same significand)
        r = x.copy()
    for eps in (1e-5, 1e-6):
        got = _ln_run(dev, x, r, g, beta, eps)
        assert np.isfinite(got).all()
        assert np.array_equal(got.view(np.uint32), np.repeat(beta[None], len(vals), axis=0).view(np.uint32)), "eps %g" % eps
