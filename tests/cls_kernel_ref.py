"""fp64 references, float32 stand-ins (torch on the CPU), mutants and the check function for the fp32 kernels that
rt_debug_cls_block, rt_debug_stem and rt_debug_glue32 drive: the classifier's MobileNetV3 blocks (k_cls_block and the launch
series it replaced), the three stems, and the plain squeeze-excite series with the small glue around it
(tests/test_gpu_cls_kernels.py on the GPU, tests/test_cls_kernel_checks_cpu.py here).  No device.

A Case holds the host arrays as its entry takes them and `compute(dtype, mut=None)`: the plain mathematics of the operation in
`dtype` arithmetic, one Out per returned buffer.  torch.float64 is the reference (and carries the element bounds), torch.float32
the stand-in of the rms rule and what the mutants are applied to.

Bounds.  U = 2^-24.  A K-term fp32 sum of products costs U (K + 8) S with S = sum |w| |x| + |b|; an activation passes errors
through its Lipschitz factor L (1 for ReLU and the clamps, 1.5 for hardswish); each epilogue rounding costs 4 U |y|.  Nothing is
fitted to what a kernel returned.
  block        e  = act(Wexp x + bexp)              de = L (U (cin + 8) S_e) + 4 U |e|
               d  = act(dw_kxk(e) + bdw)            dd = L (sum_taps |w| de + U (k k + 2) S_d) + 4 U |d|
               m  = mean_pixels(d)                  dm = mean(dd) + U (P + 4) mean|d|          (P = Ho W pixels)
               h  = relu(W1 m + b1)                 dh = sum |W1| dm + U (mid + 8) S_h
               s  = clamp(0.2 (W2 h + b2) + 0.5)    ds = 0.2 (sum |W2| dh + U (Cr + 8) S_s) + 4 U
               z  = d s  (or d without SE)          dz = dd s + |d| ds + U |z|
               y  = Wlin z + blin (+ x)             bound = sum |Wlin| dz + U (mid + 8) S_y + 4 U (|y| + |x| with the shortcut)
  se_scale     the m ... s part with dd = 0 (slope 0.2, or 1/6 on the LCNetV3 layer); `residual` adds 1 exactly (s in [0, 1]: the
               sum's rounding, U, is inside the 4 U).  Scaled in place: |x| ds + U |x s|.
  global_mean  U (P + 4) mean|x|.
  stems        U (27 + 8) S L + 4 U |y|  (L = 1.5 with hardswish, 1 without an activation).
  avgpool_3x2  U 8 mean|x| over the window's six pixels (five adds, the rounded 1/6, one multiply).
  exact        maxpool_2x2, argmax_rows (index and maximum) and the index of argmax_prob_rows: compared for equality, ties to
               the lowest index.  The U8 stem has its fp64 bound and, in the GPU test, must also equal the tensor-path output
               on the same floats bit for bit.
  softmax      p_c = exp(x_c - m) / sum_j exp(x_j - m).  Three parts, all relative errors:
                 (1) x_c - m is rounded once: an absolute U |x_c - m| in the exponent, a relative U |x_c - m| after exp;
                 (2) expf itself: E ulps = 2 E U relative.  E = 1 is a STATED constant, not a derived one: HIP's published
                     math-function table gives expf a maximum error of 1 ulp.  The ROCm installation ships no accuracy table;
                     /opt/rocm/lib/llvm/lib/clang/22/include/__clang_hip_math.h is where expf is defined (as __builtin_expf,
                     the full-precision device-library routine, not the __expf intrinsic) and this project's kernels are
                     compiled without fast-math flags that would replace it;
                 (3) the C-term sum of positive terms: (C - 1) U in any order, on top of the p-weighted mean of its terms'
                     own errors (1) + (2); the division (or the reciprocal of argmax_prob_rows) one more U.
               a_j = U (|x_j - m| + 2 E);   bound_c = p_c (a_c + sum_j p_j a_j + U (C + 2)).
Constants that are not derived: E above; the + 8 / + 4 / + 2 slack terms and the 4 U per epilogue are the suite's convention
(tests/test_gpu_rec_kernels.py), kept as the issue states them.

Unreachable, so without a case: the `C & 3 != 0` branch of FC1 in k_se_fc (every squeeze-excite layer of the three networks has a
channel count that is a multiple of 4: 8, 32, 40, 48, 88, 104, 200 in the classifier, 24, 96 in the det neck, 384 / 480 in the
LCNetV3 backbones).

No element of any returned buffer is left out: outside an Out's mask every word must still be RT_DEBUG_CANARY (the 64 spare rows,
the foreign half of avgpool's rows, softmax's spare rows), `zero` elements must be +0 (scales and scaled pixels past C)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EXP_ULPS = 1          # stated, see above
CANARY = 0x7FA5C3E1   # RT_DEBUG_CANARY (as a float32: a NaN)
ACT_NONE, ACT_RELU, ACT_HSWISH = 0, 1, 2
POOL_PIX = 128        # pixels per chunk of the first stage of the squeeze-excite mean (nn_kernels.hip)
GLUE_OPS = ["se_scale", "global_mean", "maxpool_2x2", "avgpool_3x2", "softmax_rows", "argmax_prob_rows", "argmax_rows"]
# ClsSpec of nets.h: k, mid, cout, se, act, sh
CLS_SPEC = [(3, 8, 8, True, ACT_RELU, 2), (3, 24, 8, False, ACT_RELU, 2), (3, 32, 8, False, ACT_RELU, 1),
            (5, 32, 16, True, ACT_HSWISH, 2), (5, 88, 16, True, ACT_HSWISH, 1), (5, 88, 16, True, ACT_HSWISH, 1),
            (5, 40, 16, True, ACT_HSWISH, 1), (5, 48, 16, True, ACT_HSWISH, 1), (5, 104, 32, True, ACT_HSWISH, 2),
            (5, 200, 32, True, ACT_HSWISH, 1), (5, 200, 32, True, ACT_HSWISH, 1)]
CLS_H_IN = [24, 12, 6, 6, 3, 3, 3, 3, 3, 2, 2]      # the blocks' input heights on a 48 x 192 crop (width 96 throughout)
CLS_CIN = [8, 8, 8, 8, 16, 16, 16, 16, 16, 32, 32]
SERIES, SWZ9, PAD9, PAD5 = (0, 0, 0), (1, 0, 9), (1, 1, 9), (1, 1, 5)   # info_out[:3]: fused, padded rows, MAXU
INSTANCE = {SERIES: "launch series", SWZ9: "swizzle, MAXU 9", PAD9: "padded rows, MAXU 9", PAD5: "padded rows, MAXU 5"}
STEM_IMAGES = [(48, 192), (48, 37), (1, 1), (2, 2), (5, 3), (15, 63), (16, 64), (17, 65), (18, 66), (33, 130)]
SE_IMAGES = [(1, 1), (1, 127), (8, 16), (3, 43), (12, 25)]     # 1, 127, 128, 129 and 300 pixels
DET_SCALE, DET_MEAN, DET_STD = 1.0 / 255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # distinct per channel: an index slip shows


def round_up(a, b):
    return (a + b - 1) // b * b


def chan_pitch(c):
    return round_up(c, 32) if c >= 128 else round_up(c, 4)


def cls_route(k, sh, cin, mid, cout, H, W):
    """nn::cls_block_supported and nn::cls_block_shape restated: (fused, padded rows, MAXU), and the three LDS terms"""
    ho = (H - 1) // sh + 1
    small = (8 * 16 + 2 * round_up(mid, 16) + 128 + (k * k + 1) * 16) * 4
    ok = (cin % 4 == 0 and cin <= 32 and cout % 4 == 0 and cout <= 32 and mid % 4 == 0 and mid <= 512 and W % 16 == 0 and
          (ho * W + 15) // 16 <= 72 and H * W * 64 + small <= 160 * 1024)
    padded, xs = H * (W + 2 * (k // 2)) * 80, H * W * (cin + 4) * 4
    if not ok:
        return SERIES, (padded, small, xs)
    pad = padded + small + xs <= 96 * 1024
    return (1, int(pad), 9 if (not pad or (ho * W + 15) // 16 > 40) else 5), (padded, small, xs)


def offsets(imgs):
    return [int(v) for v in np.concatenate([[0], np.cumsum([h * w for h, w in imgs])])]


def uni(rng, shape, scale=1.0):
    """uniform(-1, 1) float32 with full significands"""
    return (rng.uniform(-1, 1, shape) * scale).astype(np.float32)


def T(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def act_fn(t, act):
    if act == ACT_RELU:
        return torch.relu(t)
    if act == ACT_HSWISH:
        return t * torch.clamp(t + 3.0, 0.0, 6.0) / 6.0
    return t


def lip(act):
    return 1.5 if act == ACT_HSWISH else 1.0


class Out:
    """one returned buffer [(rows + 64)][ld]: mask = what the kernel must write, v its values (float64, or int64 for an index), bound
    the element bound, zero = elements that must be +0, base = the buffer before the launch where it is not the canary; kind =
    "arith" (bound and rms rule), "exact" (the float32 bits of v) or "index" (int32)"""

    def __init__(self, name, rows, ld, kind="arith"):
        self.name, self.kind = name, kind
        self.shape = (rows + 64, ld)
        self.mask = np.zeros(self.shape, bool)
        self.v = np.zeros(self.shape, np.int64 if kind == "index" else np.float64)
        self.bound = np.zeros(self.shape)
        self.zero = np.zeros(self.shape, bool)

    def fill(self, rows, cols, v, bound=None):
        """rows (a slice) x the first `cols` columns"""
        self.mask[rows, :cols] = True
        self.v[rows, :cols] = np.asarray(v).reshape(self.v[rows, :cols].shape)
        if bound is not None:
            self.bound[rows, :cols] = np.asarray(bound).reshape(self.v[rows, :cols].shape)
        return self


def N(t):
    return t.detach().to(torch.float64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


class Case:
    family = ""
    info = None

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return self.compute(torch.float64)

    def buffers(self, dtype=torch.float32, mut=None):
        """what a kernel computing in dtype would return: the words of each buffer (uint32), canary outside the masks"""
        res = []
        for o in self.compute(dtype, mut):
            b = np.full(o.shape, CANARY, np.uint32)
            with np.errstate(invalid="ignore", over="ignore"):
                w = o.v.astype(np.int32).view(np.uint32) if o.kind == "index" else o.v.astype(np.float32).view(np.uint32)
            b[o.mask] = w[o.mask]
            res.append(b)
        return res


def check(case, outs, f32=None):
    """asserts everything the suite asks of one launch's returned buffers, in this order: canary intact outside the output, pad
    elements +0, everything finite, err <= bound element-wise (or equality), rms error at most twice the float32 CPU form's;
    returns the measured figures"""
    refs = case.reference()
    if f32 is None:
        f32 = case.buffers(torch.float32)
    assert len(outs) == len(refs) == len(f32)
    fig = {"n": 0, "worst": 0.0, "worst32": 0.0}
    for o, got, s32 in zip(refs, outs, f32):
        bits = np.ascontiguousarray(got).view(np.uint32).reshape(o.shape)
        assert o.mask[:o.shape[0] - 64].any() and not o.mask[-64:].any()
        same = bits[~o.mask] == CANARY
        assert same.all(), "%s %s: %d elements outside the op's output were changed (first at flat index %d)" % (
            case.name, o.name, int((~same).sum()), int(np.flatnonzero(~o.mask)[np.argmin(same)]))
        assert (bits[o.zero] == 0).all(), "%s %s: %d pad elements are not +0" % (case.name, o.name, int((bits[o.zero] != 0).sum()))
        m = o.mask & ~o.zero
        fig["n"] += int(o.mask.sum())
        if o.kind == "index":
            g = bits.view(np.int32)[m].astype(np.int64)
            assert np.array_equal(g, o.v[m]), "%s %s: %d of %d indices differ" % (case.name, o.name, int((g != o.v[m]).sum()), g.size)
            continue
        with np.errstate(invalid="ignore"):   # (a canary left in the output is a signalling NaN)
            g = bits.view(np.float32)[m].astype(np.float64)
        r, b = o.v[m], o.bound[m]
        assert np.isfinite(g).all(), "%s %s: non-finite output" % (case.name, o.name)
        if o.kind == "exact":
            assert np.array_equal(g.astype(np.float32).view(np.uint32), r.astype(np.float32).view(np.uint32)), "%s %s: bits differ" % (case.name, o.name)
            continue
        assert g.size and (b > 0).all()
        err = np.abs(g - r)
        w = int(np.argmax(err / b))
        fig["worst"] = max(fig["worst"], float(err[w] / b[w]))
        assert (err <= b).all(), "%s %s: %d of %d elements outside the bound, worst err %.3e bound %.3e (ref %.6g got %.6g)" % (
            case.name, o.name, int((err > b).sum()), err.size, err[w], b[w], r[w], g[w])
        e32 = np.abs(np.ascontiguousarray(s32).view(np.float32).reshape(o.shape)[m].astype(np.float64) - r)
        rms, rms32 = float(np.sqrt(np.mean(err ** 2))), float(np.sqrt(np.mean(e32 ** 2)))
        fig["worst32"] = max(fig["worst32"], float(np.max(e32 / b)))
        fig["rms_" + o.name], fig["rms32_" + o.name] = rms, rms32
        fig["ratio_" + o.name] = rms / rms32 if rms32 else 0.0
        assert rms <= 2 * rms32, "%s %s: rms error %.3e is %.2f x the float32 CPU form's %.3e" % (case.name, o.name, rms, rms / max(rms32, 1e-300), rms32)
    return fig


# ----------------------------------------------------------------------------------------------------------------------------
# the classifier's block
def dwconv(x, w, b, sh):
    """x [n][H][W][C], w [C][k][k], b [C] or None -> [n][ceil(H / sh)][W][C]: zero-padded depthwise conv, stride (sh, 1)"""
    k = w.shape[-1]
    y = F.conv2d(x.permute(0, 3, 1, 2), w[:, None], b, stride=(sh, 1), padding=k // 2, groups=w.shape[0])
    return y.permute(0, 2, 3, 1)


def se_weights(rng, mean_abs, C, Cr, slope):
    """fc1 / fc2 scaled so that the hard-sigmoid's input spreads over about [-4, 4] / (5 slope): both clamps and the linear
    part occur (asserted by the callers on the reference)"""
    w1, b1 = uni(rng, (Cr, C), 4 / np.sqrt(C)), uni(rng, (Cr,))
    w2, b2 = uni(rng, (C, Cr)), uni(rng, (C,))
    h = np.maximum(mean_abs.astype(np.float64) @ w1.astype(np.float64).T + b1, 0)
    t = h @ w2.astype(np.float64).T + b2
    b2 = (b2 - (t.max() + t.min()) / 2).astype(np.float32)       # centred: the extremes reach both clamps
    f = np.float32(4.0 / (5 * slope) / ((t.max() - t.min()) / 2))
    return w1, b1, (w2 * f).astype(np.float32), (b2 * f).astype(np.float32)


class Block(Case):
    family = "block"

    def __init__(self, name, spec, cin, H, W, form, info, seed, n=3):
        self.name, self.form, self.info, self.n, self.H, self.W, self.cin = name, form, info, n, H, W, cin
        self.k, self.mid, self.cout, self.se, self.act, self.sh = spec
        self.Ho = (H - 1) // self.sh + 1
        self.shortcut = self.sh == 1 and cin == self.cout
        self.slope = 0.2
        rng = np.random.default_rng(seed)
        k, mid, cout = self.k, self.mid, self.cout
        self.x = uni(rng, (n, H, W, cin))
        self.x[1] *= np.float32(0.05)                     # crop 1 sits in hardswish's curved part
        self.exp_w, self.exp_b = uni(rng, (mid, cin), 4 / np.sqrt(cin)), uni(rng, (mid,))
        self.dw_w, self.dw_b = uni(rng, (mid, k, k), 4 / np.sqrt(k * k)), uni(rng, (mid,))
        self.lin_w, self.lin_b = uni(rng, (cout, mid), 4 / np.sqrt(mid)), uni(rng, (cout,))
        self.fc = None
        if self.se:
            with torch.no_grad():
                e = act_fn(T(self.x, torch.float64) @ T(self.exp_w, torch.float64).T + T(self.exp_b, torch.float64), self.act)
                d = act_fn(dwconv(e, T(self.dw_w, torch.float64), T(self.dw_b, torch.float64), self.sh), self.act)
            self.fc = se_weights(rng, d.mean((1, 2)).numpy(), mid, mid // 4, self.slope)

    def compute(self, dt, mut=None):
        c, k, sh, n = self, self.k, self.sh, self.n
        ref = dt == torch.float64
        x, We, be, Wd, bd, Wl, bl = (T(a, dt) for a in (c.x, c.exp_w, c.exp_b, c.dw_w, c.dw_b, c.lin_w, c.lin_b))
        if mut == "exp_bias_next_slice":
            be = torch.cat([be[16:], torch.zeros(16, dtype=dt)])
        if mut == "dw_tap_dropped":
            Wd = Wd.clone()
            Wd[:, k // 2, k // 2 + 1] = 0
        if mut == "dw_taps_transposed":
            Wd = Wd.transpose(1, 2).contiguous()
        e = act_fn(x @ We.T + be, c.act)
        d = act_fn(dwconv(e, Wd, bd, sh), c.act)
        if mut == "stride_in_w":
            d = d[:, :, (torch.arange(c.W) * sh) % c.W]
        P = c.Ho * c.W
        s = None
        if c.se:
            W1, b1, W2, b2 = (T(a, dt) for a in c.fc)
            m = d.sum((1, 2)) / ((c.H * c.W) if mut == "pool_div_hin" else P)
            h = torch.relu(m @ W1.T + b1)
            s = torch.clamp((1.0 / 6.0 if mut == "se_slope_sixth" else c.slope) * (h @ W2.T + b2) + 0.5, 0.0, 1.0)
            if mut == "se_scale_prev_crop":
                s = torch.roll(s, 1, 0)
            z = d * s[:, None, None, :]
        else:
            z = d
        y = z @ Wl.T + bl
        if c.shortcut and mut != "shortcut_missing":
            y = y + (2 * x if mut == "shortcut_twice" else x)
        if mut == "exp_pad_nonzero":   # channels mid .. npad_e hold what was in LDS (a NaN here) and meet the zero weights of the pack
            y = y + torch.tensor(float("nan"), dtype=dt) * 0
        o = Out("y", n * P, c.cout)
        o.fill(slice(0, n * P), c.cout, N(y))
        if mut == "last_tile_unwritten":
            for i in range(n):
                o.mask[(i + 1) * P - 16:(i + 1) * P] = False
        if ref:
            a = lambda t: t.abs()   # noqa: E731
            L = lip(c.act)
            de = L * U * (c.cin + 8) * (a(x) @ a(We).T + a(be)) + 4 * U * a(e)
            dd = L * (dwconv(de, a(Wd), None, sh) + U * (k * k + 2) * dwconv(a(e), a(Wd), a(bd), sh)) + 4 * U * a(d)
            if c.se:
                dm = dd.mean((1, 2)) + U * (P + 4) * a(d).mean((1, 2))
                dh = dm @ a(W1).T + U * (c.mid + 8) * (a(m) @ a(W1).T + a(b1))
                ds = c.slope * (dh @ a(W2).T + U * (c.mid // 4 + 8) * (a(h) @ a(W2).T + a(b2))) + 4 * U
                dz = dd * s[:, None, None, :] + a(d) * ds[:, None, None, :] + U * a(z)
                t = c.slope * (h @ W2.T + b2) + 0.5
                c.regions = (int((t <= 0).sum()), int(((t > 0) & (t < 1)).sum()), int((t >= 1).sum()))
                assert min(c.regions) > 0, "%s: the hard-sigmoid's regions %s" % (c.name, c.regions)
            else:
                dz = dd
            bound = dz @ a(Wl).T + U * (c.mid + 8) * (a(z) @ a(Wl).T + a(bl)) + 4 * U * (a(y) + (a(x) if c.shortcut else 0))
            o.bound[:n * P] = N(bound).reshape(n * P, c.cout)
        return [o]


# ----------------------------------------------------------------------------------------------------------------------------
# the stems
class Stem(Case):
    family = "stem"

    def __init__(self, name, cout, u8, seed):
        self.name, self.cout, self.u8 = name, cout, u8
        self.act = ACT_HSWISH if cout == 8 else ACT_NONE
        self.imgs = STEM_IMAGES
        rng = np.random.default_rng(seed)
        pix = offsets(self.imgs)[-1]
        self.w, self.b = uni(rng, (cout, 3, 3, 3), 4 / np.sqrt(27)), uni(rng, (cout,))
        if u8:
            self.rgb = rng.integers(0, 256, (pix, 3)).astype(np.uint8)
            self.rgb[:4] = [[0, 255, 0], [255, 0, 255], [0, 0, 0], [255, 255, 255]]
            self.x4 = self.normalised(self.rgb)
        else:
            self.x4 = uni(rng, (pix, 4))       # (channel 3 is never read)

    @staticmethod
    def normalised(rgb, bgr=True):
        """k_det_normalize's three separately rounded float32 operations; tensor channel c = page byte 2 - c"""
        src = rgb[:, ::-1] if bgr else rgb
        t = src.astype(np.float32) * np.float32(DET_SCALE)
        t = t - np.array(DET_MEAN, np.float32)
        t = t / np.array(DET_STD, np.float32)
        return np.concatenate([t, np.zeros((len(t), 1), np.float32)], 1).astype(np.float32)

    def compute(self, dt, mut=None):
        c = self
        ref = dt == torch.float64
        x4 = c.normalised(c.rgb, bgr=False) if mut == "u8_no_bgr" else c.x4
        w, b = T(c.w, dt), T(c.b, dt)
        offs = offsets(c.imgs)
        outs = [((h + 1) // 2, (ww + 1) // 2) for h, ww in c.imgs]
        oo = offsets(outs)
        o = Out("y", oo[-1], c.cout)
        L = lip(c.act)
        for i, (h, ww) in enumerate(c.imgs):
            x = T(x4[offs[i]:offs[i + 1], :3].reshape(1, h, ww, 3), dt).permute(0, 3, 1, 2)
            if mut == "col64_zero":          # column 64 of each 65-column patch: input column 64 tx + 63
                x = x.clone()
                x[..., 63::64] = 0
            if mut == "pad0":                # the patch starts at (2 oy, 2 ox): zero padding below and to the right only
                xp = F.pad(x, (0, 2, 0, 2))
                y = F.conv2d(xp, w, b, stride=2)[..., :outs[i][0], :outs[i][1]]
            else:
                y = F.conv2d(x, w, b, stride=2, padding=1)
            y = act_fn(y, c.act).permute(0, 2, 3, 1)[0]
            if mut == "tile_rows_swapped" and outs[i][0] >= 4:   # first tile: the rows of wave 0 and wave 1 exchanged
                y = y.clone()
                y[[0, 1, 2, 3]] = y[[2, 3, 0, 1]]
            bound = None
            if ref:
                S = F.conv2d(x.abs(), w.abs(), b.abs(), stride=2, padding=1).permute(0, 2, 3, 1)[0]
                bound = N(U * (27 + 8) * S * L + 4 * U * y.abs())
            o.fill(slice(oo[i], oo[i + 1]), c.cout, N(y), bound)
        return [o]


# ----------------------------------------------------------------------------------------------------------------------------
# squeeze-excite series and glue
class Glue(Case):
    family = "glue"
    ip, fp, w = (), (0.0,), None
    imgs = None


class SeScale(Glue):
    op = "se_scale"

    def __init__(self, name, C, slope, residual, apply, seed):
        self.name, self.C, self.Cp, self.Cr, self.slope, self.residual, self.apply = name, C, chan_pitch(C), C // 4, slope, residual, apply
        self.imgs = SE_IMAGES
        rng = np.random.default_rng(seed)
        pix = offsets(self.imgs)[-1]
        self.x = np.zeros((pix, self.Cp), np.float32)
        self.x[:, :C] = uni(rng, (pix, C)) + uni(rng, (1, C), 0.5)        # a mean per channel
        o = offsets(self.imgs)
        means = np.stack([self.x[o[i]:o[i + 1], :C].astype(np.float64).mean(0) for i in range(len(self.imgs))])
        self.w = se_weights(rng, means, C, self.Cr, slope)
        self.ip, self.fp = (C, self.Cr, residual, apply), (slope,)

    def compute(self, dt, mut=None):
        c, C, Cp = self, self.C, self.Cp
        ref = dt == torch.float64
        n, offs = len(c.imgs), offsets(c.imgs)
        x = T(c.x[:, :C], dt)
        W1, b1, W2, b2 = (T(a, dt) for a in c.w)
        rows = []
        for i in range(n):
            xi = x[offs[i]:offs[i + 1]]
            sm = xi.sum(0)
            if mut == "chunk_twice" and len(xi) == POOL_PIX + 1:
                sm = sm + xi[:POOL_PIX].sum(0)
            rows.append(sm / len(xi))
        m = torch.stack(rows)
        h = torch.relu(m @ W1.T + b1)
        if mut == "fc2_remainder_dropped" and c.Cr % 4:
            h = h.clone()
            h[:, c.Cr - c.Cr % 4:] = 0
        t = c.slope * (h @ W2.T + b2) + 0.5
        s = torch.clamp(t + 1.0, 0.0, 1.0) if (mut == "residual_before_clamp" and c.residual) else torch.clamp(t, 0.0, 1.0) + (1.0 if c.residual else 0.0)
        so = Out("scale", n, Cp)
        so.fill(slice(0, n), C, N(s))
        so.mask[:n] = True
        so.zero[:n, C:] = True
        P = torch.tensor([float(hh * ww) for hh, ww in c.imgs], dtype=dt)[:, None]
        outs = [so]
        if ref:
            a = lambda v: v.abs()   # noqa: E731
            am = torch.stack([a(x[offs[i]:offs[i + 1]]).mean(0) for i in range(n)])
            dm = U * (P + 4) * am
            dh = dm @ a(W1).T + U * (C + 8) * (a(m) @ a(W1).T + a(b1))
            ds = c.slope * (dh @ a(W2).T + U * (c.Cr + 8) * (a(h) @ a(W2).T + a(b2))) + 4 * U
            so.bound[:n, :C] = N(ds)
            c.regions = (int((t <= 0).sum()), int(((t > 0) & (t < 1)).sum()), int((t >= 1).sum()))
            assert min(c.regions) > 0, "%s: the hard-sigmoid's regions %s" % (c.name, c.regions)
        if c.apply:
            pix = offs[-1]
            xo = Out("x", pix, Cp)
            xo.mask[:pix] = True
            xo.zero[:pix, C:] = True
            for i in range(n):
                xi = x[offs[i]:offs[i + 1]]
                bound = N(xi.abs() * ds[i] + U * (xi * s[i]).abs()) if ref else None
                xo.fill(slice(offs[i], offs[i + 1]), C, N(xi * s[i]), bound)
            # (an element of x that is 0 would have a zero bound: none is, the operands are continuous)
            outs.append(xo)
        return outs


class GlobalMean(Glue):
    op = "global_mean"

    def __init__(self, name, C, seed):
        self.name, self.C, self.imgs, self.ip = name, C, SE_IMAGES, (C,)
        rng = np.random.default_rng(seed)
        self.x = uni(rng, (offsets(self.imgs)[-1], C)) + uni(rng, (1, C), 0.5)

    def compute(self, dt, mut=None):
        c, offs, n = self, offsets(self.imgs), len(self.imgs)
        x = T(c.x, dt)
        o = Out("mean", n, c.C)
        for i in range(n):
            xi = x[offs[i]:offs[i + 1]]
            sm = xi.sum(0)
            if mut == "chunk_twice" and len(xi) == POOL_PIX + 1:
                sm = sm + xi[:POOL_PIX].sum(0)
            o.fill(slice(i, i + 1), c.C, N(sm / len(xi)), N(U * (len(xi) + 4) * xi.abs().mean(0)))
        return [o]


class Pool(Glue):
    def __init__(self, name, op, C, imgs, ldy, seed):
        self.name, self.op, self.C, self.imgs, self.ldy = name, op, C, imgs, ldy
        self.kh, self.kw = (2, 2) if op == "maxpool_2x2" else (3, 2)
        self.ip = (C,) if op == "maxpool_2x2" else (C, ldy)
        self.x = uni(np.random.default_rng(seed), (offsets(imgs)[-1], C))

    def compute(self, dt, mut=None):
        c, offs, kh, kw = self, offsets(self.imgs), self.kh, self.kw
        outs = [(h // kh, w // kw) for h, w in c.imgs]
        oo = offsets(outs)
        o = Out("y", oo[-1], c.ldy, "exact" if c.op == "maxpool_2x2" else "arith")
        for i, (h, w) in enumerate(c.imgs):
            x = T(c.x[offs[i]:offs[i + 1]], dt)
            oh, ow = outs[i]
            taps = []
            for dy in range(kh):
                for dx in range(kw):
                    if mut == "maxpool_col_plus2" and dx == 1:     # column 2 ox + 2: the flat index as the kernel forms it
                        idx = ((torch.arange(oh)[:, None] * kh + dy) * w + torch.arange(ow)[None] * kw + 2) % (h * w)
                    else:
                        idx = (torch.arange(oh)[:, None] * kh + dy) * w + torch.arange(ow)[None] * kw + dx
                    taps.append(x[idx.reshape(-1)])
            st = torch.stack(taps)
            if c.op == "maxpool_2x2":
                o.fill(slice(oo[i], oo[i + 1]), c.C, N(st.max(0).values))
            else:
                o.fill(slice(oo[i], oo[i + 1]), c.C, N(st.sum(0) * (1.0 / 6.0)), N(U * 8 * st.abs().mean(0)))
        return [o]


class Softmax(Glue):
    def __init__(self, name, op, C, ld, seed):
        self.name, self.op, self.C, self.ld, self.ip = name, op, C, ld, (C, ld)
        rng = np.random.default_rng(seed)
        R = 8
        x = uni(rng, (R, C), 6.0)
        x[1, :] = x[1, 0]                                 # a row of equal values
        x[2, C - 1] = x[2].max() + np.float32(1.0)        # the maximum at the last index
        x[3, [C // 3, C - 1]] = x[3].max() + np.float32(0.5)   # an exact tie of two maxima (C = 2: the whole row)
        x[4] *= np.float32(4.0)                           # a wide row: most terms underflow towards 0
        x[5, 0] = x[5, C - 1] = x[5].max()                # a tie that includes an existing maximum
        if op == "argmax_rows":                           # rows that already hold probabilities
            e = np.exp(x.astype(np.float64) - x.max(1, keepdims=True))
            x = (e / e.sum(1, keepdims=True)).astype(np.float32)
            x[3, [C // 3, C - 1]] = x[3].max()
        self.x = np.full((R, ld), 100.0, np.float32)      # the pad columns must not be read
        self.x[:, :C] = x
        self.rows = R

    def compute(self, dt, mut=None):
        c, R, C = self, self.rows, self.C
        x = T(c.x[:, :C], dt)
        m = x.max(1, keepdim=True).values
        xn = c.x[:, :C]
        if mut == "tie_to_higher":
            idx = C - 1 - np.argmax(xn[:, ::-1], 1)
        else:
            idx = np.argmax(xn, 1)                        # the first maximum
        io = Out("idx", R, 1, "index").fill(slice(0, R), 1, idx)
        if c.op == "argmax_rows":
            return [Out("max", R, 1, "exact").fill(slice(0, R), 1, N(m)), io]
        e = torch.exp(x - m)
        p = e / e.sum(1, keepdim=True)
        a = U * ((x - m).abs() + 2 * EXP_ULPS)
        bound = p * (a + (p * a).sum(1, keepdim=True) + U * (C + 2))
        if c.op == "softmax_rows":
            return [Out("p", R, C).fill(slice(0, R), C, N(p), N(bound))]
        pm, bm = p.max(1).values, bound[torch.arange(R), torch.from_numpy(np.argmax(xn, 1))]
        return [Out("prob", R, 1).fill(slice(0, R), 1, N(pm), N(bm)), io]


# ----------------------------------------------------------------------------------------------------------------------------
def _block_cases():
    cs = {}
    for i, spec in enumerate(CLS_SPEC):
        for form in (0, 1):
            # (blocks 0 and 1, 24 x 96 and 12 x 96 inputs, pass the 96 KB switch and take the swizzled layout; the others padded rows, MAXU 5)
            inst = cls_route(spec[0], spec[5], CLS_CIN[i], spec[1], spec[2], CLS_H_IN[i], 96)[0] if form else SERIES
            cs["blk%d-f%d" % (i, form)] = lambda i=i, spec=spec, form=form, inst=inst: Block(
                "block %d %dx96 form %d" % (i, CLS_H_IN[i], form), spec, CLS_CIN[i], CLS_H_IN[i], 96, form, inst, 100 + i)
    S = CLS_SPEC
    edges = [  # id, spec row, cin, H, W, instance
        ("edge-w16", 3, 8, 6, 16, PAD5), ("edge-w32", 2, 8, 6, 32, PAD5), ("edge-h5-s2", 0, 8, 5, 32, PAD5),
        ("edge-h1-k5", 4, 16, 1, 32, PAD5), ("edge-h1-s2", 8, 16, 1, 16, PAD5),
        ("edge-40tiles-pad5", 6, 4, 5, 128, PAD5), ("edge-41tiles-pad9-k3", 2, 4, 41, 16, PAD9), ("edge-41tiles-pad9-k5se", 6, 4, 41, 16, PAD9),
        ("edge-41tiles-pad9-s2", 3, 4, 1, 656, PAD9),      # (the padded layout with MAXU 9 at stride 2 exists at H = 1 only)
        ("edge-72tiles-swz-k5se", 5, 16, 24, 48, SWZ9), ("edge-72tiles-swz-k3", 2, 8, 12, 96, SWZ9), ("edge-swz-k5-s2", 3, 8, 24, 96, SWZ9),
        ("edge-96k-below", 2, 8, 43, 16, PAD9), ("edge-96k-above", 2, 8, 44, 16, SWZ9),
        ("refused-w24", 2, 8, 6, 24, SERIES), ("refused-73tiles", 2, 8, 73, 16, SERIES), ("refused-cin36", 2, 36, 6, 32, SERIES),
        ("refused-mid520", (5, 520, 32, True, ACT_HSWISH, 1), 32, 2, 32, SERIES)]
    for j, (cid, row, cin, H, W, inst) in enumerate(edges):
        spec = S[row] if isinstance(row, int) else row
        cs[cid] = lambda cid=cid, spec=spec, cin=cin, H=H, W=W, inst=inst, j=j: Block(cid, spec, cin, H, W, 1, inst, 200 + j)
    return cs


def _stem_cases():
    return {"stem8": lambda: Stem("stem8 (k_stem<8>)", 8, False, 301), "stem16": lambda: Stem("stem16 (k_stem_mfma<0>)", 16, False, 302),
            "stem16-u8": lambda: Stem("stem16-u8 (k_stem_mfma<1>)", 16, True, 303)}


def _glue_cases():
    cs = {}
    for C, slope in ((8, 0.2), (48, 0.2), (88, 0.2), (200, 0.2), (480, float(np.float32(0.1666667)))):
        for res in (0, 1):
            for ap in (0, 1):
                cid = "se-c%d-r%d-a%d" % (C, res, ap)
                cs[cid] = lambda cid=cid, C=C, slope=slope, res=res, ap=ap: SeScale(cid, C, slope, res, ap, 400 + C + 2 * res + ap)
    cs["gmean-200"] = lambda: GlobalMean("gmean-200", 200, 500)
    cs["maxpool-200"] = lambda: Pool("maxpool-200", "maxpool_2x2", 200, [(2, 2), (3, 5), (4, 6), (7, 2), (2, 96)], 200, 501)
    cs["avgpool-120"] = lambda: Pool("avgpool-120", "avgpool_3x2", 120, [(3, 2), (3, 7), (3, 80)], 240, 502)
    for op in ("softmax_rows", "argmax_prob_rows", "argmax_rows"):
        for C, ld in ((2, 4), (257, 260), (6625, 6628)):
            cid = "%s-%d" % (op.replace("_rows", ""), C)
            cs[cid] = lambda cid=cid, op=op, C=C, ld=ld: Softmax(cid, op, C, ld, 600 + C)
    return cs


_MAKERS = {}
_MAKERS.update(_block_cases())
_MAKERS.update(_stem_cases())
_MAKERS.update(_glue_cases())
CASE_IDS = list(_MAKERS)
BLOCK_IDS = [i for i in CASE_IDS if i.startswith(("blk", "edge", "refused"))]
STEM_IDS = [i for i in CASE_IDS if i.startswith("stem")]
GLUE_IDS = [i for i in CASE_IDS if i not in BLOCK_IDS and i not in STEM_IDS]


@functools.lru_cache(maxsize=None)
def case(case_id):
    return _MAKERS[case_id]()


# mutant -> the cases it is tried on (at least one must refuse it)
MUTANTS = {
    "dw_tap_dropped": ["blk2-f1", "blk4-f1"], "dw_taps_transposed": ["blk2-f1", "blk4-f1"], "stride_in_w": ["blk1-f1", "blk3-f1"],
    "pool_div_hin": ["blk3-f1", "blk0-f1"], "se_scale_prev_crop": ["blk4-f1", "blk0-f1"], "se_slope_sixth": ["blk4-f1", "blk6-f1"],
    "shortcut_missing": ["blk2-f1", "blk5-f1"], "shortcut_twice": ["blk2-f1", "blk5-f1"], "exp_bias_next_slice": ["blk2-f1", "blk4-f1"],
    "last_tile_unwritten": ["blk2-f1", "edge-41tiles-pad9-k3"], "exp_pad_nonzero": ["blk0-f1", "blk6-f1"],
    "pad0": ["stem8", "stem16"], "u8_no_bgr": ["stem16-u8"], "col64_zero": ["stem16", "stem16-u8"], "tile_rows_swapped": ["stem16"],
    "chunk_twice": ["se-c48-r0-a0", "gmean-200"], "fc2_remainder_dropped": ["se-c88-r0-a0", "se-c8-r1-a1"],
    "residual_before_clamp": ["se-c48-r1-a0", "se-c200-r1-a1"], "maxpool_col_plus2": ["maxpool-200"],
    "tie_to_higher": ["argmax-257", "argmax_prob-6625", "argmax-2"],
}
