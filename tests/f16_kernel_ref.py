"""fp64 references, float32 stand-ins, numpy mutants and the check functions for the fp16 glue kernels that rt_debug_glue16
drives (tests/test_gpu_f16_kernels.py on the GPU, tests/test_f16_kernel_checks_cpu.py here).  Plain numpy, no device.

A Case holds the host arrays exactly as rt_debug_glue16 takes them (whole buffers, float32, every fp16 operand already rounded
to fp16) and `compute(dtype, mut)`: the operation on those buffers in `dtype` arithmetic, returning (mask, values) over the whole
output buffer [(rows + 64)][pitch] -- mask = the elements the kernel must write.  dtype = float64 is the reference, float32
rounded once to the output type is the stand-in a right kernel is expected to match in accuracy, and `mut` names a deliberately
wrong variant.  Elements outside the mask must come back as they went in (the canary, or the buffer's own contents where the op
runs in place), bit for bit."""
import functools

import numpy as np

U = 2.0 ** -24
H = 2.0 ** -11
CANARY = 0x7FA5C3E1   # RT_DEBUG_CANARY; as two fp16: 0xC3E1 (even index), 0x7FA5 (odd index, a NaN)
NONE, RELU, HSWISH = 0, 1, 2
LAB = (1.3, 0.07)
HSIG_LCNET, HSIG_MBV3, GATE_SIGMOID = 0.1666667, 0.2, -1.0   # the three gates nets_f16.cpp passes
OPS = ["dwconv16", "global_mean16", "gate16", "scale_channels16", "upsample_add16", "upsample_into16", "maxpool16", "avgpool16",
       "pixel_shuffle16", "deconv_to_map16", "map_window16", "u8_to_h8", "f32x4_to_h8", "h_to_f32", "f32_to_h"]
IMAGES = [(7, 9), (1, 1), (2, 5), (6, 4), (3, 18)]
POOL_PIX = 1024   # pixels per chunk of the mean's first stage
STALE = 0.375     # what the mean's scratch holds where no chunk sum was written (the chunks_alloc mutant reads it)


def h16(a):
    """round to fp16 (nearest even), back as float32"""
    return np.asarray(a).astype(np.float16).astype(np.float32)


def vals(rng, shape):
    """sign * uniform[1/16, 1] rounded to fp16: no operand and no product of two is subnormal"""
    return h16(rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0 / 16, 1.0, shape))


def offsets(imgs):
    o = np.concatenate([[0], np.cumsum([h * w for h, w in imgs])])
    return [int(v) for v in o]


def act64(v, act):
    if act == RELU:
        return np.maximum(v, 0)
    if act == HSWISH:
        return v * np.clip(v + 3, 0, 6) / 6
    return v


class Case:
    kind = "arith"        # "exact" | "arith" | "sigmoid"
    out_half = True
    in_place = None       # the buffer the output starts as (float32), for ops that run in place
    x2 = None
    tab = None
    res_add = False       # sigmoid: + 1 after the gate
    sig_scale = 1.0       # sigmoid: the factor on the sigmoid in the output (0.5 where the dot epilogue averages it into the map)
    sig_extra = 0.0       # sigmoid: what the arithmetic after the sigmoid may add (array over the buffer, or 0)

    def __init__(self, name, op, ip, fp, src, dst, x, out_rows, out_ld):
        self.name, self.op, self.src, self.dst = name, op, src, dst
        self.ip = np.zeros(12, np.int32)
        self.ip[:len(ip)] = ip
        self.fp = np.zeros(8, np.float32)
        self.fp[:len(fp)] = fp
        self.x, self.out_rows, self.out_ld = np.ascontiguousarray(x, np.float32), out_rows, out_ld

    # -- buffers ---------------------------------------------------------------------------------------------------------
    def shape(self):
        return (self.out_rows + 64, self.out_ld)

    def base_bits(self):
        """the output buffer before the launch, as bits of the output type"""
        n = (self.out_rows + 64) * self.out_ld
        if not self.out_half:
            b = np.full(n, CANARY, np.uint32)
            if self.in_place is not None:
                b[:self.in_place.size] = np.ascontiguousarray(self.in_place, np.float32).ravel().view(np.uint32)
            return b.reshape(self.shape())
        b = np.empty(n, np.uint16)
        b[0::2], b[1::2] = 0xC3E1, 0x7FA5
        if self.in_place is not None:
            b[:self.in_place.size] = self.in_place.astype(np.float16).ravel().view(np.uint16)
        return b.reshape(self.shape())

    def to_bits(self, out):
        """a float32 buffer as rt_debug_glue16 returns it -> bits of the output type"""
        out = np.asarray(out, np.float32).reshape(self.shape())
        return out.astype(np.float16).view(np.uint16) if self.out_half else out.view(np.uint32)

    def buffer(self, dtype=np.float32, mut=None):
        """what a kernel computing in `dtype` (rounding once to the output type) would return"""
        mask, v = self.compute(dtype, mut)
        bits = self.base_bits()
        if self.out_half:
            with np.errstate(over="ignore", invalid="ignore"):
                bits[mask] = v[mask].astype(np.float16).view(np.uint16)
            return bits.view(np.float16).astype(np.float32)
        bits[mask] = v[mask].astype(np.float32).view(np.uint32)
        return bits.view(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# checks
def check(case, out, sig_frac=1.0, f32=None, only=None):
    """Asserts everything the suite asks of one launch's output and returns the measured figures.  out: the float32 buffer as
    returned.  sig_frac: the c of the sigmoid bound as a fraction of |v| + 8.  f32: the stand-in's buffer for the
    rms rule (computed when None).  only: flat indices of the output elements to hold to the reference (the rest of the buffer is
    then the caller's to check)."""
    mask, y = case.compute(np.float64, None)
    got_bits, base = case.to_bits(out), case.base_bits()
    if only is not None:
        sel = np.zeros(mask.size, bool)
        sel[only] = True
        mask = mask & sel.reshape(mask.shape)
    untouched = got_bits[~mask] == base[~mask] if only is None else np.ones(1, bool)
    assert untouched.all(), "%s: %d elements outside the op's output were changed (first at flat index %d)" % (
        case.name, int((~untouched).sum()), int(np.flatnonzero(~mask)[np.argmin(untouched)]))
    zero = getattr(case, "zero", None)
    if zero is not None:   # elements the kernel writes as exact zeros (pad channels)
        assert (got_bits[zero] == 0).all(), "%s: %d pad elements are not +0" % (case.name, int((got_bits[zero] != 0).sum()))
        mask = mask & ~zero
    got = np.asarray(out, np.float32).reshape(case.shape())[mask].astype(np.float64)
    ref = y[mask]
    fig = {"n": int(mask.sum())}
    if case.kind == "exact":
        want = case.buffer(np.float64)
        same = case.to_bits(want)[mask] == got_bits[mask]
        assert same.all(), "%s: %d of %d elements differ from the reference's bits" % (case.name, int((~same).sum()), same.size)
        return fig
    assert np.isfinite(got).all(), "%s: non-finite output" % case.name
    err = np.abs(got - ref)
    if case.kind == "sigmoid":
        v = case.arg[mask]
        g = 1 / (1 + np.exp(-v))                      # fp64 sigmoid of the argument
        extra = case.sig_extra[mask] if isinstance(case.sig_extra, np.ndarray) else case.sig_extra
        rest = case.sig_scale * g * (1 - g) * case.arg_bound[mask] + (U * (1 + g) if case.res_add else 0) + extra   # (the rounding of the + 1)
        bound = rest + case.sig_scale * sig_frac * (np.abs(v) + 8) * U * g
        fig["c_frac"] = float(np.max((err - rest) / (case.sig_scale * (np.abs(v) + 8) * U * g)))
    else:
        hout = H if case.out_half else 2 * U
        T = case.T[mask] if isinstance(case.T, np.ndarray) else case.T
        bound = U * (T + 8) * case.S[mask] * case.L + hout * np.abs(ref) + 2.0 ** -25
    worst = int(np.argmax(err / bound))
    fig["worst"] = float(err[worst] / bound[worst])
    assert (err <= bound).all(), "%s: %d of %d elements outside the bound, worst err %.3e bound %.3e (ref %.6g got %.6g)" % (
        case.name, int((err > bound).sum()), err.size, err[worst], bound[worst], ref[worst], got[worst])
    if case.kind == "sigmoid":   # (no rms rule: __expf is allowed c ulps by the bound above, a libm float32 sigmoid has about one)
        return fig
    if f32 is None:
        f32 = case.buffer(np.float32)
    e32 = np.asarray(f32, np.float32).reshape(case.shape())[mask].astype(np.float64) - ref
    rms, rms32 = float(np.sqrt(np.mean(err ** 2))), float(np.sqrt(np.mean(e32 ** 2)))
    fig["rms"], fig["rms32"] = rms, rms32
    assert rms <= 2 * rms32, "%s: rms error %.3e is more than twice float32's %.3e" % (case.name, rms, rms32)
    return fig


# ----------------------------------------------------------------------------------------------------------------------------
# the ops
def _rows(buf, ld, off, c):
    return buf.reshape(-1, ld)[:, off:off + c]


class DwConv(Case):
    def __init__(self, K, sh, sw, mode, Cp=24, ldy=None, yoff=0, imgs=IMAGES):
        act, lab = {"none": (NONE, 0), "relu": (RELU, 0), "hswish_lab": (HSWISH, 1)}[mode]
        ldy = ldy or Cp
        dst = [((h + sh - 1) // sh, (w + sw - 1) // sw) for h, w in imgs]
        rng = np.random.default_rng(K * 100 + sh * 10 + sw + Cp)
        ps = offsets(imgs)[-1]
        ldx, xoff = Cp + 8, 8                                        # the input as a view of a wider buffer
        x = vals(rng, (ps, ldx))
        super().__init__("dwconv16 %dx%d s(%d,%d) %s Cp%d ldy%d" % (K, K, sh, sw, mode, Cp, ldy), 0,
                         [Cp, ldx, xoff, ldy, yoff, K, sh, sw, act, lab], LAB, imgs, dst, x, offsets(dst)[-1], ldy)
        self.w = h16(vals(rng, (K * K, Cp)) * (4 / np.sqrt(K * K)))
        self.b = rng.uniform(-1, 1, Cp).astype(np.float32)
        self.tab = np.concatenate([self.w.ravel(), self.b])
        self.K, self.sh, self.sw, self.act, self.lab, self.Cp, self.yoff = K, sh, sw, act, lab, Cp, yoff
        self.T, self.L = K * K + 1, (1.5 * abs(LAB[0]) if lab else 1.0)

    def compute(self, dtype, mut):
        K, sh, sw, Cp, P = self.K, self.sh, self.sw, self.Cp, self.K // 2
        xs = _rows(self.x, self.ip[1], self.ip[2], Cp).astype(dtype)
        w, b = self.w.astype(dtype), self.b.astype(dtype)
        taps = list(range(K * K))
        if mut == "taps_swapped":
            taps[0], taps[1] = taps[1], taps[0]
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        S = np.zeros(self.shape())
        so, do = offsets(self.src), offsets(self.dst)
        for (hh, ww), (ho, wo), o, q in zip(self.src, self.dst, so, do):
            pad = np.zeros((hh + 2 * P + sh, ww + 2 * P + sw, Cp), dtype)
            pad[P:P + hh, P:P + ww] = xs[o:o + hh * ww].reshape(hh, ww, Cp)
            acc = np.zeros((ho, wo, Cp), dtype) + b
            s_abs = np.zeros((ho, wo, Cp)) + np.abs(b)
            for t in range(K * K):
                dy, dx = t // K, t % K
                win = pad[dy:dy + (ho - 1) * sh + 1:sh, dx:dx + (wo - 1) * sw + 1:sw].copy()
                if mut == "tap_dropped_last_column" and dx == 0:
                    win[:, -1] = 0
                acc = acc + win * w[taps[t]]
                s_abs += np.abs(win.astype(np.float64)) * np.abs(w[taps[t]].astype(np.float64))
            if self.lab and mut == "lab_before_act":
                acc = act64(acc * dtype(np.float32(LAB[0])) + dtype(np.float32(LAB[1])), self.act)
            else:
                acc = act64(acc, self.act)
                if self.lab:
                    acc = acc * dtype(np.float32(LAB[0])) + dtype(np.float32(LAB[1]))
            v[q:q + ho * wo, self.yoff:self.yoff + Cp] = acc.reshape(-1, Cp)
            S[q:q + ho * wo, self.yoff:self.yoff + Cp] = s_abs.reshape(-1, Cp)
            mask[q:q + ho * wo, self.yoff:self.yoff + Cp] = True
        self.S = S
        return mask, v

    mutants = ("tap_dropped_last_column", "taps_swapped", "lab_before_act")


MEAN_IMAGES = [(1, 1), (31, 33), (32, 32), (25, 41), (7, 293), (2, 3), (3, 3), (1, 7), (5, 2)]   # 1, 1023, 1024, 1025, 2051 pixels + 4


class GlobalMean(Case):
    out_half = False
    L = 1.0

    def __init__(self, Cp, ldx=None, xoff=0):
        ldx = ldx or Cp
        rng = np.random.default_rng(Cp)
        ps = offsets(MEAN_IMAGES)[-1]
        x = h16(0.5 + rng.standard_normal((ps, ldx)))
        n = len(MEAN_IMAGES)
        super().__init__("global_mean16 Cp%d ldx%d" % (Cp, ldx), 1, [Cp, ldx, xoff, Cp, 0], [], MEAN_IMAGES, [(1, 1)] * n, x, n, Cp)
        self.Cp = Cp

    def compute(self, dtype, mut):
        Cp = self.Cp
        xs = _rows(self.x, self.ip[1], self.ip[2], Cp)
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        S, T = np.zeros(self.shape()), np.zeros(self.shape())
        largest = max(h * w for h, w in self.src)
        chunks_alloc = -(-largest // POOL_PIX)
        # the first stage's scratch [n_img][chunks_alloc][Cp]: an image writes its own ceil(n / 1024) chunk sums, the rest of its
        # row keeps what the scratch held (STALE); the second stage must add up the image's own chunks only
        partial = np.full((len(self.src), chunks_alloc, Cp), STALE, dtype)
        for i, ((hh, ww), o) in enumerate(zip(self.src, offsets(self.src))):
            n = hh * ww
            img = xs[o:o + n]
            chunks = -(-n // POOL_PIX)
            for k in range(chunks):
                partial[i, k] = img[k * POOL_PIX:(k + 1) * POOL_PIX].sum(axis=0, dtype=dtype)
            s = partial[i, :chunks_alloc if mut == "chunks_alloc" else chunks].sum(axis=0, dtype=dtype)
            v[i] = s / dtype(largest if mut == "largest_count" else n)
            S[i] = np.abs(img.astype(np.float64)).mean(axis=0)
            T[i] = n
            mask[i] = True
        self.S, self.T = S, T
        return mask, v

    mutants = ("largest_count", "chunks_alloc")


class Gate(Case):
    out_half = False
    T, L = 1, 1.0

    def __init__(self, slope, residual, C=20, Cp=24, lds=32, n=11):
        rng = np.random.default_rng(int(abs(slope) * 1000) + residual)
        lim = 6.0 if slope < 0 else 0.5 / slope
        x = rng.uniform(-2 * lim, 2 * lim, (n, lds)).astype(np.float32)
        if slope > 0:   # the clamp points themselves, and their float32 neighbours
            pts = np.float32([-0.5 / slope, 0.5 / slope, 0.0])
            x[0, :9] = np.concatenate([pts, np.nextafter(pts, np.float32(9)), np.nextafter(pts, np.float32(-9))])
        super().__init__("gate16 slope %g residual %d" % (slope, residual), 2, [C, lds, 0, Cp, 0, residual], [slope], [(1, 1)] * n,
                         [(1, 1)] * n, x, n, Cp)
        self.slope, self.residual, self.C, self.n = slope, residual, C, n
        if slope < 0:
            self.kind, self.res_add = "sigmoid", bool(residual)

    def compute(self, dtype, mut):
        C, n = self.C, self.n
        mask = np.zeros(self.shape(), bool)
        mask[:n] = True
        v = np.zeros(self.shape(), dtype)
        s = self.x[:, :C].astype(dtype)
        if self.slope < 0:
            g = 1 / (1 + np.exp(-s))
            self.arg = np.zeros(self.shape())
            self.arg[:n, :C] = self.x[:, :C]
            self.arg_bound = np.zeros(self.shape())
        else:
            g = np.clip(s * dtype(np.float32(self.slope)) + dtype(0.5), 0, 1)
        v[:n, :C] = g + (1 if self.residual else 0)
        if mut == "pad_nonzero":
            v[:n, C:] = v[:n, C - 1:C]
        S = np.zeros(self.shape())
        S[:n, :C] = np.abs(self.x[:, :C].astype(np.float64) * self.slope) + 0.5 + (1 if self.residual else 0)
        self.S = S
        self.zero = np.zeros(self.shape(), bool)
        self.zero[:n, C:] = True   # the pad columns C .. Cp
        return mask, v

    mutants = ("pad_nonzero",)


class ScaleChannels(Case):
    T, L = 2, 1.0

    def __init__(self, name, ldx, xoff, ldy, yoff, ldr, roff, in_place, Cp=24):
        rng = np.random.default_rng(ldx * 7 + ldy + ldr)
        ps = offsets(IMAGES)[-1]
        x = vals(rng, (ps, ldx))
        super().__init__("scale_channels16 " + name, 3, [Cp, ldx, xoff, ldy, yoff, ldr, roff, in_place], [], IMAGES, IMAGES, x, ps, ldy)
        self.tab = rng.uniform(1, 2, (len(IMAGES), Cp)).astype(np.float32)
        self.x2 = vals(rng, (ps, ldr)) if ldr else None
        self.in_place = self.x if in_place else None
        self.Cp = Cp

    def compute(self, dtype, mut):
        Cp, (_, ldx, xoff, ldy, yoff, ldr, roff) = self.Cp, self.ip[:7]
        xs = _rows(self.x, ldx, xoff, Cp).astype(dtype)
        img = np.repeat(np.arange(len(self.src)), [h * w for h, w in self.src])
        sc = self.tab.astype(dtype)[img if mut != "scale_of_image_0" else 0 * img]
        r = 0
        if ldr:
            r = _rows(self.x2, ldr, roff, Cp)
            if mut == "residual_at_output_pitch":   # the residual's rows walked with the output's pitch
                flat = np.concatenate([self.x2.ravel(), np.zeros(len(xs) * ldy, np.float32)])
                r = np.stack([flat[p * ldy + roff:p * ldy + roff + Cp] for p in range(len(xs))])
            r = r.astype(dtype)
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        S = np.zeros(self.shape())
        v[:len(xs), yoff:yoff + Cp] = xs * sc + r
        S[:len(xs), yoff:yoff + Cp] = np.abs(xs * sc) + np.abs(r)
        mask[:len(xs), yoff:yoff + Cp] = True
        self.S = S
        return mask, v

    mutants = ("scale_of_image_0", "residual_at_output_pitch")


def _up_index(src, dst, shift):
    """for every destination pixel: its image and the source pixel nearest-upsampling reads"""
    idx, img = [], []
    for i, ((hs, ws), (hd, wd), o) in enumerate(zip(src, dst, offsets(src))):
        yy, xx = np.meshgrid(np.arange(hd), np.arange(wd), indexing="ij")
        idx.append((o + np.minimum(yy >> shift, hs - 1) * ws + np.minimum(xx >> shift, ws - 1)).ravel())
        img.append(np.full(hd * wd, i))
    return np.concatenate(idx), np.concatenate(img)


class UpsampleAdd(Case):
    T, L = 2, 1.0

    def __init__(self, has_scale, Cp=96):
        B = [(1, 1), (3, 2), (2, 9)]
        A = [(2 * h, 2 * w) for h, w in B]
        rng = np.random.default_rng(40 + has_scale)
        x = vals(rng, (offsets(B)[-1], Cp))
        pd = offsets(A)[-1]
        super().__init__("upsample_add16 scale_a %d" % has_scale, 4, [Cp, Cp, 0, Cp, 0, 1, has_scale], [], B, A, x, pd, Cp)
        self.x2 = vals(rng, (pd, Cp))
        self.in_place = self.x2
        self.tab = rng.uniform(1, 2, (len(B), Cp)).astype(np.float32) if has_scale else None
        self.Cp, self.pd = Cp, pd

    def compute(self, dtype, mut):
        idx, img = _up_index(self.src, self.dst, 1)
        if mut == "source_not_halved":
            idx, _ = _up_index(self.src, self.dst, 0)
        a, b = self.x2.astype(dtype), self.x.astype(dtype)[idx]
        sc = 1 if self.tab is None else self.tab.astype(dtype)[0 * img if mut == "scale_of_image_0" else img]
        mask = np.zeros(self.shape(), bool)
        mask[:self.pd] = True
        v = np.zeros(self.shape(), dtype)
        v[:self.pd] = a * sc + b
        self.S = np.zeros(self.shape())
        self.S[:self.pd] = np.abs(a * sc) + np.abs(b)
        return mask, v

    mutants = ("source_not_halved", "scale_of_image_0")


class UpsampleInto(Case):
    T, L = 1, 1.0

    def __init__(self, shift, has_scale, C=24, ldd=96, ld_scale=32):
        S = [(1, 1), (3, 2), (2, 5)]
        D = [(h << shift, w << shift) for h, w in S]
        rng = np.random.default_rng(50 + shift * 2 + has_scale)
        x = vals(rng, (offsets(S)[-1], C))
        coff = (3 - shift) * C
        super().__init__("upsample_into16 shift %d scale %d" % (shift, has_scale), 5,
                         [C, C, 0, ldd, coff, shift, ld_scale if has_scale else 0], [], S, D, x, offsets(D)[-1], ldd)
        self.tab = rng.uniform(1, 2, (len(S), ld_scale)).astype(np.float32) if has_scale else None
        self.C, self.coff, self.shift = C, coff, shift
        if not has_scale:
            self.kind = "exact"

    def compute(self, dtype, mut):
        C, coff = self.C, self.coff
        idx, img = _up_index(self.src, self.dst, self.shift)
        b = self.x.astype(dtype)[idx]
        sc = 1
        if self.tab is not None:
            sc = self.tab.astype(dtype)[0 * img if mut == "scale_of_image_0" else img][:, :C]
            if mut == "scale_at_source_pitch":   # the table walked with the source's pitch (C) in place of its own
                sc = np.concatenate([self.tab.ravel(), np.ones(C, np.float32)]).astype(dtype)[img[:, None] * C + np.arange(C)]
        elif mut is not None:
            idx, _ = _up_index(self.src, self.dst, self.shift + 1)
            b = self.x.astype(dtype)[idx]
        n = len(idx)
        mask = np.zeros(self.shape(), bool)
        mask[:n, coff:coff + C] = True
        v = np.zeros(self.shape(), dtype)
        v[:n, coff:coff + C] = b * sc
        self.S = np.abs(v).astype(np.float64)
        return mask, v

    mutants = ("scale_of_image_0", "scale_at_source_pitch")


class Pool(Case):
    L = 1.0

    def __init__(self, op, name, k, s, p, imgs, dst, Cp, ldy, negative=()):
        rng = np.random.default_rng(Cp + k[0] * 10 + len(imgs))
        x = vals(rng, (offsets(imgs)[-1], Cp))
        for i in negative:   # all-negative images: a padding value of 0 in place of -inf shows
            x[offsets(imgs)[i]:offsets(imgs)[i + 1]] = -np.abs(x[offsets(imgs)[i]:offsets(imgs)[i + 1]])
        ip = [Cp, Cp, 0, ldy, 0, k[0], k[1]] + ([s[0], s[1], p[0], p[1]] if op == 6 else [])
        super().__init__(name, op, ip, [], imgs, dst, x, offsets(dst)[-1], ldy)
        self.k, self.s, self.p, self.Cp, self.is_max = k, s, p, Cp, op == 6
        self.kind = "exact" if self.is_max else "arith"
        self.T = k[0] * k[1]

    def compute(self, dtype, mut):
        (kh, kw), (sh, sw), (ph, pw), Cp = self.k, self.s, self.p, self.Cp
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        S = np.zeros(self.shape())
        fill = (0.0 if mut == "pad_zero" else -np.inf) if self.is_max else 0.0
        for (hh, ww), (ho, wo), o, q in zip(self.src, self.dst, offsets(self.src), offsets(self.dst)):
            pad = np.full((ph + max(hh, (ho - 1) * sh + kh), pw + max(ww, (wo - 1) * sw + kw), Cp), fill, dtype)
            pad[ph:ph + hh, pw:pw + ww] = self.x[o:o + hh * ww].reshape(hh, ww, Cp)
            wins = [pad[dy:dy + (ho - 1) * sh + 1:sh, dx:dx + (wo - 1) * sw + 1:sw] for dy in range(kh) for dx in range(kw)]
            if mut == "last_tap_dropped":
                wins = wins[:-1]
            if self.is_max:
                r = np.max(wins, axis=0)
            else:
                r = np.sum(wins, axis=0, dtype=dtype) * (dtype(1) / dtype(4 if mut == "over_4" else kh * kw))
                S[q:q + ho * wo, :Cp] = (np.sum(np.abs(wins), axis=0, dtype=np.float64) / (kh * kw)).reshape(-1, Cp)
            v[q:q + ho * wo, :Cp] = r.reshape(-1, Cp)
            mask[q:q + ho * wo, :Cp] = True
        self.S = S
        return mask, v


class PixelShuffle(Case):
    kind = "exact"

    def __init__(self, C, lds, ldd):
        rng = np.random.default_rng(C)
        D = [(2 * h, 2 * w) for h, w in IMAGES]
        x = vals(rng, (offsets(IMAGES)[-1], lds))
        super().__init__("pixel_shuffle16 C%d %d->%d" % (C, lds, ldd), 8, [C, lds, 0, ldd, 0], [], IMAGES, D, x, offsets(D)[-1], ldd)
        self.C = C

    def compute(self, dtype, mut):
        C = self.C
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        for (hs, ws), o, q in zip(self.src, offsets(self.src), offsets(self.dst)):
            s = self.x[o:o + hs * ws, :4 * C].reshape(hs, ws, 2, 2, C)          # [y][x][dy][dx][c]
            if mut == "phase_dx_dy":
                s = s.transpose(0, 1, 3, 2, 4)
            d = s.transpose(0, 2, 1, 3, 4).reshape(4 * hs * ws, C)               # [(2y + dy)][(2x + dx)][c]
            v[q:q + 4 * hs * ws, :C] = d
            mask[q:q + 4 * hs * ws, :C] = True
        return mask, v

    mutants = ("phase_dx_dy",)


FEATURE_IMAGES = [(1, 1), (3, 11), (5, 7)]   # 1, 33 and 35 pixels: groups of 8 lanes, 32 pixels per block


class DeconvToMap(Case):
    kind, out_half = "sigmoid", False

    def __init__(self, C, ldf):
        rng = np.random.default_rng(C + ldf)
        M = [(2 * h, 2 * w) for h, w in FEATURE_IMAGES]
        x = vals(rng, (offsets(FEATURE_IMAGES)[-1], ldf))
        x[:, C:] = np.nan   # the channels beyond C must not be read
        super().__init__("deconv_to_map16 C%d ldf%d" % (C, ldf), 9, [C, ldf, 0, 1, 0], [0.1], FEATURE_IMAGES, M, x, offsets(M)[-1], 1)
        self.tab = (rng.uniform(-1, 1, (C, 4)) * (4 / np.sqrt(C))).astype(np.float32)
        self.C = C

    def compute(self, dtype, mut):
        C = self.C
        n = self.out_rows
        f = self.x[:, :C + (8 if mut == "reads_past_C" and self.x.shape[1] > C else 0)].astype(dtype)
        w = self.tab.astype(dtype)
        if f.shape[1] > C:
            w = np.concatenate([w, np.zeros((f.shape[1] - C, 4), dtype)])
        b = dtype(np.float32(0.1))
        s = f @ w + b                                                            # [pix][dy * 2 + dx]
        sabs = np.abs(f[:, :C].astype(np.float64)) @ np.abs(self.tab.astype(np.float64)) + abs(float(b))
        arg, ab = np.zeros(n), np.zeros(n)
        for (hs, ws), o, q in zip(self.src, offsets(self.src), offsets(self.dst)):
            def place(a):
                a = a[o:o + hs * ws].reshape(hs, ws, 2, 2)
                if mut == "phase_dx_dy":
                    a = a.transpose(0, 1, 3, 2)
                return a.transpose(0, 2, 1, 3).reshape(-1)
            arg[q:q + 4 * hs * ws] = place(s)
            ab[q:q + 4 * hs * ws] = place(sabs)
        mask = np.zeros(self.shape(), bool)
        mask[:n] = True
        v = np.zeros(self.shape(), dtype)
        with np.errstate(invalid="ignore"):
            v[:n, 0] = 1 / (1 + np.exp(-arg.astype(dtype)))
        self.arg = np.zeros(self.shape())
        self.arg[:n, 0] = arg
        self.arg_bound = np.zeros(self.shape())
        self.arg_bound[:n, 0] = U * (C + 1 + 8) * ab                             # the C + 1 term fp32 sum behind the argument
        return mask, v

    mutants = ("phase_dx_dy",)


class MapWindow(Case):
    kind = "exact"

    def __init__(self, ldd=80, coff=64):
        rng = np.random.default_rng(7)
        M = [(2 * h, 2 * w) for h, w in FEATURE_IMAGES]
        x = rng.uniform(0, 1, offsets(M)[-1]).astype(np.float32)
        super().__init__("map_window16", 10, [16, 1, 0, ldd, coff], [], M, FEATURE_IMAGES, x, offsets(FEATURE_IMAGES)[-1], ldd)
        self.coff = coff

    def compute(self, dtype, mut):
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        lo = 0 if mut == "window_from_2y" else 1
        for (hm, wm), (hf, wf), o, q in zip(self.src, self.dst, offsets(self.src), offsets(self.dst)):
            m = self.x[o:o + hm * wm].reshape(hm, wm)
            pad = np.pad(m, 2, mode="edge" if mut == "border_clamped" else "constant")
            for i in range(4):
                for j in range(4):
                    win = pad[2 - lo + i:2 - lo + i + 2 * hf:2, 2 - lo + j:2 - lo + j + 2 * wf:2]
                    v[q:q + hf * wf, self.coff + 4 * i + j] = win.ravel()
            mask[q:q + hf * wf, self.coff:self.coff + 16] = True
        return mask, v

    mutants = ("border_clamped", "window_from_2y")


class U8ToH8(Case):
    T, L = 2, 1.0

    def __init__(self):
        pages, D = [(16, 16), (10, 30)], [(17, 16), (10, 31)]
        p = np.arange(offsets(pages)[-1])
        x = np.stack([(p * 3 + 1) % 256, (p * 5 + 7) % 256, (p * 7 + 14) % 256], axis=1).astype(np.float32)   # every byte value in each channel
        self.scale, self.mean, self.std = np.float32(1 / 255), np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
        super().__init__("u8_to_h8", 11, [8, 3, 0, 8, 0], [self.scale, *self.mean, *self.std], pages, D, x, offsets(D)[-1], 8)

    def compute(self, dtype, mut):
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        S = np.zeros(self.shape())
        for (hh, ww), o, q in zip(self.src, offsets(self.src), offsets(self.dst)):
            rgb = self.x[o:o + hh * ww].astype(dtype)
            bgr = rgb if mut == "rgb" else rgb[:, ::-1]
            v[q:q + hh * ww, :3] = (bgr * dtype(self.scale) - self.mean.astype(dtype)) / self.std.astype(dtype)
            S[q:q + hh * ww, :3] = (np.abs(bgr * float(self.scale)) + self.mean) / self.std
            mask[q:q + hh * ww] = True    # channels 3 .. 7 are written as zeros
        self.S = S
        self.zero = mask.copy()
        self.zero[:, :3] = False
        return mask, v

    mutants = ("rgb",)


def _conv_values(rng, shape):
    """values of several binades, with ones that round up to the next binade in fp16 (and fp16-exact ones)"""
    v = (rng.choice([-1.0, 1.0], shape) * rng.uniform(1, 2, shape) * 2.0 ** rng.integers(-6, 6, shape)).astype(np.float32)
    flat = v.ravel()
    flat[::7] = np.nextafter(np.float32(2.0) ** rng.integers(-5, 6, flat[::7].shape), np.float32(0)).astype(np.float32)
    return v


class Convert(Case):
    kind = "exact"

    def __init__(self, op, rows, lds, ldd, coff, C=120):
        rng = np.random.default_rng(op * 1000 + rows)
        if op == 12:
            C, lds, ldd, coff = 8, 4, 8, 0
        x = _conv_values(rng, (rows, lds))
        if op == 13:
            x = h16(x)
        super().__init__("%s rows %d %d->%d+%d" % (OPS[op], rows, lds, ldd, coff), op, [C, lds, 0, ldd, coff], [], [(1, rows)], [(1, rows)], x, rows, ldd)
        self.out_half = op != 13
        self.C, self.coff, self.rows = C, coff, rows

    def compute(self, dtype, mut):
        C, coff, n = self.C, self.coff, self.rows
        mask = np.zeros(self.shape(), bool)
        v = np.zeros(self.shape(), dtype)
        src = self.x[:, :4] if self.op == 12 else self.x[:, :C]
        if mut == "truncated":   # round toward zero in place of nearest-even
            bits = src.astype(np.float16).view(np.uint16)
            over = np.abs(src.astype(np.float16).astype(np.float32)) > np.abs(src)
            src = np.where(over, (bits - 1).astype(np.uint16).view(np.float16).astype(np.float32), src)
        if mut == "source_at_output_pitch":
            flat = np.concatenate([self.x.ravel(), np.zeros(n * self.out_ld, np.float32)])
            src = np.stack([flat[r * self.out_ld:r * self.out_ld + C] for r in range(n)])
        if mut == "last_channel_dropped":
            src = src.copy()
            src[:, -1] = 0.25
        if self.op == 12:
            v[:n, :4] = src
            mask[:n] = True       # channels 4 .. 7 are written as zeros
            self.zero = mask.copy()
            self.zero[:, :4] = False
        else:
            v[:n, coff:coff + C] = src
            mask[:n, coff:coff + C] = True
        return mask, v


# ----------------------------------------------------------------------------------------------------------------------------
# nh::conv16 through rt_debug_conv16x: epilogue and addressing forms
K_CONV16, K_CONV16V2, K_GEMM16P, ROUTE_DOT = 1, 2, 3, 8
ROUTE_NAMES = {1: "k_conv16", 2: "k_conv16v2", 3: "k_gemm16p", 10: "k_conv16v2<2, 4, 2, 1, ., false> (dot)"}
RAGGED = [(26, 100), (13, 37), (1, 1), (5, 16), (24, 17), (7, 2)]
PHASE_IMAGES = [(16, 16), (1, 1), (3, 40), (17, 5)]   # half resolution


def pitch8(c):
    return (c + 7) // 8 * 8


def _conv_image(img, w, sh, sw, pt, pl, ho, wo, dtype, mut=None):
    """img [h][w][cin], w [cout][cin][kh][kw] -> (acc [ho][wo][cout] in dtype, sum |w| |x| in float64); zero padding (pt, pl) at
    the top / left, whatever the output geometry implies at the bottom / right"""
    hh, ww, cin = img.shape
    cout, _, kh, kw = w.shape
    pad = np.zeros((max(hh + pt, (ho - 1) * sh + kh), max(ww + pl, (wo - 1) * sw + kw), cin), dtype)
    pad[pt:pt + hh, pl:pl + ww] = img
    acc, s_abs = np.zeros((ho, wo, cout), dtype), np.zeros((ho, wo, cout))
    taps = list(range(kh * kw))
    if mut == "taps_swapped":
        taps[0], taps[1] = taps[1], taps[0]
    for t in range(kh * kw):
        dy, dx = t // kw, t % kw
        win = pad[dy:dy + (ho - 1) * sh + 1:sh, dx:dx + (wo - 1) * sw + 1:sw].copy()
        if mut == "tap_dropped_last_column" and dx == 0:
            win[:, -1] = 0
        wt = w[:, :, taps[t] // kw, taps[t] % kw]
        acc = acc + (win.reshape(-1, cin) @ wt.T.astype(dtype)).reshape(ho, wo, cout)
        s_abs += (np.abs(win.reshape(-1, cin).astype(np.float64)) @ np.abs(wt.T.astype(np.float64))).reshape(ho, wo, cout)
    return acc, s_abs


class Conv16x(Case):
    """one conv16 launch with a store epilogue"""
    op = -1
    res = None
    dot_w = None

    def __init__(self, name, route, imgs, cin, cout, k=1, stride=(1, 1), flat=0, act=NONE, lab=0, ldx=None, xoff=0, ldy=None, coff=0,
                 ld_res=0, in_place=0, seed=0):
        kh = kw = k
        sh, sw = stride
        ldx, ldy = ldx or cin, ldy or pitch8(cout)
        rng = np.random.default_rng(1000 + seed)
        dst = [((h - 1) // sh + 1, (w - 1) // sw + 1) for h, w in imgs]
        pin, pout = offsets(imgs)[-1], offsets(dst)[-1]
        Case.__init__(self, "conv16x " + name, -1, [], [], imgs, dst, vals(rng, (pin, ldx)), pout, ldy)
        self.ip = np.array([cin, ldx, xoff, cout, ldy, coff, kh, kw, sh, sw, -1, -1, flat, act, lab, ld_res, 0, in_place, 0, 0], np.int32)
        self.fp = np.array([LAB[0], LAB[1], 0.0], np.float32)
        self.w = h16(vals(rng, (cout, cin, kh, kw)) * (4 / np.sqrt(cin * kh * kw)))
        self.b = rng.uniform(-1, 1, cout).astype(np.float32)
        if ld_res:
            self.res = vals(rng, (pout, ld_res))
        if in_place:
            self.in_place = self.x
        self.route, self.cin, self.cout, self.k, self.stride, self.act, self.lab = route, cin, cout, k, stride, act, lab
        self.T = cin * kh * kw + 1 + (1 if ld_res else 0)
        self.L = (1.5 if act == HSWISH else 1.0) * (abs(LAB[0]) if lab else 1.0)

    def compute(self, dtype, mut):
        cin, ldx, xoff, cout, ldy, coff = (int(v) for v in self.ip[:6])
        (sh, sw), k, ld_res = self.stride, self.k, int(self.ip[15])
        cop = pitch8(cout)
        if mut == "source_at_cin_pitch":   # the input's rows walked with the pitch Cin in place of ldx
            xs = self.x.ravel()[xoff:xoff + len(self.x) * cin].reshape(-1, cin).astype(dtype)
        else:
            xs = _rows(self.x, ldx, xoff, cin).astype(dtype)
        w, b = self.w.astype(dtype), self.b.astype(dtype)
        if mut == "bias_of_next_channel":
            b = np.roll(b, -1)
        mask, v, S = np.zeros(self.shape(), bool), np.zeros(self.shape(), dtype), np.zeros(self.shape())
        for (hh, ww), (ho, wo), o, q in zip(self.src, self.dst, offsets(self.src), offsets(self.dst)):
            acc, s_abs = _conv_image(xs[o:o + hh * ww].reshape(hh, ww, cin), w, sh, sw, k // 2, k // 2, ho, wo, dtype, mut)
            acc = (acc + b).reshape(-1, cout)
            s_abs = (s_abs + np.abs(self.b.astype(np.float64))).reshape(-1, cout)
            if self.lab and mut == "lab_before_act":
                acc = act64(acc * dtype(np.float32(LAB[0])) + dtype(np.float32(LAB[1])), self.act)
            else:
                acc = act64(acc, self.act)
                if self.lab:
                    acc = acc * dtype(np.float32(LAB[0])) + dtype(np.float32(LAB[1]))
            if ld_res:
                r = self.res[q:q + ho * wo, :cout]
                if mut == "residual_at_output_pitch":   # the residual's rows walked with the output's pitch
                    r = np.concatenate([self.res.ravel(), np.zeros(len(self.res) * ldy, np.float32)])[:len(self.res) * ldy].reshape(-1, ldy)[q:q + ho * wo, :cout]
                acc = acc + r.astype(dtype)
                s_abs = s_abs + np.abs(r.astype(np.float64))
            v[q:q + ho * wo, coff:coff + cout] = acc
            S[q:q + ho * wo, coff:coff + cout] = s_abs
            mask[q:q + ho * wo, coff:coff + cop] = True
        if mut == "pad_nonzero":
            v[:self.out_rows, coff + cout:coff + cop] = v[:self.out_rows, coff + cout - 1:coff + cout]
        self.S = S
        self.zero = np.zeros(self.shape(), bool)
        self.zero[:self.out_rows, coff + cout:coff + cop] = True   # the pad channels N .. pitch8(N)
        return mask, v

    def mutants(self):
        m = ["bias_of_next_channel"]
        if self.k > 1:
            m += ["tap_dropped_last_column", "taps_swapped"]
        if self.lab:
            m.append("lab_before_act")
        if self.res is not None and self.ip[15] != self.ip[4] and self.out_rows > 1:
            m.append("residual_at_output_pitch")
        if self.cout % 8:
            m.append("pad_nonzero")
        if self.ip[1] != self.cin and self.k == 1:
            m.append("source_at_cin_pitch")
        return tuple(m)


class Conv16Dot(Case):
    """the four PFHeadLocal 2x2 phase convs with the dot epilogue, in sequence on one map: phase (a, b) has pads (1 - a, 1 - b)
    and updates map pixel (2y + a, 2x + b) to 0.5 * (map + sigmoid(dot_b + sum_n relu(conv + bias)[n] dot_w[n]))"""
    op = -1
    kind, out_half = "sigmoid", False
    sig_scale = 0.5
    res = None
    route = K_CONV16V2 | ROUTE_DOT
    CIN, N = 80, 64

    def __init__(self):
        rng = np.random.default_rng(2200)
        imgs = PHASE_IMAGES
        maps = [(2 * h, 2 * w) for h, w in imgs]
        pin, pmap = offsets(imgs)[-1], offsets(maps)[-1]
        Case.__init__(self, "conv16x PFHeadLocal phase convs", -1, [], [], imgs, maps, vals(rng, (pin, self.CIN)), pmap, 1)
        self.w = h16(vals(rng, (4, self.N, self.CIN, 2, 2)) * (4 / np.sqrt(self.CIN * 4)))   # [2 a + b]
        self.b = rng.uniform(-1, 1, (4, self.N)).astype(np.float32)
        self.dot_w = (rng.uniform(-1, 1, self.N) * (4 / np.sqrt(self.N))).astype(np.float32)
        self.dot_b = np.float32(0.1)
        self.in_place = rng.uniform(0, 1, pmap).astype(np.float32)   # the map before the four launches
        self.fp = np.array([1.0, 0.0, self.dot_b], np.float32)

    def ip_of(self, a, b):
        return np.array([self.CIN, self.CIN, 0, self.N, 8, 0, 2, 2, 1, 1, 1 - a, 1 - b, 0, RELU, 0, 0, 0, 0, a, b], np.int32)

    def phase_pixels(self, a, b):
        """flat indices of the map pixels phase (a, b) owns"""
        idx = []
        for (hm, wm), o in zip(self.dst, offsets(self.dst)):
            yy, xx = np.meshgrid(np.arange(a, hm, 2), np.arange(b, wm, 2), indexing="ij")
            idx.append((o + yy * wm + xx).ravel())
        return np.concatenate(idx)

    def compute(self, dtype, mut):
        n, C, N = self.out_rows, self.CIN, self.N
        xs = self.x.astype(dtype)
        arg, ab = np.zeros(n, dtype), np.zeros(n)
        dw = self.dot_w.astype(dtype)
        for a in range(2):
            for b in range(2):
                w, bias = self.w[2 * a + b].astype(dtype), self.b[2 * a + b].astype(dtype)
                pa, pb = (b, a) if mut == "phase_b_a" else (a, b)   # where the result lands
                for (hh, ww), (hm, wm), o, q in zip(self.src, self.dst, offsets(self.src), offsets(self.dst)):
                    acc, s_abs = _conv_image(xs[o:o + hh * ww].reshape(hh, ww, C), w, 1, 1, 1 - a, 1 - b, hh, ww, dtype)
                    f = act64(acc + bias, RELU)
                    s = f @ dw + dtype(self.dot_b)
                    sa = (s_abs + np.abs(bias.astype(np.float64))) @ np.abs(self.dot_w.astype(np.float64)) + abs(float(self.dot_b))
                    arg[q:q + hm * wm].reshape(hm, wm)[pa::2, pb::2] = s
                    ab[q:q + hm * wm].reshape(hm, wm)[pa::2, pb::2] = sa
        m0 = self.in_place.astype(dtype)
        mask = np.zeros(self.shape(), bool)
        mask[:n] = True
        v = np.zeros(self.shape(), dtype)
        v[:n, 0] = dtype(0.5) * (m0 + 1 / (1 + np.exp(-arg)))
        self.arg = np.zeros(self.shape())
        self.arg[:n, 0] = arg
        self.arg_bound = np.zeros(self.shape())
        # the argument: N channels, each a sum of 4 C + 1 terms in fp32 (relu: L = 1), then the N + 1 term dot in fp32
        self.arg_bound[:n, 0] = U * ((4 * C + 1 + 8) + (N + 1 + 8)) * ab
        # after the sigmoid: map + sigmoid rounds once (U |map + sigmoid| = 2 U |y|), the halving is exact; the map before
        # contributes 0.5 * map exactly
        self.sig_extra = np.zeros(self.shape())
        self.sig_extra[:n, 0] = 2 * U * np.abs(v[:n, 0].astype(np.float64))
        return mask, v

    def check_step(self, before, after, a, b, sig_frac=1.0):
        """one phase launch changed nothing but its own pixels (bits of the fp32 map buffer), and every one of those now holds
        0.5 * (map + sigmoid) of this phase's conv, within the bound"""
        before, after = np.asarray(before, np.float32).view(np.uint32), np.asarray(after, np.float32).view(np.uint32)
        own = np.zeros(before.size, bool)
        own[self.phase_pixels(a, b)] = True
        assert (after[~own] == before[~own]).all(), "%s: phase (%d, %d) changed %d pixels of other phases or spare rows" % (
            self.name, a, b, int((after[~own] != before[~own]).sum()))
        # (0.5 * (m + s) == m only if s == m to the last bit; the map is uniform(0, 1), independent of the features)
        assert (after[own] != before[own]).mean() > 0.99, "%s: phase (%d, %d) left pixels of its own untouched" % (self.name, a, b)
        return check(self, after.view(np.float32), sig_frac=sig_frac, only=self.phase_pixels(a, b))

    def mutants(self):
        return ("phase_b_a",)


_CONV = {}
for _cin, _n in ((88, 16), (200, 32)):
    for _m in (1, 255, 4100):
        _CONV["conv16x-residual-%d-%d-M%d" % (_cin, _n, _m)] = functools.partial(
            Conv16x, "residual %d->%d M%d" % (_cin, _n, _m), K_CONV16, [(1, _m)], _cin, _n, flat=1, ld_res=pitch8(_n) + 8, seed=_cin + _m)
_CONV["conv16x-lab-48-96-M300"] = functools.partial(Conv16x, "LAB hswish 48->96 M300", K_CONV16, [(1, 300)], 48, 96, flat=1, act=HSWISH, lab=1, seed=1)
_CONV["conv16x-lab-240-240-M4100"] = functools.partial(Conv16x, "LAB hswish 240->240 M4100", K_GEMM16P, [(1, 4100)], 240, 240, flat=1, act=HSWISH, lab=1, seed=2)
_CONV["conv16x-pad-96-18"] = functools.partial(Conv16x, "pad channels 96->18 M257", K_CONV16, [(1, 257)], 96, 18, flat=1, ldy=40, coff=8, seed=3)
_CONV["conv16x-pad-192-42"] = functools.partial(Conv16x, "pad channels 192->42 M257", K_CONV16, [(1, 257)], 192, 42, flat=1, ldy=56, seed=4)
_CONV["conv16x-concat-3x3-ragged"] = functools.partial(Conv16x, "concat in place 3x3 32->32 ragged", K_CONV16V2, RAGGED, 32, 32, k=3, act=RELU,
                                                      ldx=96, xoff=32, ldy=96, coff=64, in_place=1, seed=5)
_CONV["conv16x-concat-1x1-flat"] = functools.partial(Conv16x, "concat in place 1x1 64->64 M4100", K_GEMM16P, [(1, 4100)], 64, 64, flat=1, act=RELU,
                                                    ldx=128, xoff=0, ldy=128, coff=64, in_place=1, seed=6)
_CONV["conv16x-3x3-s2-ragged"] = functools.partial(Conv16x, "3x3 stride 2 64->64 ragged", K_CONV16V2, RAGGED, 64, 64, k=3, stride=(2, 2), seed=7)
_CONV["conv16x-phase-dot"] = Conv16Dot
CONV_CASE_IDS = list(_CONV)


def _pool_case(which):
    if which == "max2 odd":
        return Pool(6, "maxpool16 2x2 s2 Cp200 odd", (2, 2), (2, 2), (0, 0), IMAGES, [((h + 1) // 2, (w + 1) // 2) for h, w in IMAGES], 200, 200, (0, 2))
    if which == "max2 even":
        im = [(6, 8), (2, 2), (4, 10)]
        return Pool(6, "maxpool16 2x2 s2 Cp200 even", (2, 2), (2, 2), (0, 0), im, [(h // 2, w // 2) for h, w in im], 200, 200, (1,))
    if which == "max3":
        return Pool(6, "maxpool16 3x3 s2 p1 Cp128 into pitch 256", (3, 3), (2, 2), (1, 1), IMAGES, [((h - 1) // 2 + 1, (w - 1) // 2 + 1) for h, w in IMAGES], 128, 256, (0, 2))
    im = [(3, 2), (3, 3), (3, 7), (3, 50)]
    return Pool(7, "avgpool16 3x2 C480 into pitch 960", (3, 2), (3, 2), (0, 0), im, [(1, w // 2) for _, w in im], 480, 960)


DW_FORMS = [(3, 1, 1), (3, 2, 2), (3, 2, 1), (3, 1, 2), (5, 1, 1), (5, 2, 2), (5, 2, 1)]
_BUILDERS = {}
for _k, _sh, _sw in DW_FORMS:
    for _m in ("none", "relu", "hswish_lab"):
        _BUILDERS["dwconv16-%d-s%d%d-%s" % (_k, _sh, _sw, _m)] = functools.partial(DwConv, _k, _sh, _sw, _m)
_BUILDERS["dwconv16-3-s22-concat72"] = functools.partial(DwConv, 3, 2, 2, "relu", 24, 72, 0)
_BUILDERS["dwconv16-5-s11-Cp200"] = functools.partial(DwConv, 5, 1, 1, "hswish_lab", 200)
_BUILDERS["global_mean16-Cp24-view"] = functools.partial(GlobalMean, 24, 72, 24)
_BUILDERS["global_mean16-Cp200"] = functools.partial(GlobalMean, 200)
_BUILDERS["global_mean16-Cp2048"] = functools.partial(GlobalMean, 2048)
for _s, _n in ((HSIG_LCNET, "lcnet"), (HSIG_MBV3, "mbv3"), (GATE_SIGMOID, "sigmoid")):
    for _r in (0, 1):
        _BUILDERS["gate16-%s-res%d" % (_n, _r)] = functools.partial(Gate, _s, _r)
_BUILDERS["scale_channels16-plain"] = functools.partial(ScaleChannels, "x 24 -> y 72+24", 24, 0, 72, 24, 0, 0, 0)
_BUILDERS["scale_channels16-res"] = functools.partial(ScaleChannels, "x 72+48, res 48+16 -> y 24", 72, 48, 24, 0, 48, 16, 0)
_BUILDERS["scale_channels16-inplace"] = functools.partial(ScaleChannels, "in place 48+24, res 24", 48, 24, 48, 24, 24, 0, 1)
for _r in (0, 1):
    _BUILDERS["upsample_add16-scale%d" % _r] = functools.partial(UpsampleAdd, _r)
    for _j in range(4):
        _BUILDERS["upsample_into16-shift%d-scale%d" % (_j, _r)] = functools.partial(UpsampleInto, _j, _r)
for _w in ("max2 odd", "max2 even", "max3", "avg"):
    _BUILDERS[("maxpool16-" if _w != "avg" else "avgpool16-") + _w.replace(" ", "-")] = functools.partial(_pool_case, _w)
_BUILDERS["pixel_shuffle16-C24"] = functools.partial(PixelShuffle, 24, 96, 24)
_BUILDERS["pixel_shuffle16-C64"] = functools.partial(PixelShuffle, 64, 256, 80)
_BUILDERS["deconv_to_map16-C24"] = functools.partial(DeconvToMap, 24, 24)
_BUILDERS["deconv_to_map16-C64"] = functools.partial(DeconvToMap, 64, 80)
_BUILDERS["map_window16"] = MapWindow
_BUILDERS["u8_to_h8"] = U8ToH8
for _op in (12, 13, 14):
    for _nr, _lds, _ldd, _coff in ((1, 120, 120, 0), (255, 128, 128, 8), (257, 120, 128, 8)):
        _BUILDERS["%s-rows%d" % (OPS[_op], _nr)] = functools.partial(Convert, _op, _nr, _lds, _ldd, _coff)
CASE_IDS = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(case_id):
    return (_BUILDERS.get(case_id) or _CONV[case_id])()


def mutants_of(c):
    """the wrong variants of a case's op that its data can tell from the right one"""
    if isinstance(c, (Conv16x, Conv16Dot)):
        return c.mutants()
    if isinstance(c, DwConv):
        return ("tap_dropped_last_column", "taps_swapped") + (("lab_before_act",) if c.lab else ())
    if isinstance(c, Pool):
        return ("pad_zero" if c.p != (0, 0) or any(2 * a != h for (a, _), (h, _) in zip(c.dst, c.src)) else "last_tap_dropped",) if c.is_max else ("over_4",)
    if isinstance(c, ScaleChannels):
        return ("scale_of_image_0",) + (("residual_at_output_pitch",) if c.ip[5] and c.ip[5] != c.ip[3] else ())
    if isinstance(c, UpsampleAdd):
        return ("source_not_halved",) + (("scale_of_image_0",) if c.tab is not None else ())
    if isinstance(c, UpsampleInto):
        return ("scale_of_image_0", "scale_at_source_pitch") if c.tab is not None else ("source_shift_plus_1",)
    if isinstance(c, DeconvToMap):
        return ("phase_dx_dy",) + (("reads_past_C",) if c.x.shape[1] > c.C else ())
    if isinstance(c, Convert):
        return ("last_channel_dropped",) + (("truncated",) if c.op != 13 and c.rows > 1 else ()) + (("source_at_output_pitch",) if c.op != 12 and c.ip[1] != c.ip[3] else ())
    return c.mutants

