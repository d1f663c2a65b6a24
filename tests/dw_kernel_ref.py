"""fp64 references, float32 stand-ins (torch on the CPU), mutants and the cases for the fp32 depthwise kernels (k_dwconv_rows,
k_dwconv_sweep, one launch through rt_debug_dwconv) and the wide LCNetV3 blocks run_lc builds from them (depthwise -> squeeze-excite
from the depthwise kernel's partial sums -> pointwise GEMM with the scales folded into its A rows, or run_se in place; through
rt_debug_lc_wide).  tests/test_gpu_dw_kernels.py on the GPU, tests/test_dw_kernel_checks_cpu.py here.  No device.  check(), Out and
the operand helpers are those of tests/cls_kernel_ref.py.

A case holds the host arrays as its entry takes them and `compute(dtype, mut=None)`: the plain mathematics in `dtype` arithmetic,
one Out per returned buffer.  torch.float64 is the reference (and carries the element bounds), torch.float32 the stand-in of the
rms rule and what the mutants are applied to.  The convolution is the zero-padded sum over taps per image; nothing here walks
strips or tiles except the LAYOUT of the pooled partial sums, which is what that buffer is (dw_plan() below restates nn::dw_plan;
the CPU test holds it to the plan driver, the GPU test to rt_debug_dw_plan).

Operands: uniform(-1, 1) float32, pointwise weights scaled by 4 / sqrt(K), every bias random per channel, two different LAB
pairs (neither (1, 0)), and non-zero noise in the input's pad channels C .. Cp (240 in 256): the kernel promises +0 there
whatever the input padding held.

Bounds.  U = 2^-24; the suite's stage bound: a K-term fp32 sum of products costs U (K + 2) S (K + 8 for a GEMM row) with S =
|b| + sum |w| |x|, an activation passes errors through its Lipschitz factor, each epilogue rounding costs 4 U |y|.
  depthwise    d = lab(act(dw(x) + b))       dd = L U (K K + 2) S + 4 U |d|,  L = 1.5 |lab_a| with hardswish, |lab_a| or 1 without
  partial sum  p = sum of n outputs          dp = sum dd + U (n + 2) sum |d|        (n = the pixels of the block's strips)
  mean         m = sum d / P                 dm = mean dd + U (P + 2) mean |d|      (the n-term bound of test_gpu_dwconv_sweep.py)
  FCs          h = relu(W1 m + b1)           dh = sum |W1| dm + U (C + 8) S_h
               s = clamp(h W2 / 6 + b2 / 6 + 0.5)   ds = (sum |W2| dh + U (Cr + 8) S_s) / 6 + 4 U
  scale        z = d s                       dz = dd s + |d| ds + U |z|             (z = d, dz = dd without squeeze-excite)
  pointwise    y = lab(hswish(Wp z + bp))    dy = 1.5 |lab_a| (sum |Wp| dz + U (C + 8) S_y) + 4 U |y|
The y1 buffer is held to dd where the scales are folded into the GEMM (it stays unscaled) and to dz where run_se scaled it in place.
Constants that are not derived: the + 2 / + 8 slack terms and the 4 U per epilogue are the suite's convention.

No element of any returned buffer is left out: outside an Out's mask every word must still be RT_DEBUG_CANARY -- the 64 spare
rows (which rt_debug_dwconv's partial sums and means do not have on the device: the GPU test says what that leaves unseen), the partial-sum slots of blocks an image does not own, the output's columns past cout -- and `zero` elements must be +0
(channels C .. Cp of the depthwise output, the partial sums, the means, the scales).

Out of scope: the 3-int row table of k_gemm32p+se starts at M = 131072 rows; an fp64 block of that size is no test of seconds
(tests/test_gpu_ops.py::test_gemm_squeeze_excite keeps holding that kernel on scales and a table it supplies)."""
import functools

import numpy as np
import torch

import cls_kernel_ref as B
from cls_kernel_ref import ACT_HSWISH, ACT_NONE, CANARY, N, Out, T, U, act_fn, chan_pitch, check, offsets, uni  # noqa: F401

HSIG_SLOPE = float(np.float32(0.1666667))   # HSIG_LCNET of nets.cpp
LAB_DW, LAB_PW = (1.3, 0.07), (0.8, -0.05)
ROWS32, ROWS64, SWEEP = 1, 2, 3             # nn::DwKernel
GEMM_KERNELS = ["none", "invalid", "split", "w", "dma", "wide_256x240", "wide_128x240", "wide_128x128", "stream", "narrow"]   # nn::GemmKernel
SWEEPS = [(5, 1, 1, 5, 1, 3), (3, 1, 1, 3, 2, 0), (5, 2, 1, 3, 4, 5), (3, 1, 2, 3, 6, 0)]   # lc_plan.cpp: K, sh, sw, min_ho, inst, pooled inst


def dw_plan(K, sh, sw, Cp, maxHo, maxWo, pooled, sweep_on):
    """nn::dw_plan restated: (kernel, inst, R, lanes, spb, chunks, grid_x, grid_z)"""
    R = 3 if (maxHo == 6 or (maxHo == 3 and sh == 1)) else (4 if sh == 1 else 2)
    wide = (Cp >= 192 and (sw == 1 or (sh == 2 and R == 2))) if K == 5 else (Cp >= 128 and sh == 1 and R == 4 and not pooled)
    lanes = 16 if wide else 8
    spb = 256 // lanes
    sx, sy = (maxWo + 3) // 4, (maxHo + R - 1) // R
    chunks = (sx * sy + spb - 1) // spb
    grid_z = (Cp + lanes * 4 - 1) // (lanes * 4)
    inst = 0
    if sweep_on and wide and maxHo * sh <= 24:
        for k, a, b, min_ho, i, ip in SWEEPS:
            if (k, a, b) == (K, sh, sw) and maxHo >= min_ho:
                inst = i if not pooled else (ip if (R == 3 and sy <= 4) else 0)
    if inst:
        return (SWEEP, inst, R, lanes, spb, chunks, (sx + spb - 1) // spb, grid_z)
    return (ROWS64 if wide else ROWS32, (((lanes * 8 + K) * 8 + R) * 4 + sh) * 4 + sw, R, lanes, spb, chunks, chunks, grid_z)


def instance_name(plan, K, sh, sw, pooled):
    if plan[0] == SWEEP:
        return "sweep %d" % plan[1]
    return "rows<%d,%d,%d,%d,%d,%d>" % (K, plan[2], sh, sw, int(bool(pooled)), plan[3])


def all_instances():
    """the 44 k_dwconv_rows and 6 k_dwconv_sweep instances of dwconv()'s switch (nn_kernels.hip)"""
    s = {"sweep %d" % i for i in range(1, 7)}
    for p in (0, 1):
        for R in (3, 4):
            s.add("rows<5,%d,1,1,%d,16>" % (R, p))
        for R in (3, 2):
            s.add("rows<5,%d,2,1,%d,16>" % (R, p))
        s.add("rows<5,2,2,2,%d,16>" % p)
        for K in (3, 5):
            for sh, sw in ((1, 1), (1, 2), (2, 1), (2, 2)):
                for R in (3, 4 if sh == 1 else 2):
                    s.add("rows<%d,%d,%d,%d,%d,8>" % (K, R, sh, sw, p))
    s |= {"rows<3,4,1,1,0,16>", "rows<3,4,1,2,0,16>"}
    return s


def takes_xcd_remap(plan, n_img):
    """the branch at the top of k_dwconv_rows: the (strip block, image) grid a multiple of 8 (the sweep kernel has no remap)"""
    return plan[0] != SWEEP and plan[6] * n_img >= 8 and (plan[6] * n_img) % 8 == 0


def out_dims(imgs, sh, sw):
    return [((h + sh - 1) // sh, (w + sw - 1) // sw) for h, w in imgs]


# ----------------------------------------------------------------------------------------------------------------------------
# the plain operations
def dwconv(x, imgs, w, K, sh, sw, mut=None):
    """x [pixels][C] (the images consecutive), w [K][K][C] -> [output pixels][C]: the zero-padded K x K depthwise sum per image,
    stride (sh, sw), without bias.  The mutants of the tap loop read through an index map of the flat buffer instead."""
    P, C = K // 2, x.shape[1]
    offs, total, res = offsets(imgs), x.shape[0], []
    if mut == "taps_transposed":
        w = w.transpose(0, 1)
    ty, tx = (sw, sh) if mut == "stride_swapped" else (sh, sw)   # (the output geometry stays the caller's)
    for i, (H, W) in enumerate(imgs):
        Ho, Wo = (H + sh - 1) // sh, (W + sw - 1) // sw
        y = torch.zeros((Ho, Wo, C), dtype=x.dtype)
        if mut in (None, "taps_transposed"):
            xp = torch.zeros((H + 2 * P + sh, W + 2 * P + sw, C), dtype=x.dtype)
            xp[P:P + H, P:P + W] = x[offs[i]:offs[i + 1]].reshape(H, W, C)
            for dy in range(K):
                for dx in range(K):
                    y += xp[dy:dy + (Ho - 1) * sh + 1:sh, dx:dx + (Wo - 1) * sw + 1:sw] * w[dy, dx]
        else:
            oy, ox = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
            for dy in range(K):
                for dx in range(K):
                    iy, ix = oy * ty + dy - P, ox * tx + dx - P
                    flat = offs[i] + iy * W + ix
                    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                    if mut == "row_below_next_image":      # no test against the image's height: the rows that follow in memory
                        ok = (iy >= 0) & (ix >= 0) & (ix < W) & (flat < total)
                    if mut == "col_right_wraps":           # no test against the image's width: the next row's first pixels
                        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (flat < total)
                    if mut == "tap_dropped_strip_end" and dy == P and dx == K - 1:
                        ok = ok & (ox % 4 != 3)
                    v = x[flat.clamp(0, total - 1).reshape(-1)].reshape(Ho, Wo, C)
                    y += torch.where(ok[..., None], v, torch.zeros((), dtype=x.dtype)) * w[dy, dx]
        res.append(y.reshape(Ho * Wo, C))
    return torch.cat(res)


def tail(acc, b, act, lab, mut=None):
    """bias, activation, LAB"""
    a, c = lab if lab else (1.0, 0.0)
    if mut == "bias_after_act":
        t = act_fn(acc, act) + b
    elif mut == "lab_before_act":
        return act_fn((acc + b) * a + c, act) if lab else act_fn(acc + b, act)
    else:
        t = act_fn(acc + b, act)
    return t * a + c if lab else t


def tail_lip(act, lab):
    return (1.5 if act == ACT_HSWISH else 1.0) * (abs(lab[0]) if lab else 1.0)


def strip_blocks(Ho, Wo, R, spb, row_major=False):
    """block of the pooled layout each output pixel of an Ho x Wo image falls in: strips of R rows x 4 pixels numbered column-major,
    spb strips per block -> ([Ho * Wo] block index, blocks of the image)"""
    sx, sy = (Wo + 3) // 4, (Ho + R - 1) // R
    oy, ox = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
    strip = (oy // R) * sx + ox // 4 if row_major else (ox // 4) * sy + oy // R
    return (strip // spb).reshape(-1), (sx * sy + spb - 1) // spb


def strips_mutant(Ho, Wo, R, spb, chunks, mut):
    """the two ways the strip height of the pooled layout can disagree between k_dwconv_rows and k_se_fc, which count an image's
    blocks each from the image's OWN height -- ceil(W / 4) * ceil(H / R) strips -- while dw_plan() chose R from the batch's
    largest.  On a 6-row map (R = 3) a 4-row image has two strips per column with R = 3 and one with R = 4.
      strips_r4        the row kernel instantiated with R + 1: it fills fewer slots, k_se_fc adds one that still holds the canary
      se_fc_strip_r4   k_se_fc handed strip_R = R + 1: it counts fewer blocks than the image owns
    -> (the R of the layout written, pixels whose block k_se_fc adds [Ho * Wo] bool, whether it adds an unwritten slot)"""
    blk, own = strip_blocks(Ho, Wo, R, spb)
    short = min(strip_blocks(Ho, Wo, R + 1, spb)[1], chunks)
    if mut == "strips_r4":
        return R + 1, torch.ones(Ho * Wo, dtype=torch.bool), short < min(own, chunks)
    if mut == "se_fc_strip_r4":
        return R, blk < short, False
    return R, torch.ones(Ho * Wo, dtype=torch.bool), False


CANARY_F32 = np.array(CANARY, np.uint32).view(np.float32).item()   # a NaN


class Case(B.Case):
    def reference(self):
        if getattr(self, "_ref", None) is None:
            self._ref = self.compute(torch.float64)
        return self._ref


class Dw(Case):
    """one rt_debug_dwconv launch"""
    family = "dw"

    def __init__(self, name, K, C, sh, sw, act, lab, pooled, form, imgs, seed):
        self.name, self.K, self.C, self.Cp, self.sh, self.sw = name, K, C, chan_pitch(C), sh, sw
        self.act, self.lab, self.pooled, self.form, self.imgs = act, lab, pooled, form, imgs
        self.outs = out_dims(imgs, sh, sw)
        self.maxHo, self.maxWo = max(h for h, _ in self.outs), max(w for _, w in self.outs)
        self.plan = dw_plan(K, sh, sw, self.Cp, self.maxHo, self.maxWo, pooled, form)
        self.instance = instance_name(self.plan, K, sh, sw, pooled)
        self.remap = takes_xcd_remap(self.plan, len(imgs))
        rng = np.random.default_rng(seed)
        pix = offsets(imgs)[-1]
        self.x = uni(rng, (pix, self.Cp))                        # (the pad channels hold noise)
        self.w = np.zeros((K * K, self.Cp), np.float32)          # [tap dy * K + dx][Cp], as pack_dw lays it out
        self.w[:, :C] = uni(rng, (K * K, C), 4 / K)
        self.b = np.zeros(self.Cp, np.float32)
        self.b[:C] = uni(rng, (C,))

    def compute(self, dt, mut=None):
        c, K, C, Cp = self, self.K, self.C, self.Cp
        ref = dt == torch.float64
        x, w, b = T(c.x[:, :C], dt), T(c.w[:, :C].reshape(K, K, C), dt), T(c.b[:C], dt)
        y = tail(dwconv(x, c.imgs, w, K, c.sh, c.sw, mut), b, c.act, c.lab, mut)
        oo = offsets(c.outs)
        pout, n = oo[-1], len(c.imgs)
        dd = None
        if ref:
            dd = tail_lip(c.act, c.lab) * U * (K * K + 2) * (dwconv(x.abs(), c.imgs, w.abs(), K, c.sh, c.sw) + b.abs()) + 4 * U * y.abs()
        o = Out("y", pout, Cp)
        o.mask[:pout] = True
        o.zero[:pout, C:] = True
        o.fill(slice(0, pout), C, N(y), None if dd is None else N(dd))
        if mut == "pad_passthrough":            # the pad lanes' own results: the input noise at the centre tap
            offs = offsets(c.imgs)
            for i, ((H, W), (Ho, Wo)) in enumerate(zip(c.imgs, c.outs)):
                src = c.x[offs[i]:offs[i + 1], C:].reshape(H, W, Cp - C)[::c.sh, ::c.sw][:Ho, :Wo]
                o.v[oo[i]:oo[i + 1], C:] = src.reshape(Ho * Wo, Cp - C)
        if mut == "last_strip_unwritten":
            for i, (Ho, Wo) in enumerate(c.outs):
                r0 = (Ho - 1) // c.plan[2] * c.plan[2]
                o.mask[oo[i] + r0 * Wo:oo[i + 1]] = False
        if not c.pooled:
            return [o]
        _, _, R, _, spb, chunks, gx, _ = c.plan
        po, mo = Out("partial", n * chunks, Cp), Out("mean", n, Cp)
        mo.mask[:n] = True
        mo.zero[:n, C:] = True
        for i, (Ho, Wo) in enumerate(c.outs):
            yi = y[oo[i]:oo[i + 1]]
            Rw, counted, unwritten = strips_mutant(Ho, Wo, R, spb, chunks, mut)
            blk, nblk = strip_blocks(Ho, Wo, Rw, spb, mut == "pool_row_major")
            nblk = min(nblk, chunks)
            psum = torch.zeros((nblk, C), dtype=dt).index_add_(0, blk.clamp(max=nblk - 1), yi)
            rows = slice(i * chunks, i * chunks + nblk)
            po.mask[rows] = True
            po.zero[rows, C:] = True
            P = Ho * Wo
            mean = yi[counted].sum(0) / (c.maxHo * c.maxWo if mut == "mean_div_max" else P)
            if (mut == "pool_foreign_block" and nblk < chunks) or unwritten:    # a slot the image did not fill still holds the canary
                mean = mean + torch.tensor(CANARY_F32, dtype=dt)
            pb = mb = None
            if ref:
                cnt = torch.zeros(nblk, dtype=dt).index_add_(0, blk, torch.ones(P, dtype=dt))[:, None]
                zeros = torch.zeros((nblk, C), dtype=dt)
                pb = N(zeros.clone().index_add_(0, blk, dd[oo[i]:oo[i + 1]]) + U * (cnt + 2) * zeros.clone().index_add_(0, blk, yi.abs()))
                mb = N(dd[oo[i]:oo[i + 1]].mean(0) + U * (P + 2) * yi.abs().mean(0))
            po.fill(rows, C, N(psum), pb)
            mo.fill(slice(i, i + 1), C, N(mean), mb)
        if mut == "pool_unremapped" and c.remap:   # work item w = (lin & 7) * (total / 8) + lin / 8 stored at its raw block index lin
            total = gx * n
            lin = np.arange(total)
            src = (lin & 7) * (total // 8) + (lin >> 3)
            for arr in (po.v, po.mask, po.zero, po.bound):
                arr[:total] = arr[:total][src]
        return [o, po, mo]


class Lc(Case):
    """one block through rt_debug_lc_wide"""
    family = "block"

    def __init__(self, name, K, cin, cout, sh, sw, se, form, imgs, scaled, seed):
        """scaled: None without squeeze-excite, "fold" (the scales folded into the GEMM: y1 stays unscaled) or "place" (run_se)"""
        self.name, self.K, self.cin, self.cout, self.sh, self.sw, self.se, self.form = name, K, cin, cout, sh, sw, se, form
        self.imgs, self.scaled = imgs, scaled
        self.Cp, self.ldy = chan_pitch(cin), chan_pitch(cout)
        self.act, self.lab = (ACT_NONE, None) if (sh, sw) == (2, 2) else (ACT_HSWISH, LAB_DW)   # LearnableRepLayer: no tail at stride 2
        self.outs = out_dims(imgs, sh, sw)
        self.maxHo, self.maxWo = max(h for h, _ in self.outs), max(w for _, w in self.outs)
        self.rows, self.min_pix = offsets(self.outs)[-1], min(h * w for h, w in self.outs)
        self.plan = dw_plan(K, sh, sw, self.Cp, self.maxHo, self.maxWo, scaled == "fold", form)
        rng = np.random.default_rng(seed)
        self.x = uni(rng, (offsets(imgs)[-1], self.Cp))
        self.x[offsets(imgs)[1]:offsets(imgs)[2]] *= np.float32(0.25)      # image 1 sits in hardswish's curved part
        self.dw_w, self.dw_b = uni(rng, (cin, K, K), 4 / K), uni(rng, (cin,))
        self.pw_w, self.pw_b = uni(rng, (cout, cin), 4 / np.sqrt(cin)), uni(rng, (cout,))
        self.fc = None
        if se:
            with torch.no_grad():
                d = self.depthwise(torch.float64)
            oo = offsets(self.outs)
            means = np.stack([N(d[oo[i]:oo[i + 1]].mean(0)) for i in range(len(imgs))])
            self.fc = B.se_weights(rng, means, cin, cin // 4, HSIG_SLOPE)

    def depthwise(self, dt, mut=None):
        c = self
        x, w, b = T(c.x[:, :c.cin], dt), T(c.dw_w, dt).permute(1, 2, 0), T(c.dw_b, dt)
        return tail(dwconv(x, c.imgs, w, c.K, c.sh, c.sw, mut), b, c.act, c.lab, mut)

    def compute(self, dt, mut=None):
        c, C, Cp, n = self, self.cin, self.Cp, len(self.imgs)
        ref = dt == torch.float64
        a = lambda t: t.abs()   # noqa: E731
        d = c.depthwise(dt, mut)
        oo = offsets(c.outs)
        P = oo[-1]
        img = torch.repeat_interleave(torch.arange(n), torch.tensor([h * w for h, w in c.outs]))
        dd = None
        if ref:
            x, w, b = T(c.x[:, :C], dt), T(c.dw_w, dt).permute(1, 2, 0), T(c.dw_b, dt)
            dd = tail_lip(c.act, c.lab) * U * (c.K * c.K + 2) * (dwconv(a(x), c.imgs, a(w), c.K, c.sh, c.sw) + a(b)) + 4 * U * a(d)
        Wp, bp = T(c.pw_w, dt), T(c.pw_b, dt)
        outs, z, dz, s = [], d, dd, None
        if c.se:
            W1, b1, W2, b2 = (T(v, dt) for v in c.fc)
            m = torch.stack([d[oo[i]:oo[i + 1]].mean(0) for i in range(n)])
            if mut in ("strips_r4", "se_fc_strip_r4") and c.scaled == "fold":   # (the pooled layout exists where the fold is on)
                for i, (Ho, Wo) in enumerate(c.outs):
                    _, counted, unwritten = strips_mutant(Ho, Wo, c.plan[2], c.plan[4], c.plan[5], mut)
                    m[i] = d[oo[i]:oo[i + 1]][counted].sum(0) / (Ho * Wo) + (CANARY_F32 if unwritten else 0.0)
            h = torch.relu(m @ W1.T + b1)
            t = (0.2 if mut == "hsig_slope_02" else HSIG_SLOPE) * (h @ W2.T + b2) + 0.5
            s = torch.clamp(t, 0.0, 1.0)
            if mut == "scale_prev_image":
                s = torch.roll(s, 1, 0)
            rows_img = img
            if mut == "row_table_equal_images":      # the table of a batch of n equal images
                rows_img = (torch.arange(P) // ((P + n - 1) // n)).clamp(max=n - 1)
            z = d * s[rows_img]
            so = Out("scale", n, Cp)
            so.mask[:n] = True
            so.zero[:n, C:] = True
            ds = None
            if ref:
                Pi = torch.tensor([float(hh * ww) for hh, ww in c.outs], dtype=dt)[:, None]
                dm = torch.stack([dd[oo[i]:oo[i + 1]].mean(0) for i in range(n)]) + U * (Pi + 2) * torch.stack([a(d[oo[i]:oo[i + 1]]).mean(0) for i in range(n)])
                dh = dm @ a(W1).T + U * (C + 8) * (a(m) @ a(W1).T + a(b1))
                ds = HSIG_SLOPE * (dh @ a(W2).T + U * (C // 4 + 8) * (a(h) @ a(W2).T + a(b2))) + 4 * U
                dz = dd * s[img] + a(d) * ds[img] + U * a(z)
                c.regions = (int((t <= 0).sum()), int(((t > 0) & (t < 1)).sum()), int((t >= 1).sum()))
                assert min(c.regions) > 0, "%s: the hard-sigmoid's regions %s" % (c.name, c.regions)
            so.fill(slice(0, n), C, N(s), None if ds is None else N(ds))
            outs.append(so)
        zz = z * s[img] if (mut == "scale_twice" and c.se) else z
        yv = act_fn(zz @ Wp.T + bp, ACT_HSWISH) * LAB_PW[0] + LAB_PW[1]
        yb = None
        if ref:
            yb = N(1.5 * abs(LAB_PW[0]) * (dz @ a(Wp).T + U * (C + 8) * (a(z) @ a(Wp).T + a(bp))) + 4 * U * a(yv))
        yo = Out("y", P, c.ldy).fill(slice(0, P), c.cout, N(yv), yb)
        in_place = c.scaled == "place" or (mut == "scale_twice" and c.se)
        y1 = Out("y1", P, Cp)
        y1.mask[:P] = True
        y1.zero[:P, C:] = True
        y1.fill(slice(0, P), C, N(z if in_place else d), None if not ref else N(dz if in_place else dd))
        return [yo, y1] + outs


# ----------------------------------------------------------------------------------------------------------------------------
# the cases
def in_dims(outs, sh, sw):
    """input images that give these output images: every other one odd in the strided dimension"""
    return [(ho * sh - (i % 2 if sh == 2 else 0), wo * sw - ((i + 1) % 2 if sw == 2 else 0)) for i, (ho, wo) in enumerate(outs)]


def ragged_outs(maxHo):
    """output images of a launch whose largest has maxHo rows: widths 33 / 68 (17 strips of 4 pixels) / 7 (the last strip partial),
    a 1-pixel column and a 1 x 1 image; a last row strip that is partial, an image shorter than a strip, a 1-row image; for the
    pooled layout images below one block of strips and one of several.  Five images: the row kernel's (strip block, image) grid is
    a multiple of 8 only where a case asks for it (X8 below).  A 6-row batch (3-row strips) holds a wide 4-row image: the only
    height at which ceil(H / 3) != ceil(H / 4), so the only image whose strips, blocks and partial-sum slots depend on R being the
    3 the plan says (strips_mutant above; a 4 x 68 image is an ordinary member of a 6-row batch at the detector's coarsest level)."""
    if maxHo >= 10:
        return [(maxHo, 33), (maxHo - 1, 7), (1, 100), (2, 1), (1, 1)]
    if maxHo == 6:
        return [(6, 33), (4, 68), (1, 7), (2, 1), (1, 1)]
    return [(maxHo, 68), (max(1, maxHo - 1), 33), (1, 7), (min(2, maxHo), 1), (1, 1)]


X8 = [(2, 5), (1, 3), (3, 9)]   # three more small images: 8 in all, so that k_dwconv_rows takes its XCD remap


HS = (ACT_HSWISH, LAB_DW)
PLAIN = (ACT_NONE, None)
# id, K, C, (sh, sw), tail, pooled forms, maxHo values, "x8": also as a batch of 8 images
_DW_LAYERS = [
    ("det-s4.1", 3, 96, (1, 1), HS, (0,), (30,), True),
    ("det-s5.0", 3, 96, (2, 2), PLAIN, (0,), (6, 10), False),
    ("det-s5.x", 5, 192, (1, 1), HS, (0,), (4, 6, 12, 30), True),
    ("det-s6.0", 5, 192, (2, 2), PLAIN, (0, 1), (6, 5), True),
    ("det-s6.1", 5, 384, (1, 1), HS, (0, 1), (3, 6, 10), False),
    ("rec-s4.1", 3, 128, (1, 1), HS, (0,), (12,), False),
    ("rec-s5.0", 3, 128, (1, 2), HS, (0,), (12,), False),
    ("rec-s5.1", 5, 240, (1, 1), HS, (0,), (12,), False),
    ("rec-s6.0", 5, 240, (2, 1), HS, (0, 1), (6,), False),
    ("rec-s6.1", 5, 480, (1, 1), HS, (0, 1), (6,), False),
    ("rec-s6.2", 5, 480, (2, 1), HS, (0,), (3,), False),
    ("rec-s6.3", 5, 480, (1, 1), HS, (0,), (3,), False),
]


def _dw_cases():
    cs, seed = {}, 1000
    for lid, K, C, (sh, sw), (act, lab), pools, heights, x8 in _DW_LAYERS:
        for maxHo in heights:
            for pooled in pools:
                outs = ragged_outs(maxHo)
                batches = [("", outs)]
                if x8 and (maxHo == max(heights) or pooled):
                    batches.append(("-x8", outs + [(min(h, maxHo), w) for h, w in X8]))
                for suffix, ob in batches:
                    imgs = in_dims(ob, sh, sw)
                    forms = (1, 0) if dw_plan(K, sh, sw, chan_pitch(C), maxHo, max(w for _, w in ob), pooled, 1)[0] == SWEEP else (1,)
                    seed += 1            # (a sweep case and its row-kernel twin share their operands)
                    for form in forms:
                        cid = "%s-h%d%s%s%s" % (lid, maxHo, "-pool" if pooled else "", suffix, "" if form else "-rows")
                        cs[cid] = lambda cid=cid, K=K, C=C, sh=sh, sw=sw, act=act, lab=lab, pooled=pooled, form=form, imgs=imgs, seed=seed: Dw(
                            cid, K, C, sh, sw, act, lab, pooled, form, imgs, seed)
    return cs


# the 13 distinct wide block shapes of DET_SPEC / REC_SPEC (nets.h): id, K, cin, cout, (sh, sw), se, output images of the small batch
_DET_OUTS = [(9, 13), (5, 7), (1, 30), (3, 1)]
_REC = lambda h: [(h, 33), (h, 7), (h, 100), (h, 1)]   # noqa: E731  (the lines of a rec batch share their height)
_BLOCKS = [
    ("det-s4.1", 3, 96, 96, (1, 1), False, _DET_OUTS), ("det-s5.0", 3, 96, 192, (2, 2), False, _DET_OUTS),
    ("det-s5.1", 5, 192, 192, (1, 1), False, _DET_OUTS), ("det-s6.0", 5, 192, 384, (2, 2), True, _DET_OUTS),
    ("det-s6.1", 5, 384, 384, (1, 1), True, _DET_OUTS), ("det-s6.2", 5, 384, 384, (1, 1), False, _DET_OUTS),
    ("rec-s4.1", 3, 128, 128, (1, 1), False, _REC(12)), ("rec-s5.0", 3, 128, 240, (1, 2), False, _REC(12)),
    ("rec-s5.1", 5, 240, 240, (1, 1), False, _REC(12)), ("rec-s6.0", 5, 240, 480, (2, 1), True, _REC(6)),
    ("rec-s6.1", 5, 480, 480, (1, 1), True, _REC(6)), ("rec-s6.2", 5, 480, 480, (2, 1), False, _REC(3)),
    ("rec-s6.3", 5, 480, 480, (1, 1), False, _REC(3)),
]
# Rows from which gemm_plan() takes each folded form under the default switches: found with the plan driver by
# tests/test_dw_kernel_checks_cpu.py (a scan over M), asserted there against these, and on the GPU from info_out.  They are
# literals here because the case table is built at import, where neither the plan driver (compiled per test session) nor a
# device exists; the price: under a switch that moves them (RT_GEMM_MID=0 moves the 128 x 240 one) the plan test and the GPU
# -fold240 cases FAIL, naming the form the plan took instead, where a derived table would have followed the plan.
FOLD_M = {"wide_128x128": 8192, "wide_128x240": 32641}


def fold_outs(net, M, small=None):
    """output images of a folded batch of at least M rows: neighbours of 128 .. 140 pixels (a 128-row tile spans two images), then
    one large image; small: one more image of that many pixels in front (below 128: the fold is refused)"""
    if net == "det":
        outs = [(11, 12), (10, 13), (12, 11), (13, 10)]
        rest = M - sum(h * w for h, w in outs)
        h = 71
        outs.append((h, (rest + h - 1) // h))
    else:
        outs = [(6, 22), (6, 23), (4, 34), (6, 23)]   # (the 4-row line: strips_mutant above)
        rest = M - sum(h * w for h, w in outs)
        outs.append((6, (rest + 5) // 6))
    return ([small] if small else []) + outs


def _block_cases():
    cs, seed = {}, 2000
    for bid, K, cin, cout, (sh, sw), se, outs in _BLOCKS:
        imgs = in_dims(outs, sh, sw)
        swept = dw_plan(K, sh, sw, chan_pitch(cin), max(h for h, _ in outs), max(w for _, w in outs), False, 1)[0] == SWEEP
        seed += 1
        for form in ((1, 0) if swept else (1,)):
            cid = "%s%s" % (bid, "" if form else "-rows")
            cs[cid] = lambda cid=cid, K=K, cin=cin, cout=cout, sh=sh, sw=sw, se=se, form=form, imgs=imgs, seed=seed: Lc(
                cid, K, cin, cout, sh, sw, se, form, imgs, "place" if se else None, seed)
        if not se:
            continue
        net = bid[:3]
        folds = [("fold128", FOLD_M["wide_128x128"], None, "fold")] + ([("fold240", FOLD_M["wide_128x240"], None, "fold")] if cout % 240 == 0 else [])
        if bid in ("det-s6.1", "rec-s6.0"):
            folds.append(("minpix", FOLD_M["wide_128x128"], (9, 14) if net == "det" else (6, 21), "place"))   # one image of 126 pixels
        for tag, M, small, scaled in folds:
            fo = fold_outs(net, M, small)
            fi = in_dims(fo, sh, sw)
            seed += 1
            for form in ((1, 0) if (net == "rec" and scaled == "fold") else (1,)):   # (the det folds are too tall for a sweep)
                cid = "%s-%s%s" % (bid, tag, "" if form else "-rows")
                cs[cid] = lambda cid=cid, K=K, cin=cin, cout=cout, sh=sh, sw=sw, form=form, fi=fi, scaled=scaled, seed=seed: Lc(
                    cid, K, cin, cout, sh, sw, True, form, fi, scaled, seed)
    return cs


_MAKERS = {}
_MAKERS.update(_dw_cases())
DW_IDS = list(_MAKERS)
_MAKERS.update({"blk-" + k: v for k, v in _block_cases().items()})
CASE_IDS = list(_MAKERS)
BLOCK_IDS = [i for i in CASE_IDS if i.startswith("blk-")]
# a case that runs the sweep and its twin on the row kernel: the same operands, bit-identical results
TWINS = [(i, i + "-rows") for i in CASE_IDS if i + "-rows" in _MAKERS]


@functools.lru_cache(maxsize=3)
def case(case_id):
    return _MAKERS[case_id]()


# mutant -> the cases it is tried on (at least one must refuse it)
MUTANTS = {
    "tap_dropped_strip_end": ["det-s4.1-h30", "rec-s5.1-h12"], "taps_transposed": ["det-s5.x-h12", "rec-s4.1-h12"],
    "stride_swapped": ["rec-s5.0-h12", "rec-s6.2-h3"], "row_below_next_image": ["det-s5.x-h4", "rec-s6.3-h3"],
    "col_right_wraps": ["det-s4.1-h30", "rec-s6.0-h6"], "bias_after_act": ["det-s5.x-h30", "rec-s4.1-h12"],
    "lab_before_act": ["det-s6.1-h10", "rec-s5.0-h12"], "pad_passthrough": ["rec-s5.1-h12", "rec-s6.0-h6-pool"],
    "last_strip_unwritten": ["det-s5.x-h30", "det-s6.0-h5"], "pool_row_major": ["det-s6.0-h5-pool", "rec-s6.1-h6-pool"],
    "pool_foreign_block": ["det-s6.1-h10-pool", "det-s6.0-h6-pool"], "mean_div_max": ["det-s6.1-h3-pool", "rec-s6.0-h6-pool"],
    "pool_unremapped": ["det-s6.0-h6-pool-x8", "det-s6.0-h5-pool-x8"],
    "strips_r4": ["det-s6.0-h6-pool", "det-s6.1-h6-pool-rows", "blk-rec-s6.1-fold128-rows"],
    "se_fc_strip_r4": ["det-s6.0-h6-pool", "rec-s6.1-h6-pool", "blk-rec-s6.0-fold128"],
    "scale_prev_image": ["blk-det-s6.0-fold128", "blk-rec-s6.1"], "hsig_slope_02": ["blk-det-s6.1", "blk-rec-s6.0"],
    "row_table_equal_images": ["blk-det-s6.1-fold128", "blk-rec-s6.0-fold128"], "scale_twice": ["blk-det-s6.0-fold128", "blk-rec-s6.1"],
}
