"""fp64 references, float32 stand-ins, numpy mutants and the check function for the kernels of the fp32 detector's neck and head
that rt_debug_fpn drives (tests/test_gpu_fpn_kernels.py on the GPU, tests/test_fpn_kernel_checks_cpu.py here).  Plain numpy, no
device.

A Case holds the host arrays exactly as rt_debug_fpn takes them and `compute(dtype, mut=None, form="plain")`: the operation on
those arrays in `dtype` arithmetic, returning one Out per output buffer.  dtype = float64 with form = "plain" is the reference: the
plain mathematics on the MATERIALISED tensor (nearest-neighbour upsample, multiply by the per-image scales, concatenate, lateral
1x1 and its squeeze-excite factor, then a zero-padded 3x3 conv), never the restructured form.  float32 / "plain" is the stand-in
of the rms rule.  form = "kernel" is the kernels' own form in numpy (pre-summed phase / class weights, per-image composed weights,
gathers by class and parity): it is what the mutants are applied to, and the CPU test proves that in float32 it passes every
check and stays within twice the plain float32 form's rms error.

Bounds.  The suite's stage bound for one accumulation stage is  U (T + 8) S L + 4 U |y|  with U = 2^-24, T the summed terms, S =
sum |w| |x| + |bias| over the plain form's products and L the Lipschitz factor of what follows (1 throughout: ReLU, the clamps of
the hard-sigmoid).  Every bound here is built from it; nothing is fitted to what a kernel returned.
  pre-summed weights   a phase / class weight is the float32 rounding of an exact sum of at most 9 raw weights: relative error
                       <= U / 2 per product, at most U S over the sum.  T stays the plain form's term count: the kernel sums
                       fewer terms than the plain form, never more.
  scale multiply       x * s is rounded once before it meets the weight: another U S.  So a conv with n such extras is bounded
                       by U (T + 8 + n) S + 4 U |y| (n = 2 for every phase / class / fused-head conv: pre-sum and scale).
  head chain           class(p5) -> class(p4) -> phase is ONE running sum: the class tensors are stored unrounded fp32
                       accumulators, the next kernel continues from them.  96 + 96 + 96 + 216 products and 3 adds are fewer than
                       the plain 864 + 1: the single stage bound with T = 865 holds for the chain as for the fused launch.
  compose -> phase     a composed weight W'[tap][n][c] = sum_m Wlat[c][m] s[m] Wm[tap][n][m] is a product rounded once
                       (Wlat * s) and a 96-term fp32 fma chain: |dW'| <= U (96 + 2) sum_m |Wlat s Wm| =: E.  It reaches the
                       output through |x|: + sum_{tap, c} |x| E, added to the phase launch's own stage bound computed with the
                       exact W' (as the thin-block test composes its two stages).  Where the scales themselves come from a
                       measured table with error ds, E grows by sum_m |Wlat| ds[m] |Wm|.
  pool sums            a tile's channel sum adds <= 256 stored outputs in fp32: sum of the elements' own bounds (the summands
                       are the kernel's outputs, not the reference's) + U (256 + 8) sum |y| + 4 U |sum|.
  squeeze-excite       mean: a P-term sum (P pixels, or tiles) and one multiply: dm = U (P + 8) mean|x|.  Projection (cin
                       terms), fc1, ReLU, fc2 are stages of their own, each adding U (T + 8) S to the |w|-weighted error of
                       its input; the hard-sigmoid multiplies by its slope, and fma, two clamps and the + 1 are within 4 U |y|.
  tail                 deconv1 (24 terms + bias) -> ReLU -> deconv2 (24 terms + bias) gives the logit v with
                       A = sum |w2| (U (25 + 8) S1 + 4 U |h|) + U (25 + 8) S2 + 4 U |v|;  |err| <= y (1 - y) A + c U y with y the
                       sigmoid and c = |v| + 8: what exp2(v log2 e) with a 1-ulp v_exp_f32, one add and one reciprocal allow
                       (tests/f16_kernel_ref.py derives it), used at fraction 1.
  glue                 lateral_add is a cin-term stage, one multiply by s and one add: U (cin + 8 + 1) S + 4 U |y|, S =
                       sum |x| |Wlat| |s| + |b|.  upsample_add is a multiply and an add: 4 U |y| + U |a s|.
No element of any returned buffer is left out: outside an Out's mask every word must still be RT_DEBUG_CANARY (the 64 spare rows,
the pool tiles an image does not have), `zero` elements must be +0 (the composed weights' pad columns), and for an in-place op
the mask covers the whole operand."""
import functools

import numpy as np

U = 2.0 ** -24
CANARY = 0x7FA5C3E1   # RT_DEBUG_CANARY (as a float32: a NaN)
HSIG_MBV3 = 0.2       # slope of the det FPN's hard-sigmoid, F.hardsigmoid(slope=0.2, offset=0.5); its RSE layers add 1
POOL_PIX = 128        # pixels per chunk of the first stage of the squeeze-excite mean (nn_kernels.hip)
OPS = ["phase", "class", "compose", "tail", "lateral_add", "upsample_add", "se_projected", "se_tiles", "head_fused", "conv3"]
F_BIAS, F_POOL, F_RELU, F_G, F_FS, F_CS, F_COMPOSE = 1, 2, 4, 8, 16, 32, 64
INSTANCE_NAMES = {340: "k_fpn_phase<3, 4, 0>", 540: "k_fpn_phase<5, 4, 0>", 611: "k_fpn_phase<6, 1, 1>", 610: "k_fpn_phase<6, 1, 0>"}

BATCH_A = [(40, 24), (8, 8), (16, 16), (24, 56)]      # partial tiles in both axes, below a tile, an exact tile, several tiles
BATCH_B = [(4, 4), (12, 20), (36, 20), (16, 32)]
BATCH_HEAD = BATCH_A + [(72, 64)]


def half(imgs, n=1):
    for _ in range(n):
        assert all(h % 2 == 0 and w % 2 == 0 for h, w in imgs)
        imgs = [(h // 2, w // 2) for h, w in imgs]
    return imgs


def offsets(imgs):
    return [int(v) for v in np.concatenate([[0], np.cumsum([h * w for h, w in imgs])])]


def pixels(imgs):
    return offsets(imgs)[-1]


def tiles_alloc(imgs):
    return ((max(w for _, w in imgs) + 15) // 16) * ((max(h for h, _ in imgs) + 15) // 16)


def uni(rng, shape, scale=1.0):
    """uniform(-1, 1) float32 with full significands"""
    return (rng.uniform(-1, 1, shape) * scale).astype(np.float32)


def conv_w(rng, cin=96):
    return uni(rng, (24, cin, 3, 3), 4 / np.sqrt(cin * 9))


def scales(rng, n, c):
    return rng.uniform(0.5, 1.5, (n, c)).astype(np.float32)


def split(buf, imgs, c):
    """a level's buffer [pixels][c] as per-image [H][W][c] views"""
    o = offsets(imgs)
    b = np.asarray(buf).reshape(-1, c)
    return [b[o[i]:o[i + 1]].reshape(h, w, c) for i, (h, w) in enumerate(imgs)]


def up(z, s):
    return np.repeat(np.repeat(z, s, axis=0), s, axis=1)


def conv3(x, w, dtype):
    """zero-padded 3x3 conv: x [H][W][C], w [N][C][3][3] -> [H][W][N] in dtype arithmetic"""
    H, W, C = x.shape
    pad = np.zeros((H + 2, W + 2, C), dtype)
    pad[1:-1, 1:-1] = x
    acc = np.zeros((H, W, w.shape[0]), dtype)
    for dy in range(3):
        for dx in range(3):
            acc += pad[dy:dy + H, dx:dx + W] @ np.ascontiguousarray(w[:, :, dy, dx].T).astype(dtype)
    return acc


def conv3_abs(x, w):
    return conv3(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.float64)


class Out:
    """one output buffer [(rows + spare)][ld]: mask = what the kernel must write, v its values, bound the element bound (None: exact
    bits of v as float32), zero = elements that must be +0"""

    def __init__(self, rows, ld, spare=64):
        self.shape = (rows + spare, ld)
        self.mask = np.zeros(self.shape, bool)
        self.v = None
        self.bound = np.zeros(self.shape)
        self.zero = np.zeros(self.shape, bool)
        self.base = None          # the buffer before the launch (in place), else the canary
        self.kind = "arith"
        self.slot = 0             # which of rt_debug_fpn's out[3] it is

    def put(self, dtype):
        self.v = np.zeros(self.shape, dtype)
        return self


class Case:
    fine = coarse = None
    fp = (0.0,)
    info = 0

    def args(self):
        """(op, ip, fp, fine, coarse, ins[10]) for rt_debug_fpn"""
        ins = list(self.ins) + [None] * (10 - len(self.ins))
        return OPS.index(self.op), list(self.ip), list(self.fp), self.fine, self.coarse or self.fine, ins

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return self.compute(np.float64)

    def buffers(self, dtype=np.float32, mut=None, form="plain"):
        """what a kernel computing in dtype would return: float32 buffers, canary outside the masks"""
        res = []
        for o in self.compute(dtype, mut, form):
            b = np.full(o.shape, CANARY, np.uint32)
            if o.base is not None:
                b[:] = np.asarray(o.base, np.float32).view(np.uint32)
            with np.errstate(invalid="ignore", over="ignore"):
                b[o.mask] = o.v[o.mask].astype(np.float32).view(np.uint32)
            res.append(b.view(np.float32))
        return res


def check(case, outs, f32=None):
    """asserts everything the suite asks of one launch's outputs (float32 buffers as returned) and returns the measured figures"""
    refs = case.reference()
    if f32 is None:
        f32 = case.buffers(np.float32)
    assert len(outs) == len(refs)
    fig = {"n": 0, "worst": 0.0}
    for k, (o, got, s32) in enumerate(zip(refs, outs, f32)):
        got = np.asarray(got, np.float32).reshape(o.shape)
        bits = got.view(np.uint32)
        base = np.full(o.shape, CANARY, np.uint32) if o.base is None else np.asarray(o.base, np.float32).reshape(o.shape).view(np.uint32)
        assert o.mask[:o.shape[0] - 64].any() and not o.mask[-64:].any()
        same = bits[~o.mask] == base[~o.mask]
        assert same.all(), "%s out %d: %d elements outside the op's output were changed (first at flat index %d)" % (
            case.name, k, int((~same).sum()), int(np.flatnonzero(~o.mask)[np.argmin(same)]))
        assert (bits[o.zero] == 0).all(), "%s out %d: %d pad elements are not +0" % (case.name, k, int((bits[o.zero] != 0).sum()))
        m = o.mask & ~o.zero
        g, r, b = got[m].astype(np.float64), o.v[m], o.bound[m]
        fig["n"] += int(o.mask.sum())
        assert np.isfinite(g).all(), "%s out %d: non-finite output" % (case.name, k)
        if not g.size:
            continue
        err = np.abs(g - r)
        if o.kind == "exact":
            assert np.array_equal(g.astype(np.float32).view(np.uint32), r.astype(np.float32).view(np.uint32)), "%s out %d: bits differ" % (case.name, k)
            continue
        assert (b > 0).all()
        w = int(np.argmax(err / b))
        fig["worst"] = max(fig["worst"], float(err[w] / b[w]))
        assert (err <= b).all(), "%s out %d: %d of %d elements outside the bound, worst err %.3e bound %.3e (ref %.6g got %.6g)" % (
            case.name, k, int((err > b).sum()), err.size, err[w], b[w], r[w], g[w])
        if o.kind == "sigmoid":   # (no rms rule: the bound allows __expf more than a libm float32 sigmoid needs)
            continue
        # the rms rule, per output buffer: a launch's conv output, its pool sums and its composed weights each stand alone (pooled
        # over them the 256-term tile sums' error, 75 x the conv output's in squares, would hide the conv's)
        rms = float(np.sqrt(np.mean(err ** 2)))
        rms32 = float(np.sqrt(np.mean((np.asarray(s32, np.float32).reshape(o.shape)[m].astype(np.float64) - r) ** 2)))
        fig["rms%d" % o.slot], fig["rms32_%d" % o.slot] = rms, rms32
        fig["ratio%d" % o.slot] = rms / rms32 if rms32 else 0.0
        assert rms <= 2 * rms32, "%s out %d: rms error %.3e is %.2f x the float32 stand-in's %.3e" % (case.name, k, rms, rms / rms32, rms32)
    return fig


# ----------------------------------------------------------------------------------------------------------------------------
# the kernels' form in numpy: what nets.cpp's packers and nn_fpn.hip do, restated for the stand-in and the mutants
def phase_taps(ph, t, mut=None):
    """taps of the 3-tap axis that land on tap t of the 2-tap phase axis"""
    if ph == 0:
        return [0] if t == 0 else [1, 2]
    if mut == "phase_taps_swapped":
        return [2] if t == 0 else [0, 1]
    return [0, 1] if t == 0 else [2]


def phase_weights(w, dtype, mut=None):
    """[py][px][ty][tx][N][C] pre-summed weights of conv3x3(up2(z)), rounded to float32 as the packer stores them"""
    o = np.zeros((2, 2, 2, 2) + w.shape[:2])
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    for dy in phase_taps(py, ty, mut):
                        for dx in phase_taps(px, tx, mut):
                            o[py, px, ty, tx] += w[:, :, dy, dx].astype(np.float64)
    return o.astype(np.float32).astype(dtype)


def phase_conv(z, w, dtype, mut=None):
    """conv3x3(up2(z)) as four 2 x 2 convs of z: z [h][w][C] -> [2h][2w][N]"""
    h, ww, C = z.shape
    pw = phase_weights(w, dtype, mut)
    pad = np.zeros((h + 2, ww + 2, C), dtype)
    pad[1:-1, 1:-1] = z
    out = np.zeros((2 * h, 2 * ww, w.shape[0]), dtype)
    for py in range(2):
        for px in range(2):
            wy, wx = (px, py) if mut == "phase_pxpy" else (py, px)
            acc = np.zeros((h, ww, w.shape[0]), dtype)
            for ty in range(2):
                for tx in range(2):   # coarse pixel (Y + py + ty - 1, X + px + tx - 1)
                    acc += pad[py + ty:py + ty + h, px + tx:px + tx + ww] @ pw[wy, wx, ty, tx].T
            out[py::2, px::2] = acc
    return out


CLS_POS = (0, 1, 3)   # a first / interior / last row of a block of 4


def class_span(cls, r):
    """taps of the 3-tap axis that land on relative row r of z for row class cls"""
    return {(0, -1): [0], (0, 0): [1, 2], (1, 0): [0, 1, 2], (2, 0): [0, 1], (2, 1): [2]}.get((cls, r), [])


def class_form(z, w, dtype):
    """[9][h][w][N]: the class tensor by pre-summed weights"""
    h, ww, C = z.shape
    pad = np.zeros((h + 2, ww + 2, C), dtype)
    pad[1:-1, 1:-1] = z
    V = np.zeros((9, h, ww, w.shape[0]), dtype)
    for rc in range(3):
        for cc in range(3):
            for ry in (-1, 0, 1):
                for rx in (-1, 0, 1):
                    ys, xs = class_span(rc, ry), class_span(cc, rx)
                    if ys and xs:
                        wsum = sum(w[:, :, dy, dx].astype(np.float64) for dy in ys for dx in xs).astype(np.float32).astype(dtype)
                        V[rc * 3 + cc] += pad[1 + ry:1 + ry + h, 1 + rx:1 + rx + ww] @ wsum.T
    return V


def class_plain(z, w, dtype):
    """[9][h][w][N]: the value a 3x3 conv over up4(z) takes at the first / interior / last row and column of each block"""
    full = conv3(up(z, 4), w.astype(dtype), dtype)
    return np.stack([full[CLS_POS[rc]::4, CLS_POS[cc]::4] for rc in range(3) for cc in range(3)])


def lower_class(rc, y):
    """row class, in the next coarser level's blocks of 8, of full-resolution row 4 y + CLS_POS[rc]"""
    pos = 4 * (y & 1) + CLS_POS[rc]
    return 0 if pos == 0 else 2 if pos == 7 else 1


def cls4(r):
    return 0 if r == 0 else 2 if r == 3 else 1


# ----------------------------------------------------------------------------------------------------------------------------
class Phase(Case):
    """nn::fpn_phase.  cin = 24: the head conv (p2 fine, p3 coarse, G for p4 / p5 or a bias); cin < 24: an inp conv over the tap
    tensor with per-image weights Wf, given or composed from (lat, lat_scale) in the same call."""
    op = "phase"

    def __init__(self, name, cin, fine, flags, seed, **over):
        rng = np.random.default_rng(seed)
        self.name, self.cin, self.cf, self.fine, self.coarse, self.flags = name, cin, (cin + 3) // 4 * 4, fine, half(fine), flags
        self.head = cin == 24
        self.cc = 24 if self.head else 96
        self.info = {12: 340, 18: 540, 24: 611 if flags & F_G else 610}[cin]
        n, pf, pc = len(fine), pixels(fine), pixels(self.coarse)
        self.ip = [cin, self.cc, flags]
        self.x = uni(rng, (pf, self.cf))          # (pad channels cin .. cf hold finite noise)
        self.z = uni(rng, (pc, self.cc))
        self.w = conv_w(rng)
        self.bias = uni(rng, 24)
        self.lat = uni(rng, (96, cin), 4 / np.sqrt(cin)) if not self.head else None
        self.lat_scale = (1 + rng.uniform(0, 1, (n, 96))).astype(np.float32) if flags & F_COMPOSE else None
        self.lat_scale_ref = self.lat_scale_err = None   # chains: the fp64 scale table and the bound of the given one's error
        self.wf = None
        if not self.head and not flags & F_COMPOSE:
            self.wf = np.zeros((n, 9, 24, self.cf), np.float32)
            self.wf[..., :cin] = uni(rng, (n, 9, 24, cin), 4 / np.sqrt(9 * cin))
        self.fs = scales(rng, n, 24) if flags & F_FS else None
        self.cs = scales(rng, n, 24) if flags & F_CS else None
        self.G = None
        if flags & F_G and "G" not in over:   # the class tensor of two coarser levels, built in fp64 and rounded
            q = half(fine, 2)
            c4 = ClassOp("G", q, 7, seed + 1, w=self.w, bias=self.bias)
            self.G = c4.compute(np.float64)[0].v[:9 * pixels(q)].astype(np.float32)
        self.__dict__.update(over)

    @property
    def ins(self):
        fl = self.flags
        return [self.x, self.z, self.w, self.bias if fl & F_BIAS else None, self.wf, self.lat if fl & F_COMPOSE else None,
                self.lat_scale, self.fs, self.cs, self.G]

    def with_noise(self, seed):
        """the tap tensor with other finite values in its pad channels"""
        x = self.x.copy()
        x[:, self.cin:] = uni(np.random.default_rng(seed), (x.shape[0], self.cf - self.cin), 8.0)
        return x

    def composed(self, dtype, mut=None):
        """W'[img][tap][n][cf] = sum_m lat[m][c] s[img][m] w[n][m][tap], pad columns zero (k_fpn_compose) and its error bound E"""
        n = len(self.fine)
        s = self.lat_scale.astype(dtype) if dtype != np.float64 or self.lat_scale_ref is None else self.lat_scale_ref
        if mut == "compose_no_se":
            s = np.ones_like(s)
        wm = self.w.reshape(24, 96, 9).transpose(2, 0, 1).astype(dtype)     # [tap][n][m]
        ls = self.lat.T.astype(dtype)[None] * s[:, None, :]                  # [img][c][m]
        out = np.zeros((n, 9, 24, self.cf), dtype)
        out[..., :self.cin] = np.einsum("icm,tnm->itnc", ls, wm)
        if mut == "compose_pad_nonzero":
            out[..., self.cin:] = out[..., :self.cf - self.cin]
        a = np.abs(self.lat.T.astype(np.float64))[None] * np.abs(self.lat_scale.astype(np.float64))[:, None, :]
        E = np.zeros((n, 9, 24, self.cf))
        E[..., :self.cin] = U * 98 * np.einsum("icm,tnm->itnc", a, np.abs(wm.astype(np.float64)))
        if self.lat_scale_err is not None:
            d = np.abs(self.lat.T.astype(np.float64))[None] * self.lat_scale_err[:, None, :]
            E[..., :self.cin] += np.einsum("icm,tnm->itnc", d, np.abs(wm.astype(np.float64)))
        return out, E

    def compute(self, dtype, mut=None, form="plain"):
        n, cin, fl = len(self.fine), self.cin, self.flags
        pf = pixels(self.fine)
        y = Out(pf, 24).put(dtype)
        outs = [y]
        pool = None
        tiles = tiles_alloc(self.fine)
        if fl & F_POOL:
            pool = Out(n * tiles, 24).put(dtype)
            pool.slot = 1
            outs.append(pool)
        wf, E = (self.composed(dtype, mut) if fl & F_COMPOSE else (None if self.head else self.wf.astype(dtype), None))
        if fl & F_COMPOSE:
            comp = Out(n * 216, self.cf).put(dtype)
            comp.slot = 2
            comp.v[:n * 216] = wf.reshape(n * 216, self.cf)
            comp.mask[:n * 216] = True
            comp.zero[:n * 216, cin:] = True
            comp.bound[:n * 216] = E.reshape(n * 216, self.cf) + 4 * U * np.abs(comp.v[:n * 216].astype(np.float64)) + 1e-300
            outs.append(comp)
        xs, zs = split(self.x, self.fine, self.cf), split(self.z, self.coarse, self.cc)
        w = self.w
        Gs = None
        if fl & F_G:
            q = half(self.fine, 2)
            Gs = [np.stack(v) for v in zip(*[split(self.G[k * pixels(q):(k + 1) * pixels(q)], q, 24) for k in range(9)])]
        off = offsets(self.fine)
        for i, (H, W) in enumerate(self.fine):
            x = xs[i][..., :cin].astype(dtype)
            z = zs[i].astype(dtype)
            if self.fs is not None:
                x = x * self.fs[0 if mut == "fine_scale_img0" else i].astype(dtype)
            if self.cs is not None:
                z = z * self.cs[i].astype(dtype)
            if self.head:
                wfine, wco = w[:, 72:96], w[:, 48:72]
            else:
                j = 0 if mut == "wf_img0" else i
                wfine, wco = wf[j][..., :cin].transpose(1, 2, 0).reshape(24, cin, 3, 3), w
            acc = conv3(x, wfine.astype(dtype), dtype)
            acc += conv3(up(z, 2), wco.astype(dtype), dtype) if form == "plain" else phase_conv(z, wco, dtype, mut)
            S = conv3_abs(x, wfine) + conv3_abs(up(z, 2), wco)
            T, extra = 9 * cin + 9 * self.cc + 1, 2
            if E is not None:
                S_E = sum(np.abs(np.pad(x.astype(np.float64), ((1, 1), (1, 1), (0, 0))))[dy:dy + H, dx:dx + W] @ E[i, dy * 3 + dx, :, :cin].T
                          for dy in range(3) for dx in range(3))
            else:
                S_E = 0.0
            oy, ox = np.mgrid[0:H, 0:W]
            if fl & F_G:
                qy, qx = oy >> 2, ox >> 2
                ry, rx = oy & 3, ox & 3
                if mut == "quarter_index_off":
                    qy = np.minimum((oy + 1) >> 2, H // 4 - 1)
                rcl = np.where(ry == 0, 0, np.where(ry == 3, 1 if mut == "rowclass3_interior" else 2, 1))
                ccl = np.where(rx == 0, 0, np.where(rx == 3, 2, 1))
                g = Gs[i][rcl * 3 + ccl, qy, qx]
                acc += g.astype(dtype)
                S += np.abs(g.astype(np.float64))
                if mut == "bias_twice":
                    acc += self.bias.astype(dtype)
            if fl & F_BIAS:
                acc += self.bias.astype(dtype)
                S += np.abs(self.bias.astype(np.float64))
            if fl & F_RELU:
                acc = np.maximum(acc, 0)
            y.v[off[i]:off[i + 1]] = acc.reshape(-1, 24)
            y.mask[off[i]:off[i + 1]] = True
            bnd = U * (T + 8 + extra) * S + S_E + 4 * U * np.abs(acc.astype(np.float64))
            y.bound[off[i]:off[i + 1]] = bnd.reshape(-1, 24)
            if pool is not None:
                ty_n, tx_n = (H + 15) // 16, (W + 15) // 16
                for ty in range(ty_n):
                    for tx in range(tx_n):
                        t = acc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].reshape(-1, 24)
                        r = i * tiles + ty * tx_n + tx
                        pool.v[r] = t.sum(0)
                        if mut == "pool_premask":   # the tile's out-of-image lanes hold the epilogue's value of an all-zero window
                            pool.v[r] += (256 - t.shape[0]) * (self.bias.astype(dtype) if fl & F_BIAS else 0)
                        a = np.abs(t.astype(np.float64)).sum(0)
                        pool.bound[r] = bnd[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].reshape(-1, 24).sum(0) + U * (256 + 8) * a + 4 * U * np.abs(pool.v[r].astype(np.float64))
                        pool.mask[r] = True
        return outs


class ClassOp(Case):
    """nn::fpn_class: the class tensor of z for the head conv's channels [c0, c0 + 24), (+ bias) (+ the lower level's tensor at the
    class the pixel's place in the lower level's blocks implies).  flags: 1 bias, 2 scale, 4 lower"""
    op = "class"

    def __init__(self, name, imgs, flags, seed, w=None, bias=None, lower=None, z=None, scale=None, lower_scale=None):
        rng = np.random.default_rng(seed)
        self.name, self.fine, self.flags = name, imgs, flags
        self.coarse = half(imgs) if flags & 4 else None
        n = len(imgs)
        self.c0 = 24 if flags & 4 else 0
        self.ip = [self.c0, flags]
        self.z = uni(rng, (pixels(imgs), 24)) if z is None else z
        self.w = conv_w(rng) if w is None else w
        self.bias = uni(rng, 24) if bias is None else bias
        self.scale = (scales(rng, n, 24) if scale is None else scale) if flags & 2 else None
        self.lower = None
        if flags & 4:
            if lower is None:   # the level below, built in fp64 and rounded
                lo = ClassOp("lower", self.coarse, 2, seed + 1, w=self.w, scale=lower_scale)
                lower = lo.compute(np.float64)[0].v[:9 * pixels(self.coarse)].astype(np.float32)
                self.lower_case = lo
            self.lower = lower
        self.ins = [self.z, self.w, self.bias if flags & 1 else None, self.scale, self.lower]

    def compute(self, dtype, mut=None, form="plain"):
        P = pixels(self.fine)
        o = Out(9 * P, 24).put(dtype)
        w = self.w[:, self.c0:self.c0 + 24]
        off = offsets(self.fine)
        zs = split(self.z, self.fine, 24)
        if self.lower is not None:
            pl = pixels(self.coarse)
            lows = [np.stack(v) for v in zip(*[split(self.lower[k * pl:(k + 1) * pl], self.coarse, 24) for k in range(9)])]
        for i, (H, W) in enumerate(self.fine):
            z = zs[i].astype(dtype)
            if self.scale is not None:
                z = z * self.scale[i].astype(dtype)
            V = class_plain(z, w, dtype) if form == "plain" else class_form(z, w, dtype)
            S = class_plain(np.abs(z.astype(np.float64)), np.abs(w.astype(np.float64)), np.float64)
            if self.flags & 1:
                V += self.bias.astype(dtype)
                S += np.abs(self.bias.astype(np.float64))
            if self.lower is not None:
                yy, xx = np.mgrid[0:H, 0:W]
                for rc in range(3):
                    for cc in range(3):
                        lr = np.vectorize(lambda y: lower_class(rc, y))(yy)
                        lc = np.vectorize(lambda x: lower_class(cc, x))(xx)
                        if mut == "lower_parity_inverted":
                            lr = np.where((rc == 0) & (yy & 1 == 1), 0, np.where((rc == 2) & (yy & 1 == 0), 2, 1))
                            lc = np.where((cc == 0) & (xx & 1 == 1), 0, np.where((cc == 2) & (xx & 1 == 0), 2, 1))
                        ly, lx = yy >> 1, xx >> 1
                        if mut == "lower_at_yx":
                            ly, lx = np.minimum(yy, H // 2 - 1), np.minimum(xx, W // 2 - 1)
                        g = lows[i][lr * 3 + lc, ly, lx]
                        V[rc * 3 + cc] += g.astype(dtype)
                        S[rc * 3 + cc] += np.abs(g.astype(np.float64))
            for k in range(9):
                rows = slice(k * P + off[i], k * P + off[i + 1])
                o.v[rows] = V[k].reshape(-1, 24)
                o.mask[rows] = True
                o.bound[rows] = (U * (9 * 24 + 2 + 8 + 2) * S[k] + 4 * U * np.abs(V[k].astype(np.float64))).reshape(-1, 24)
        return [o]


class Compose(Phase):
    """nn::fpn_compose alone"""
    op = "compose"

    def __init__(self, name, cin, n, seed):
        Phase.__init__(self, name, cin, [(2, 2)] * n, F_COMPOSE, seed)
        self.coarse = None
        self.ip = [cin]
        self.info = 0

    @property
    def ins(self):
        return [self.lat, self.lat_scale, self.w]

    def compute(self, dtype, mut=None, form="plain"):
        n = len(self.fine)
        wf, E = self.composed(dtype, mut)
        o = Out(n * 216, self.cf).put(dtype)
        o.v[:n * 216] = wf.reshape(n * 216, self.cf)
        o.mask[:n * 216] = True
        o.zero[:n * 216, self.cin:] = True
        o.bound[:n * 216] = E.reshape(n * 216, self.cf) + 4 * U * np.abs(o.v[:n * 216].astype(np.float64)) + 1e-300
        return [o]


class Tail(Case):
    """nn::db_head_tail: convT 2x2 s2 24 -> 24, ReLU, convT 2x2 s2 24 -> 1, sigmoid; the map at four times the input's sides"""
    op = "tail"
    ip = [0]

    def __init__(self, name, imgs, seed):
        rng = np.random.default_rng(seed)
        self.name, self.fine = name, imgs
        self.x = uni(rng, (pixels(imgs), 24))
        self.w1, self.b1 = uni(rng, (24, 24, 2, 2), 4 / np.sqrt(24)), uni(rng, 24)
        self.w2, self.b2 = uni(rng, (24, 1, 2, 2), 1.1), uni(rng, 1)   # logits over about +-12
        self.ins = [self.x, self.w1, self.b1, self.w2, self.b2]

    def compute(self, dtype, mut=None, form="plain"):
        P = pixels(self.fine)
        o = Out(16 * P, 1, spare=1024).put(dtype)
        o.kind = "sigmoid"
        w1, w2 = self.w1.astype(dtype), self.w2.astype(dtype)
        if mut == "tail_dydx_transposed":
            w1 = w1.transpose(0, 1, 3, 2)
        x = self.x.astype(dtype)
        ax = np.abs(self.x.astype(np.float64))
        off, q = offsets(self.fine), 0
        self.logit_span = 0.0
        for i, (H, W) in enumerate(self.fine):
            xi, ai = x[off[i]:off[i + 1]], ax[off[i]:off[i + 1]]
            m = np.zeros((4 * H, 4 * W), dtype)
            A = np.zeros((4 * H, 4 * W))
            for d1y in range(2):
                for d1x in range(2):
                    h = xi @ w1[:, :, d1y, d1x] + self.b1.astype(dtype)
                    S1 = ai @ np.abs(self.w1[:, :, d1y, d1x].astype(np.float64)) + np.abs(self.b1.astype(np.float64))
                    dh = U * 33 * S1 + 4 * U * np.abs(h.astype(np.float64))
                    if mut != "tail_no_relu":
                        h = np.maximum(h, 0)
                    for d2y in range(2):
                        for d2x in range(2):
                            v = h @ w2[:, 0, d2y, d2x] + self.b2.astype(dtype)[0]
                            a2 = np.abs(self.w2[:, 0, d2y, d2x].astype(np.float64))
                            S2 = np.abs(h.astype(np.float64)) @ a2 + abs(float(self.b2[0]))
                            r, c = 2 * d1y + d2y, 2 * d1x + d2x
                            if mut == "tail_rows_swapped":
                                r = (r & 1) * 2 + (r >> 1)
                            m[r::4, c::4] = v.reshape(H, W)
                            A[r::4, c::4] = (dh @ a2 + U * 33 * S2 + 4 * U * np.abs(v.astype(np.float64))).reshape(H, W)
            v64 = m.astype(np.float64)
            self.logit_span = max(self.logit_span, float(np.abs(v64).max()))
            with np.errstate(over="ignore"):
                y = 1 / (1 + np.exp(-m))
                y64 = 1 / (1 + np.exp(-v64))
            rows = slice(q, q + 16 * H * W)
            o.v[rows, 0] = y.ravel()
            o.mask[rows] = True
            o.bound[rows, 0] = (y64 * (1 - y64) * A + (np.abs(v64) + 8) * U * y64).ravel()
            q += 16 * H * W
        return [o]


class LateralAdd(Case):
    """nn::lateral_add: out = (x . lat^T) * s + up2(b)"""
    op = "lateral_add"

    def __init__(self, name, cin, imgs, has_b, seed):
        rng = np.random.default_rng(seed)
        self.name, self.cin, self.cf, self.fine = name, cin, (cin + 3) // 4 * 4, imgs
        self.coarse = half(imgs) if has_b else None
        n = len(imgs)
        self.ip = [cin, int(has_b)]
        self.x = np.zeros((pixels(imgs), self.cf), np.float32)
        self.x[:, :cin] = uni(rng, (pixels(imgs), cin))
        self.lat = uni(rng, (96, cin), 4 / np.sqrt(cin))
        self.s = (1 + rng.uniform(0, 1, (n, 96))).astype(np.float32)
        self.b = uni(rng, (pixels(self.coarse), 96)) if has_b else None
        self.ins = [self.x, self.lat, self.s, self.b]

    def compute(self, dtype, mut=None, form="plain"):
        o = Out(pixels(self.fine), 96).put(dtype)
        off = offsets(self.fine)
        for i, (H, W) in enumerate(self.fine):
            x = self.x[off[i]:off[i + 1], :self.cin].astype(dtype)
            v = x @ self.lat.T.astype(dtype)
            S = np.abs(x.astype(np.float64)) @ np.abs(self.lat.T.astype(np.float64)) * np.abs(self.s[i].astype(np.float64))
            b = 0
            if self.b is not None:
                b = up(split(self.b, self.coarse, 96)[i], 2).reshape(-1, 96).astype(dtype)
                S = S + np.abs(b.astype(np.float64))
            v = (v + b) * self.s[i].astype(dtype) if mut == "lateral_scale_after_add" else v * self.s[i].astype(dtype) + b
            o.v[off[i]:off[i + 1]] = v
            o.mask[off[i]:off[i + 1]] = True
            o.bound[off[i]:off[i + 1]] = U * (self.cin + 9) * S + 4 * U * np.abs(v.astype(np.float64)) + 1e-300
        return [o]


class UpsampleAdd(Case):
    """nn::upsample_add: out = a * s + up2(b), in place on a or not"""
    op = "upsample_add"

    def __init__(self, name, imgs, in_place, has_s, seed):
        rng = np.random.default_rng(seed)
        self.name, self.fine, self.coarse, self.in_place = name, imgs, half(imgs), in_place
        self.ip = [int(in_place), int(has_s)]
        self.a, self.b = uni(rng, (pixels(imgs), 96)), uni(rng, (pixels(self.coarse), 96))
        self.s = scales(rng, len(imgs), 96) if has_s else None
        self.ins = [self.a, self.b, self.s]

    def compute(self, dtype, mut=None, form="plain"):
        P = pixels(self.fine)
        o = Out(P, 96).put(dtype)
        if self.in_place:
            o.base = np.full(o.shape, CANARY, np.uint32).view(np.float32)
            o.base[:P] = self.a
        off = offsets(self.fine)
        for i, (H, W) in enumerate(self.fine):
            a = self.a[off[i]:off[i + 1]].astype(dtype)
            if self.s is not None:
                a = a * self.s[i].astype(dtype)
            b = split(self.b, self.coarse, 96)[i]
            if mut == "upsample_yp1":
                yy = np.minimum((np.arange(H) + 1) >> 1, H // 2 - 1)
                bu = b[yy][:, np.arange(W) >> 1]
            else:
                bu = up(b, 2)
            v = a + bu.reshape(-1, 96).astype(dtype)
            o.v[off[i]:off[i + 1]] = v
            o.mask[off[i]:off[i + 1]] = True
            o.bound[off[i]:off[i + 1]] = 4 * U * np.abs(v.astype(np.float64)) + U * np.abs(a.astype(np.float64)) + 1e-300
        return [o]


def se_chain(mean, dmean, w1, b1, w2, b2, slope, residual, dtype):
    """fc1 -> relu -> fc2 -> hard-sigmoid (+ 1) of a mean [C] with error dmean: value in dtype and the bound of its error"""
    a = lambda v: np.abs(np.asarray(v, np.float64))   # noqa: E731
    C, Cr = w1.shape[1], w1.shape[0]
    h = w1.astype(dtype) @ mean + b1.astype(dtype)
    dh = a(w1) @ dmean + U * (C + 1 + 8) * (a(w1) @ a(mean) + a(b1)) + 4 * U * a(h)
    h = np.maximum(h, 0)
    t = w2.astype(dtype) @ h + b2.astype(dtype)
    dt = a(w2) @ dh + U * (Cr + 1 + 8) * (a(w2) @ a(h) + a(b2)) + 4 * U * a(t)
    y = np.clip(t * dtype(np.float32(slope)) + dtype(0.5), 0, 1) + (1 if residual else 0)
    return y, slope * dt + 4 * U * a(y) + 4 * U


class SeProjected(Case):
    """nn::se_scale_projected: mean over the pixels of the narrow tensor, through the lateral matrix, then the FCs"""
    op = "se_projected"

    def __init__(self, name, cin, imgs, seed, x=None, lat=None):
        rng = np.random.default_rng(seed)
        self.name, self.cin, self.cf, self.fine = name, cin, (cin + 3) // 4 * 4, imgs
        self.ip, self.fp = [cin, 24, 1], [HSIG_MBV3]
        self.x = np.zeros((pixels(imgs), self.cf), np.float32)
        self.x[:, :cin] = 0.5 + uni(rng, (pixels(imgs), cin))
        if x is not None:
            self.x = x
        self.lat = uni(rng, (96, cin), 4 / np.sqrt(cin)) if lat is None else lat
        self.w1, self.b1 = uni(rng, (24, 96), 4 / np.sqrt(96)), uni(rng, 24)
        self.w2, self.b2 = uni(rng, (96, 24), 4 / np.sqrt(24)), uni(rng, 96)
        self.ins = [self.x, self.lat, self.w1, self.b1, self.w2, self.b2]

    def compute(self, dtype, mut=None, form="plain"):
        n = len(self.fine)
        o = Out(n, 96).put(dtype)
        off = offsets(self.fine)
        for i in range(n):
            x = self.x[off[i]:off[i + 1], :self.cin]
            P = x.shape[0]
            m_in = x.astype(dtype).sum(0) / dtype(P)
            d_in = U * (P + 8) * np.abs(x.astype(np.float64)).sum(0) / P
            al = np.abs(self.lat.astype(np.float64))
            m = self.lat.astype(dtype) @ m_in
            dm = al @ d_in + U * (self.cin + 8) * (al @ np.abs(m_in.astype(np.float64))) + 4 * U * np.abs(m.astype(np.float64))
            o.v[i], o.bound[i] = se_chain(m, dm, self.w1, self.b1, self.w2, self.b2, HSIG_MBV3, 1, dtype)
            o.mask[i] = True
        return [o]


class SeTiles(Case):
    """nn::se_fc_from_tiles: the FCs from the per-tile channel sums k_fpn_phase leaves (canary where an image has no tile)"""
    op = "se_tiles"

    def __init__(self, name, imgs, seed, pool=None):
        rng = np.random.default_rng(seed)
        self.name, self.fine = name, imgs
        self.ip, self.fp = [6, 1], [HSIG_MBV3]
        n, T = len(imgs), tiles_alloc(imgs)
        if pool is None:
            pool = np.full((n, T, 24), CANARY, np.uint32).view(np.float32)
            for i, (H, W) in enumerate(imgs):
                k = ((H + 15) // 16) * ((W + 15) // 16)
                pool[i, :k] = uni(rng, (k, 24), 100.0) + 20
        self.pool = np.ascontiguousarray(pool, np.float32).reshape(n, T, 24)
        self.w1, self.b1 = uni(rng, (6, 24), 4 / np.sqrt(24)), uni(rng, 6)
        self.w2, self.b2 = uni(rng, (24, 6), 4 / np.sqrt(6)), uni(rng, 24)
        self.ins = [self.pool, self.w1, self.b1, self.w2, self.b2]
        self.ref_mean = self.ref_dmean = None   # chains: the fp64 channel means of the plain form and what the pool sums may add

    def compute(self, dtype, mut=None, form="plain"):
        n, T = len(self.fine), tiles_alloc(self.fine)
        o = Out(n, 24).put(dtype)
        for i, (H, W) in enumerate(self.fine):
            k = T if mut == "se_tiles_max_tiles" else ((H + 15) // 16) * ((W + 15) // 16)
            P = max(h * w for h, w in self.fine) if mut == "se_tiles_max_pix" else H * W
            with np.errstate(invalid="ignore"):
                m = self.pool[i, :k].astype(dtype).sum(0) / dtype(P)
            dm = U * (k + 1 + 8) * np.abs(self.pool[i, :((H + 15) // 16) * ((W + 15) // 16)].astype(np.float64)).sum(0) / (H * W)
            if self.ref_mean is not None:
                dm = dm + self.ref_dmean[i]
                if dtype == np.float64:
                    m = self.ref_mean[i]
            o.v[i], o.bound[i] = se_chain(m, dm, self.w1, self.b1, self.w2, self.b2, HSIG_MBV3, 1, dtype)
            o.mask[i] = True
        return [o]


class HeadConv(Case):
    """the head conv over concat(up8(p5) s5, up4(p4) s4, up2(p3) s3, p2 s2): op "head_fused" (nn::conv3_fpn_fused) gathers the four
    levels itself, op "conv3" (nn::conv_sp) reads the tensor materialised in float32 by the test (x), op "chain" is the operands
    of class(p5) -> class(p4) -> phase.  One reference for all three."""

    def __init__(self, name, op, fine, seed, with_scales=True):
        rng = np.random.default_rng(seed)
        self.name, self.op, self.fine = name, op, fine
        self.levels = [half(fine, 3), half(fine, 2), half(fine, 1), fine]          # p5, p4, p3, p2
        self.coarse = self.levels[2]
        n = len(fine)
        self.p = [uni(rng, (pixels(l), 24)) for l in self.levels]
        self.sc = [scales(rng, n, 24) if with_scales else None for _ in range(4)]
        self.w, self.bias = conv_w(rng), uni(rng, 24)
        if op == "head_fused":
            self.ip = [(15 if with_scales else 0) | 16 | 32]
            self.ins = self.p + [self.w, self.bias] + self.sc
        else:
            self.ip = [3]
            self.x = np.concatenate([self.cat(i, np.float32).reshape(-1, 96) for i in range(n)])
            self.ins = [self.x, self.w, self.bias]
            self.info = 6

    def cat(self, i, dtype, order=(0, 1, 2, 3)):
        parts = []
        for l in order:
            z = split(self.p[l], self.levels[l], 24)[i].astype(dtype)
            if self.sc[l] is not None:
                z = z * self.sc[l][i].astype(dtype)
            parts.append(up(z, 8 >> l))
        return np.concatenate(parts, axis=-1)

    def compute(self, dtype, mut=None, form="plain"):
        o = Out(pixels(self.fine), 24).put(dtype)
        off = offsets(self.fine)
        for i in range(len(self.fine)):
            x = self.cat(i, dtype, (3, 2, 1, 0) if mut == "head_levels_reversed" else (0, 1, 2, 3))
            if self.op == "conv3" and dtype != np.float64:   # (the reference is the unrounded concat for both forms)
                x = split(self.x, self.fine, 96)[i].astype(dtype)
            v = np.maximum(conv3(x, self.w.astype(dtype), dtype) + self.bias.astype(dtype), 0)
            S = conv3_abs(self.cat(i, np.float64), self.w) + np.abs(self.bias.astype(np.float64))
            o.v[off[i]:off[i + 1]] = v.reshape(-1, 24)
            o.mask[off[i]:off[i + 1]] = True
            o.bound[off[i]:off[i + 1]] = (U * (865 + 8 + 2) * S + 4 * U * np.abs(v.astype(np.float64))).reshape(-1, 24)
        return [o]


# ----------------------------------------------------------------------------------------------------------------------------
CLASS_PLAIN = [(5, 3), (1, 1), (17, 16), (2, 2)]       # a partial last workgroup past 256 pixels, a single pixel, odd sides
CLASS_LOWER = [(18, 16), (2, 2), (10, 6), (6, 14)]     # the lower level exactly half
TAIL_IMAGES = [(8, 8), (1, 1), (16, 20), (7, 37)]      # 259 pixels: a partial wave and waves wholly past the other images
SE_IMAGES = [(1, 1), (12, 16), (6, 10)]                # one pixel, 192 pixels (two pooling chunks), in between

CASES = {
    "phase-340": lambda: Phase("phase <3, 4, 0> cin 12 bias pool", 12, BATCH_A, F_BIAS | F_POOL, 1),
    "phase-540": lambda: Phase("phase <5, 4, 0> cin 18 bias pool", 18, BATCH_B, F_BIAS | F_POOL, 2),
    "phase-611": lambda: Phase("phase <6, 1, 1> head G relu scales", 24, BATCH_HEAD, F_G | F_RELU | F_FS | F_CS, 3),
    "phase-610": lambda: Phase("phase <6, 1, 0> head bias scales", 24, BATCH_HEAD, F_BIAS | F_FS | F_CS, 4),
    "chain-compose-phase-12": lambda: Phase("compose -> phase cin 12 pool", 12, BATCH_A, F_BIAS | F_POOL | F_COMPOSE, 5),
    "chain-compose-phase-18": lambda: Phase("compose -> phase cin 18 pool", 18, BATCH_B, F_BIAS | F_POOL | F_COMPOSE, 6),
    "class-plain": lambda: ClassOp("class p5", CLASS_PLAIN, 0, 7),
    "class-lower": lambda: ClassOp("class p4 bias scale lower", CLASS_LOWER, 7, 8),
    "compose-12": lambda: Compose("compose cin 12", 12, 3, 9),
    "compose-18": lambda: Compose("compose cin 18", 18, 3, 10),
    "tail": lambda: Tail("tail", TAIL_IMAGES, 11),
    "lateral_add-12-b": lambda: LateralAdd("lateral_add cin 12 + b", 12, [(2, 2), (6, 4), (2, 6)], True, 12),
    "lateral_add-18-b": lambda: LateralAdd("lateral_add cin 18 + b", 18, [(4, 2), (2, 2), (6, 6)], True, 13),
    "lateral_add-42": lambda: LateralAdd("lateral_add cin 42", 42, [(1, 1), (1, 2), (3, 1), (2, 2), (5, 3), (3, 6)], False, 14),
    "lateral_add-12": lambda: LateralAdd("lateral_add cin 12", 12, [(1, 5), (2, 3), (1, 7), (4, 4)], False, 15),
    "upsample_add-scale-inplace": lambda: UpsampleAdd("upsample_add scale in place", [(2, 2), (6, 4), (10, 14)], True, True, 16),
    "upsample_add-plain": lambda: UpsampleAdd("upsample_add", [(4, 6), (2, 2), (8, 2)], False, False, 17),
    "se_projected-12": lambda: SeProjected("se_projected cin 12", 12, SE_IMAGES, 18),
    "se_projected-18": lambda: SeProjected("se_projected cin 18", 18, SE_IMAGES, 19),
    "se_tiles": lambda: SeTiles("se_tiles", BATCH_A, 20),
    "head_fused": lambda: HeadConv("head_fused", "head_fused", BATCH_HEAD, 21),
    "conv3": lambda: HeadConv("conv3 96 -> 24", "conv3", BATCH_HEAD, 21),
}
CASE_IDS = list(CASES)

# every mutant and the cases whose data can tell it apart
MUTANTS = {
    "phase_pxpy": ["phase-340", "phase-611"],
    "phase_taps_swapped": ["phase-340", "phase-540", "phase-611"],
    "rowclass3_interior": ["phase-611"],
    "quarter_index_off": ["phase-611"],
    "lower_parity_inverted": ["class-lower"],
    "lower_at_yx": ["class-lower"],
    "bias_twice": ["phase-611"],
    "fine_scale_img0": ["phase-611", "phase-610"],
    "wf_img0": ["phase-340", "phase-540", "chain-compose-phase-12"],
    "compose_no_se": ["compose-12", "compose-18", "chain-compose-phase-18"],
    "compose_pad_nonzero": ["compose-18", "chain-compose-phase-18"],
    "pool_premask": ["phase-340", "phase-540"],
    "se_tiles_max_tiles": ["se_tiles"],
    "se_tiles_max_pix": ["se_tiles"],
    "head_levels_reversed": ["head_fused"],
    "upsample_yp1": ["upsample_add-scale-inplace", "upsample_add-plain"],
    "lateral_scale_after_add": ["lateral_add-12-b", "lateral_add-18-b"],
    "tail_dydx_transposed": ["tail"],
    "tail_no_relu": ["tail"],
    "tail_rows_swapped": ["tail"],
}


@functools.lru_cache(maxsize=None)
def case(case_id):
    return CASES[case_id]()
