"""Kernel-level numerics: every fp32 GEMM route behind nn::gemm() and the SVTR attention, one launch at a time through
rt_debug_gemm / rt_debug_attention, against fp64 references computed with numpy on the host.

The whole-network tests (test_gpu_parity.py) reach a kernel only at the shapes the networks happen to have, after several
layers of normalisation; here each route is driven at its edges (row counts at and around its tile and threshold sizes, K
tails, pad columns, concat offsets, squeeze-excite tables, every epilogue), the plan that ran is asserted, and every output
element is held to the classical worst-case bound of a K-term fp32 sum:

    |got - ref| <= 2^-24 (K + 8) S L + 4 2^-24 R     (+ 6 2^-24 S on the split-bf16 route)

with S = sum_k |a_k w_k| + |bias|, L the epilogue's Lipschitz factor (hardswish 1.5, swish 1.1, sigmoid 0.25, else 1; times
|lab_a|) and R = |epilogue value| + |residual|.  A lost or doubled 16-deep K group moves an element by hundreds of bounds.
The rms error must also stay within twice that of a CPU fp32 product (torch) of the same operands and epilogue.  The worst
err / bound ratio per route is printed (-s); measured on an MI355X: narrow 0.183, stream 0.071, wide_128x128 0.078,
wide_128x240 0.040, wide_256x240 0.045, k_gemm32w 0.027, k_gemm32p 0.023, split-bf16 0.018.  Attention: max error 6.3e-6 ...
8.7e-6 of max|v| (bound 1e-5)."""
import ctypes as C

import numpy as np
import pytest
import torch

from retto_amd import workmodel

pytestmark = pytest.mark.gpu

NONE, RELU, HSWISH, SWISH, SIGMOID = 0, 1, 2, 3, 4
# nn::GemmKernel (gemm_plan.h)
SPLIT, W, DMA, W256, W128x240, W128, STREAM, NARROW, AM256, AM128, AMN = range(2, 13)
KNAME = {SPLIT: "split", W: "w", DMA: "dma", W256: "wide_256x240", W128x240: "wide_128x240", W128: "wide_128x128",
         STREAM: "stream", NARROW: "narrow", AM256: "argmax_256x240", AM128: "argmax_128x128", AMN: "argmax_narrow"}
CANARY = 0x7FA5C3E1   # RT_DEBUG_CANARY
U = 2.0 ** -24
LIP = {NONE: 1.0, RELU: 1.0, HSWISH: 1.5, SWISH: 1.1, SIGMOID: 0.25}
LAB = (1.3, 0.07)
WORST = {}            # route -> worst err / bound


def _pitch(c):
    return (c + 31) // 32 * 32 if c >= 128 else (c + 3) // 4 * 4


def _up4(n):
    return (n + 3) // 4 * 4


@pytest.fixture(scope="module")
def dev(hip_session):
    yield hip_session._hd.lib, hip_session._hd.h
    if WORST:
        print("\nworst err / bound per route: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def _operands(M, K, N, seed, lda=None):
    rng = np.random.default_rng(seed)
    lda = _pitch(K) if lda is None else lda
    A = np.zeros((M, lda), np.float32)
    A[:, :K] = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    Wt = (rng.uniform(-1, 1, (K, N)) * (4.0 / np.sqrt(K))).astype(np.float32)
    bias = rng.uniform(-1, 1, N).astype(np.float32)
    return A, Wt, bias


def run_gemm(dev, A, K, Wt, bias=None, act=HSWISH, lab=None, residual=None, se=None, se_rows=0, ldc=None, coff=0, variant=0,
             ctc=-1):
    """One rt_debug_gemm call: (the whole (M + 64) x ldc output buffer, plan (kernel, nt, kg, se, bf), CTC idx, CTC prob)."""
    lib, h = dev
    M, lda = A.shape
    N = Wt.shape[1]
    ldc = _pitch(N) if ldc is None else ldc
    A = np.ascontiguousarray(A, np.float32)
    Wt = np.ascontiguousarray(Wt, np.float32)
    out = np.empty((M + 64, ldc), np.float32)
    plan = (C.c_int * 5)()
    p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    bias = None if bias is None else np.ascontiguousarray(bias, np.float32)
    res = None if residual is None else np.ascontiguousarray(residual, np.float32)
    scale = rows = None
    if se is not None:
        scale = np.ascontiguousarray(se[0], np.float32)
        rows = np.ascontiguousarray(se[1], np.int64)
    idx = np.zeros(M, np.int32) if ctc >= 0 else None
    prob = np.zeros(M, np.float32) if ctc >= 0 else None
    la, lc = lab if lab else (1.0, 0.0)
    rc = lib.rt_debug_gemm(h, A.ctypes.data, M, K, lda, Wt.ctypes.data, N, p(bias), act, 1 if lab else 0, la, lc, p(res),
                           0 if res is None else res.shape[1], p(scale), 0 if scale is None else scale.shape[1], p(rows),
                           0 if rows is None else len(rows), se_rows, ldc, coff, variant, ctc, out.ctypes.data, p(idx), p(prob),
                           plan)
    assert rc == 0, lib.rt_last_error(h)
    return out, tuple(plan), idx, prob


def _act64(v, act):
    if act == HSWISH:
        return v * np.clip(v + 3.0, 0.0, 6.0) / 6.0
    if act == RELU:
        return np.maximum(v, 0.0)
    if act == SWISH:
        return v / (1.0 + np.exp(-v))
    if act == SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def _act32(v, act):
    if act == HSWISH:
        return v * torch.clamp(v + 3.0, 0.0, 6.0) / 6.0
    if act == RELU:
        return torch.clamp(v, min=0.0)
    if act == SWISH:
        return v * torch.sigmoid(v)
    if act == SIGMOID:
        return torch.sigmoid(v)
    return v


def _sample(M, tile):
    """All rows up to 20 k; else the first two and the last two row tiles plus every 61st row."""
    if M <= 20000:
        return np.arange(M)
    last = ((M + tile - 1) // tile - 2) * tile
    return np.unique(np.concatenate([np.arange(2 * tile), np.arange(last, M), np.arange(0, M, 61)]))


def _row_scales(se, rows):
    scale, img_rows = se
    img = np.searchsorted(np.cumsum(img_rows), rows, side="right")
    return scale[img]


def check(name, dev, A, K, Wt, bias=None, act=HSWISH, lab=None, residual=None, se=None, se_rows=0, ldc=None, coff=0, variant=0,
          expect=None, tile=256, split=False):
    """Runs one launch and checks plan, layout, the element bound and the rms against torch fp32.  Returns the output rows."""
    M = A.shape[0]
    N = Wt.shape[1]
    ldc = _pitch(N) if ldc is None else ldc
    out, plan, _, _ = run_gemm(dev, A, K, Wt, bias, act, lab, residual, se, se_rows, ldc, coff, variant)
    if expect is not None:
        kern, nt, kg = (tuple(expect) + (None, None))[:3]
        got_plan = (KNAME.get(plan[0], plan[0]),) + plan[1:]
        assert plan[0] == kern, "%s: plan %s, expected %s" % (name, got_plan, KNAME[kern])
        assert nt is None or plan[1] == nt, "%s: plan %s, expected nt %d" % (name, got_plan, nt)
        assert kg is None or plan[2] == kg, "%s: plan %s, expected kg %d" % (name, got_plan, kg)
        assert plan[3] == (se is not None), (name, got_plan)
    # layout: the pad columns [N, round_up(N, 4)) are zeros; nothing outside [coff, coff + round_up(N, 4)) and no row >= M is written
    bits = out.view(np.uint32)
    n4 = _up4(N)
    assert (bits[M:] == CANARY).all(), "%s: rows past M written" % name
    assert (bits[:M, :coff] == CANARY).all() and (bits[:M, coff + n4:] == CANARY).all(), "%s: columns outside the slice written" % name
    assert (bits[:M, coff + N:coff + n4] == 0).all(), "%s: pad columns are not zero" % name
    rows = _sample(M, tile)
    a32 = A[rows, :K]
    if se is not None:
        a32 = (a32 * _row_scales(se, rows)[:, :K]).astype(np.float32)   # (the kernels scale A in fp32 while staging it)
        a64 = A[rows, :K].astype(np.float64) * _row_scales(se, rows)[:, :K].astype(np.float64)
    else:
        a64 = a32.astype(np.float64)
    w64 = Wt.astype(np.float64)
    b64 = np.zeros(N) if bias is None else bias.astype(np.float64)
    acc = a64 @ w64 + b64
    S = np.abs(a64) @ np.abs(w64) + np.abs(b64)
    ev = _act64(acc, act)
    L = LIP[act]
    t = torch.from_numpy(np.ascontiguousarray(a32)) @ torch.from_numpy(Wt) + (0 if bias is None else torch.from_numpy(bias))
    t = _act32(t, act)
    if lab:
        ev = ev * lab[0] + lab[1]
        t = t * lab[0] + lab[1]
        L *= abs(lab[0])
    R = np.abs(ev)
    ref = ev
    if residual is not None:
        r = residual[rows, :N]
        ref = ev + r.astype(np.float64)
        R = R + np.abs(r)
        t = t + torch.from_numpy(np.ascontiguousarray(r))
    bound = U * (K + 8) * S * L + 4 * U * R + (6 * U * S if split else 0)
    got = out[rows, coff:coff + N].astype(np.float64)
    assert np.isfinite(got).all(), name
    err = np.abs(got - ref)
    ratio = float((err / bound).max())
    WORST[KNAME.get(plan[0], plan[0])] = max(WORST.get(KNAME.get(plan[0], plan[0]), 0.0), ratio)
    bad = np.argwhere(err > bound)
    assert ratio <= 1.0, "%s: err / bound %.3g at row %d col %d (got %r ref %r)" % (
        name, ratio, rows[bad[0][0]], bad[0][1], got[tuple(bad[0])], ref[tuple(bad[0])])
    rms = float(np.sqrt(np.mean(err ** 2)))
    rms_cpu = float(np.sqrt(np.mean((t.numpy().astype(np.float64) - ref) ** 2)))
    assert rms <= 2 * rms_cpu, "%s: rms err %.3g, torch fp32 %.3g" % (name, rms, rms_cpu)
    return out[:M]


# ------------------------------------------------------------------------------------------------------------------------------
# routes: (id, M, K, N, forced variant, extra, expected (kernel, nt, kg)); nt / kg as gemm_plan() picks them on 256 CUs
ROUTES = [
    # production thresholds: at each and one row below
    ("mid_16383", 16383, 240, 960, 0, {}, (NARROW, 6)),
    ("mid_16384", 16384, 240, 960, 0, {}, (W128x240,)),
    ("split_32767", 32767, 240, 480, 40, {}, (DMA,)),
    ("split_32768", 32768, 240, 480, 40, {}, (SPLIT,)),
    ("w_65535", 65535, 128, 128, 0, {}, (NARROW, 8)),
    ("w_65536", 65536, 128, 128, 0, {}, (W,)),
    ("stream_65535", 65535, 64, 64, 0, {}, (NARROW, 4)),
    ("stream_65536", 65536, 64, 64, 0, {}, (STREAM, 4, 4)),
    ("dma_131071", 131071, 240, 240, 0, {}, (W128x240,)),
    ("dma_131072", 131072, 240, 240, 0, {}, (DMA,)),
    # M = +-1 modulo the row tile (w 64, stream 32, narrow / 128-row wide tiles 128, 256-row tiles 256); K tails 4 / 16 / 28 mod 32
    ("w_m+1", 65537, 128, 128, 0, {}, (W,)),
    ("w_m-1", 65599, 128, 128, 0, {}, (W,)),
    ("dma_m+1_k240", 2561, 240, 480, 30, {}, (DMA,)),
    ("dma_m-1_k144", 2559, 144, 240, 30, {}, (DMA,)),
    ("dma_k480", 1279, 480, 480, 30, {}, (DMA,)),
    ("w256_m+1_k100", 2561, 100, 240, 15, {}, (W256,)),
    ("w256_m-1_k124_n202", 2559, 124, 202, 15, {}, (W256,)),
    ("w128x240_m+1_k112", 1153, 112, 240, 10, {}, (W128x240,)),
    ("w128x240_m-1_k100_n470", 1151, 100, 470, 10, {}, (W128x240,)),
    ("w128_m+1_k124_n102", 1153, 124, 102, 8, {}, (W128,)),
    ("w128_m-1_k36_n250", 1151, 36, 250, 8, {}, (W128,)),
    ("stream_m+1_k28_n30", 3201, 28, 30, 20, {}, (STREAM, 2, 2)),
    ("stream_m-1_k100_n102", 3199, 100, 102, 20, {}, (STREAM, 8, 8)),
    ("narrow_m+1_k4_n30", 1153, 4, 30, 1, {}, (NARROW, 1)),
    ("narrow_m-1_k16_n62", 1151, 16, 62, 1, {}, (NARROW, 1)),
    ("narrow_k28_n201", 1025, 28, 201, 1, {}, (NARROW, 1)),
    ("split_m+1", 32769, 240, 240, 40, {}, (SPLIT,)),
    ("split_m-1_k144", 33023, 144, 480, 40, {}, (SPLIT,)),
    # a slice of a wider tensor (the concat layers: ldc > chan_pitch(N), coff > 0)
    ("narrow_coff", 1000, 120, 60, 1, {"ldc": 128, "coff": 64}, (NARROW, 1)),
    ("dma_coff", 2000, 240, 240, 30, {"ldc": 512, "coff": 256}, (DMA,)),
    ("w128x240_coff", 1000, 120, 240, 10, {"ldc": 512, "coff": 248}, (W128x240,)),
    ("split_coff", 32768, 240, 240, 40, {"ldc": 512, "coff": 256}, (SPLIT,)),
    ("stream_coff", 3000, 64, 60, 20, {"ldc": 128, "coff": 60}, (STREAM, 4, 4)),
    # small M: the narrow kernel halves its column tiles until there is a workgroup per CU
    ("nt8", 65536, 96, 128, 0, {}, (NARROW, 8)),
    ("nt4", 32768, 96, 128, 0, {}, (NARROW, 4)),
    ("nt2", 16384, 96, 128, 0, {}, (NARROW, 2)),
    ("nt1", 8192, 96, 128, 0, {}, (NARROW, 1)),
]


@pytest.mark.parametrize("name,M,K,N,variant,extra,expect", ROUTES, ids=[r[0] for r in ROUTES])
def test_gemm_route(dev, name, M, K, N, variant, extra, expect):
    """One route at one edge, bias + hardswish + LAB (the LCNet pointwise epilogue), against fp64."""
    A, Wt, bias = _operands(M, K, N, seed=M + 7 * K + N)
    check(name, dev, A, K, Wt, bias, HSWISH, LAB, variant=variant, expect=expect, split=expect[0] == SPLIT, **extra)


def _network_layers():
    """(K, N, squeeze-excite) -> the smallest and the largest M of the pointwise GEMMs the work model prices (C3 and C4-like
    mixes, as test_gemm_plan_cpu.py collects them)."""
    seen = {}
    orig = workmodel.gemm_pw_label

    def rec(M, K, N, se=False, min_pix=1 << 30):
        seen.setdefault((K, N, bool(se)), []).append(M)
        return orig(M, K, N, se, min_pix)

    workmodel.gemm_pw_label = rec
    try:
        workmodel.det_work([(960, 960)] * 32)
        workmodel.rec_work([320] * 1024)
        workmodel.det_work([(640, 640), (960, 960), (736, 1280), (1088, 1920), (1760, 1248), (3520, 2496), (960, 960), (640, 640)])
        workmodel.rec_work([96, 160, 320, 480, 800, 1280, 3648] * 40 + [320] * 600)
        workmodel.rec_work([320, 480])
        workmodel.det_work([(960, 960)])
        workmodel.cls_work(600)
    finally:
        workmodel.gemm_pw_label = orig
    return sorted((k, min(v), max(v)) for k, v in seen.items())


NET_LAYERS = _network_layers()
# the SVTR neck's GEMMs (nets.cpp RecNet / SvtrCore): (K, N, act, ldc, coff)
NECK = [(60, 120, SWISH, 120, 0), (120, 360, NONE, 360, 0), (120, 120, NONE, 120, 0), (120, 240, SWISH, 240, 0),
        (240, 120, NONE, 120, 0), (120, 480, SWISH, 960, 480)]


def _images(total, seed):
    """Image row counts of >= 128 rows adding up to total (the squeeze-excite levels of a ragged batch)."""
    rng = np.random.default_rng(seed)
    rows = []
    while total - sum(rows) >= 3000:
        rows.append(int(rng.integers(128, 1500)))
    rest = total - sum(rows)
    return rows + [rest // 2, rest - rest // 2]


def _se_scales(n_img, ld, seed):
    # distinct per image, so that a row scaled with the wrong image's vector moves its result
    return np.random.default_rng(seed).uniform(0.2, 2.0, (n_img, ld)).astype(np.float32)


@pytest.mark.parametrize("K,N,se,Mmin,Mmax", [(k[0], k[1], k[2], a, b) for k, a, b in NET_LAYERS],
                         ids=["%dx%d%s" % (k[0], k[1], "se" if k[2] else "") for k, _, _ in NET_LAYERS])
def test_gemm_network_layer(dev, K, N, se, Mmin, Mmax):
    """Every (K, N, squeeze-excite) of the LCNet pointwise convs, production rule, hardswish + LAB: at the layer's smallest row
    count and at its largest (capped at 150 000 rows); the squeeze-excite layers with the table the networks build."""
    assert len(NET_LAYERS) >= 10
    for M in sorted({Mmin, min(Mmax, 150000)}):
        A, Wt, bias = _operands(M, K, N, seed=K * N + M)
        sc = None
        if se and M >= 8192:   # (below, no fused form: the network scales the tensor in a pass of its own)
            rows = _images(M, M)
            sc = (_se_scales(len(rows), A.shape[1], M), rows)
        check("net %dx%d M %d" % (K, N, M), dev, A, K, Wt, bias, HSWISH, LAB, se=sc)


@pytest.mark.parametrize("K,N,act,ldc,coff", NECK, ids=["neck%dx%d" % (k, n) for k, n, _, _, _ in NECK])
@pytest.mark.parametrize("M", [457, 30000])
def test_gemm_neck_layer(dev, K, N, act, ldc, coff, M):
    """The SVTR neck's GEMMs (lda = K, swish or no activation, conv3 into the second half of the 960-channel concat)."""
    A, Wt, bias = _operands(M, K, N, seed=K + N + M, lda=K)
    check("neck %dx%d" % (K, N), dev, A, K, Wt, bias, act, ldc=ldc, coff=coff)


EPI_ROUTES = [(1, 1031, 100, 70, NARROW), (8, 1031, 100, 250, W128), (10, 1031, 112, 240, W128x240), (15, 1031, 100, 240, W256),
              (20, 1031, 60, 70, STREAM), (30, 1031, 240, 480, DMA)]


@pytest.mark.parametrize("variant,M,K,N,kern", EPI_ROUTES, ids=[KNAME[r[4]] for r in EPI_ROUTES])
def test_gemm_epilogues(dev, variant, M, K, N, kern):
    """ACT_NONE / RELU / HSWISH / SWISH / SIGMOID, each with and without LAB and with and without a residual: the epilogue's
    compile-time forms (act_dispatch) and its per-element form.  Reference: epi(acc + bias), then + residual[m ld_res + n].
    (The persistent k_gemm32p takes no residual.)"""
    A, Wt, bias = _operands(M, K, N, seed=variant)
    res = np.random.default_rng(variant + 1).uniform(-2, 2, (M, _pitch(N) + 8)).astype(np.float32)
    for act in (NONE, RELU, HSWISH, SWISH, SIGMOID):
        for lab in (None, LAB):
            for r in ((None, res) if kern != DMA else (None,)):
                check("%s act %d lab %s res %s" % (KNAME[kern], act, lab, r is not None), dev, A, K, Wt, bias, act, lab, r,
                      variant=variant, expect=(kern,))


SE_MIXES = {
    "two_per_block": [200, 300, 131, 250, 128, 517, 140, 333, 129, 180],      # 128-row blocks across two images
    "three_per_256": [200, 128, 150, 131, 300, 128, 140, 129, 128, 128, 301],  # 256-row blocks across three images
    "exactly_128": [128] * 24,
    "partial_last": [128] * 10 + [129, 140, 150],                             # the last block partial
}
SE_ROUTES = [(8, 128, 384, 384, W128), (10, 128, 480, 480, W128x240), (30, 256, 480, 480, DMA), (30, 256, 240, 240, DMA)]


@pytest.mark.parametrize("mix", sorted(SE_MIXES))
@pytest.mark.parametrize("variant,se_rows,K,N,kern", SE_ROUTES, ids=["%s_%d_k%d" % (KNAME[r[4]], r[1], r[2]) for r in SE_ROUTES])
def test_gemm_squeeze_excite(dev, mix, variant, se_rows, K, N, kern):
    """The scale folded into the A staging: the 2-int table (128-row tiles of the wide kernels) and the 3-int one (k_gemm32p's
    256-row blocks), on image mixes whose row blocks span two and three images, images of exactly 128 rows, a partial last
    block; every image has its own scale vector."""
    rows = SE_MIXES[mix] * 4
    M = sum(rows)
    A, Wt, bias = _operands(M, K, N, seed=M + K)
    sc = (_se_scales(len(rows), A.shape[1], len(rows) + K), rows)
    check("se %s %s" % (KNAME[kern], mix), dev, A, K, Wt, bias, HSWISH, LAB, se=sc, se_rows=se_rows, variant=variant, expect=(kern,))


@pytest.mark.parametrize("se_rows", [128, 256])
def test_gemm_squeeze_excite_split(dev, se_rows):
    """The split-bf16 kernel with either table (32768 rows and more)."""
    rows = (SE_MIXES["three_per_256"] * 30)[:220]
    M = sum(rows)
    assert M >= 32768
    A, Wt, bias = _operands(M, 480, 480, seed=se_rows)
    sc = (_se_scales(len(rows), A.shape[1], 5), rows)
    check("se split %d" % se_rows, dev, A, 480, Wt, bias, HSWISH, LAB, se=sc, se_rows=se_rows, variant=40, expect=(SPLIT,),
          split=True)


@pytest.mark.parametrize("form,kern", [(0, AMN), (1, AM256), (2, AM128)])
def test_ctc_head_argmax(dev, form, kern):
    """The CTC head's fused argmax (6625 classes, K = 120): idx equal to the fp64 argmax wherever the fp64 top-2 margin
    exceeds twice the element bound, prob = softmax max within 1e-5 relative; many rows have their maximum in the last,
    partial column tile; the logits never reach memory (the output buffer keeps its canary)."""
    M, K, N = 1000, 120, 6625
    A, Wt, bias = _operands(M, K, N, seed=form + 11, lda=K)
    Wt[:, 6600:] *= 2.5
    out, plan, idx, prob = run_gemm(dev, A, K, Wt, bias, NONE, ctc=form, ldc=_up4(N))
    assert plan[0] == kern, plan
    assert (out.view(np.uint32) == CANARY).all()
    a64, w64 = A[:, :K].astype(np.float64), Wt.astype(np.float64)
    logits = a64 @ w64 + bias
    bound = (U * (K + 8) * (np.abs(a64) @ np.abs(w64) + np.abs(bias))).max(1)
    top = np.argmax(logits, 1)
    srt = np.sort(logits, 1)
    margin = srt[:, -1] - srt[:, -2]
    p = np.exp(logits - srt[:, -1:])
    pmax = 1.0 / p.sum(1)
    last_tile = top >= 6528
    assert 0.1 < last_tile.mean() < 0.9, last_tile.mean()
    decisive = margin > 2 * bound
    assert decisive.mean() > 0.9
    assert (idx[decisive] == top[decisive]).all()
    assert np.abs(prob - pmax).max() <= 1e-5 * pmax.max(), np.abs(prob / pmax - 1).max()


# ------------------------------------------------------------------------------------------------------------------------------
IDENTITY = [
    # (K, N): the routes that take it (variant, kernel), and the production launches at large M whose first rows are compared
    (240, 240, [(1, NARROW), (8, W128), (10, W128x240), (15, W256), (30, DMA)], [(131072, DMA), (65536, W128x240)]),
    (128, 128, [(1, NARROW), (8, W128), (20, STREAM)], [(65536, W)]),
    (64, 64, [(1, NARROW), (8, W128), (20, STREAM)], [(65536, STREAM)]),
]


@pytest.mark.parametrize("K,N,forced,big", IDENTITY, ids=["%dx%d" % (r[0], r[1]) for r in IDENTITY])
def test_gemm_routes_are_bit_identical(dev, K, N, forced, big):
    """DESIGN section 3 (a page alone equals the page in a batch) rests on this: a row gets the same bits from every fp32-MFMA
    route that accepts its shape, whatever M the launch has (split-bf16 is another summation order by construction)."""
    M0 = 2561
    Mbig = max(m for m, _ in big)
    A, Wt, bias = _operands(Mbig, K, N, seed=K)
    outs = {}
    for v, kern in forced:
        out, plan, _, _ = run_gemm(dev, A[:M0], K, Wt, bias, HSWISH, LAB, variant=v)
        assert plan[0] == kern, (v, plan)
        outs[KNAME[kern]] = out[:M0]
    for m, kern in big:
        out, plan, _, _ = run_gemm(dev, A[:m], K, Wt, bias, HSWISH, LAB)
        assert plan[0] == kern, (m, plan)
        outs["%s@%d" % (KNAME[kern], m)] = out[:M0]
    base = outs["narrow"].view(np.uint32)
    diff = {k: int((o.view(np.uint32) != base).any(1).sum()) for k, o in outs.items()}
    assert all(d == 0 for d in diff.values()), "rows differing from the narrow kernel's: %s" % diff


@pytest.mark.parametrize("variant,M,K,N,kern", [(0, 131072, 240, 240, DMA), (0, 131072, 128, 128, W), (40, 131072, 240, 240, SPLIT)],
                         ids=["dma", "w", "split"])
def test_persistent_routes_are_repeatable(dev, variant, M, K, N, kern):
    """The persistent kernels (tile queues, LDS-DMA, counted vmcnt) 8 times at >= 2 tiles per CU: bit-identical every time."""
    A, Wt, bias = _operands(M, K, N, seed=3)
    first = None
    for _ in range(8):
        out, plan, _, _ = run_gemm(dev, A, K, Wt, bias, HSWISH, LAB, variant=variant)
        assert plan[0] == kern, plan
        if first is None:
            first = out
        else:
            assert np.array_equal(out.view(np.uint32), first.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------
HD = 15


def run_attention(dev, qkv, tokens, heads):
    lib, h = dev
    qkv = np.ascontiguousarray(qkv, np.float32)
    out = np.zeros((qkv.shape[0], heads * HD), np.float32)
    t = np.ascontiguousarray(tokens, np.int32)
    rc = lib.rt_debug_attention(h, qkv.ctypes.data, qkv.shape[0], t.ctypes.data, len(t), heads, out.ctypes.data)
    assert rc == 0, lib.rt_last_error(h)
    return out


def _qkv(tokens, heads, seed, big=()):
    rng = np.random.default_rng(seed)
    C3 = 3 * heads * HD
    parts = []
    for i, T in enumerate(tokens):
        x = rng.uniform(-2, 2, (T, C3)).astype(np.float32)
        if i in big:   # q . k / sqrt(15) up to ~120: expf without the running maximum overflows
            x[:, :2 * heads * HD] = rng.uniform(4.5, 6.5, (T, 2 * heads * HD))
        parts.append(x)
    return np.concatenate(parts)


def attention_ref(qkv, tokens, heads):
    C = heads * HD
    out = np.zeros((qkv.shape[0], C))
    off = 0
    for T in tokens:
        x = qkv[off:off + T].astype(np.float64)
        for hh in range(heads):
            q, k, v = (x[:, j * C + hh * HD:j * C + (hh + 1) * HD] for j in range(3))
            s = q @ k.T / np.sqrt(HD)
            p = np.exp(s - s.max(1, keepdims=True))
            out[off:off + T, hh * HD:(hh + 1) * HD] = (p / p.sum(1, keepdims=True)) @ v
        off += T
    return out


SHORT_T = [1, 2, 15, 16, 17, 63, 64, 65, 120, 127, 128, 50]
LONG_T = [129, 200, 456]


@pytest.mark.parametrize("heads", [8, 4, 6, 12])
def test_attention_against_fp64(dev, heads):
    """softmax(Q K^T / sqrt(15)) V per head against fp64, lines of 1 ... 128 tokens (k_attention_mfma for 4 / 8 heads; the 64 KB
    LDS case at 121 ... 128) and of 129 ... 456 (k_attention_line); 6 and 12 heads take k_attention.  The last short and the
    first long line have logits beyond 88.  Error <= 1e-5 max|v| (measured: see DESIGN.md section 3)."""
    tokens = SHORT_T + LONG_T
    qkv = _qkv(tokens, heads, seed=heads, big=(len(SHORT_T) - 1, len(SHORT_T)))
    got = run_attention(dev, qkv, tokens, heads)
    ref = attention_ref(qkv, tokens, heads)
    vmax = float(np.abs(qkv[:, 2 * heads * HD:]).max())
    err = float(np.abs(got - ref).max())
    print("\nattention heads %d: max err %.3g = %.3g max|v|" % (heads, err, err / vmax))
    assert err <= 1e-5 * vmax, err


@pytest.mark.parametrize("heads", [8, 4])
def test_attention_line_does_not_depend_on_its_batch_mates(dev, heads):
    """Lines of <= 128 tokens give the same bits alone as next to a 456-token line (the kernel is chosen per line)."""
    qkv = _qkv(SHORT_T + [456], heads, seed=heads + 100)
    n = sum(SHORT_T)
    alone = run_attention(dev, qkv[:n], SHORT_T, heads)
    mixed = run_attention(dev, qkv, SHORT_T + [456], heads)
    assert np.array_equal(alone.view(np.uint32), mixed[:n].view(np.uint32))


def test_rec_lines_do_not_depend_on_a_long_line_in_their_call(hip_session):
    """rt_rec_ragged: lines of width >= 96 alone equal the same lines next to a 3648-wide (456-token) line, bit for bit.  (Every
    image keeps >= 128 rows at the squeeze-excite levels and the rows stay below the large-M routes, so no other choice moves.)"""
    rng = np.random.default_rng(77)
    widths = [96, 120, 160, 200, 320, 487]
    lines = [rng.uniform(-1, 1, (3, 48, w)).astype(np.float32) for w in widths]
    long_line = rng.uniform(-1, 1, (3, 48, 3648)).astype(np.float32)
    alone = hip_session.worker.rec_ragged(lines)
    mixed = hip_session.worker.rec_ragged(lines + [long_line])
    for w, a, m in zip(widths, alone, mixed):
        assert a.shape == m.shape
        assert np.array_equal(a.view(np.uint32), m.view(np.uint32)), "width %d: max diff %g" % (w, np.abs(a - m).max())
