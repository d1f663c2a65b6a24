"""The fp32 GEMM kernel choice (retto_amd/csrc/gemm_plan.cpp) on the host: a pinned table of shapes -> (kernel, template choice,
grid, label), read off the launch rules gemm() had before they moved into the plan, and the work model's label mirror
(retto_amd/workmodel.py gemm_pw_label) against the plan for every pointwise GEMM of the C3 / C4 networks.  The plan is compiled
with g++ into tests/native/gemm_plan_driver.cpp (tests/plan_driver.py): no GPU, no HIP runtime."""
import pytest

import plan_driver
from plan_driver import run as _run
from retto_amd import workmodel

HSWISH, RELU = 2, 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return plan_driver.build(tmp_path_factory)


def _pitch(c):
    return (c + 31) // 32 * 32 if c >= 128 else (c + 3) // 4 * 4


def plan_query(M, K, N, variant=0, dma=1, split=0, amw=0, cus=256, lda=None, ldc=None, coff=0, am=0, residual=0, se=0,
               act=HSWISH, n_img=3, ld_scale=None):
    """A gemm() call as the networks make it: K = channels rounded to 4, A pitch chan_pitch(K), C pitch chan_pitch(N);
    se = 2 / 3: a squeeze-excite scale with that row-table form."""
    npad = (N + 15) // 16 * 16
    lda = _pitch(K) if lda is None else lda
    ldc = _pitch(N) if ldc is None else ldc
    ld_scale = lda if ld_scale is None else ld_scale
    return "plan %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d 1 %d %d" % (
        variant, dma, split, amw, cus, lda, M, K, N, npad, ldc, coff, am, residual, 1 if se else 0, se or 2, act, n_img, ld_scale)


def se_query(M, K, N, variant=0, dma=1, split=0, min_pix=1 << 30, act=HSWISH):
    return "se_rows %d %d %d %d %d %d %d %d %d %d" % (variant, dma, split, _pitch(K), M, K, N, (N + 15) // 16 * 16, act, min_pix)


TH = "gemm_pw/thin"
W543, W443, W442 = "gemm_pw/k_gemm_wide<4,5,4,3>", "gemm_pw/k_gemm_wide<2,5,4,3>", "gemm_pw/k_gemm_wide<2,4,4,2>"
P, PSE, S, SSE, GW = "gemm_pw/k_gemm32p", "gemm_pw/k_gemm32p+se", "gemm_pw/k_gemm_split", "gemm_pw/k_gemm_split+se", "gemm_pw/k_gemm32w"

# (what it pins, query, "kernel nt kg bf se grid_x grid_y label")
PLAN_TABLE = [
    # M thresholds of the production rule on a k_gemm32p-capable layer (240 x 240)
    ("131071 rows: 128 x 240 tile", plan_query(131071, 240, 240), "wide_128x240 0 0 0 0 1024 1 " + W443),
    ("131072 rows: k_gemm32p", plan_query(131072, 240, 240), "dma 0 0 0 0 0 0 " + P),
    ("131072 rows, LDS-DMA off: 256 x 240 tile", plan_query(131072, 240, 240, dma=0), "wide_256x240 0 0 0 0 512 1 " + W543),
    ("16383 rows of 480: narrow", plan_query(16383, 480, 480), "narrow 6 0 1 0 128 5 " + TH),
    # the mid-tile rule: (M + 127) / 128 x Npad16 / 240 >= 512
    ("mid rule 511 blocks x 1", plan_query(65408, 240, 240), "narrow 5 0 1 0 511 3 " + TH),
    ("mid rule 512 blocks x 1", plan_query(65409, 240, 240), "wide_128x240 0 0 0 0 512 1 " + W443),
    ("mid rule 255 blocks x 2", plan_query(32640, 480, 480), "narrow 6 0 1 0 255 5 " + TH),
    ("mid rule 256 blocks x 2", plan_query(32641, 480, 480), "wide_128x240 0 0 0 0 256 2 " + W443),
    ("16384 rows of 480 below the mid rule", plan_query(16384, 480, 480), "narrow 6 0 1 0 128 5 " + TH),
    # split kernel: 32768 rows
    ("split on, 32767 rows", plan_query(32767, 240, 240, split=1), "narrow 5 0 1 0 256 3 " + TH),
    ("split on, 32768 rows", plan_query(32768, 240, 240, split=1), "split 0 0 0 0 0 0 " + S),
    # k_gemm32w (K = N = 128) and the streaming kernel (K, N <= 64): 65536 rows
    ("K = N = 128, 65535 rows", plan_query(65535, 128, 128), "narrow 8 0 1 0 512 1 " + TH),
    ("K = N = 128, 65536 rows", plan_query(65536, 128, 128), "w 0 0 0 0 0 0 " + GW),
    ("C3 rec 2456736 x 128 x 128", plan_query(2456736, 128, 128), "w 0 0 0 0 0 0 " + GW),
    ("K = N = 64, 65535 rows", plan_query(65535, 64, 64), "narrow 4 0 1 0 512 1 " + TH),
    ("K = N = 64, 65536 rows", plan_query(65536, 64, 64), "stream 4 4 0 0 512 1 " + TH),
    ("stream 2456736 x 64 x 48", plan_query(2456736, 64, 48), "stream 3 4 0 0 2048 1 " + TH),
    # the narrow kernel's NT occupancy loop: 256 CUs (a whole device) and 32 (one lane's CU partition)
    ("3600 x 480 x 480 on 256 CUs", plan_query(3600, 480, 480), "narrow 1 0 1 0 29 30 " + TH),
    ("3600 x 480 x 480 on 32 CUs", plan_query(3600, 480, 480, cus=32), "narrow 6 0 1 0 29 5 " + TH),
    ("14400 x 96 x 96 on 256 CUs", plan_query(14400, 96, 96), "narrow 1 0 1 0 113 6 " + TH),
    ("14400 x 96 x 96 on 32 CUs", plan_query(14400, 96, 96, cus=32), "narrow 6 0 1 0 113 1 " + TH),
    # K = 96 / 128: more than three 32-deep slabs
    ("K = 96 at 131072 rows", plan_query(131072, 96, 240), "wide_256x240 0 0 0 0 512 1 " + W543),
    ("K = 128 at 131072 rows", plan_query(131072, 128, 240), "dma 0 0 0 0 0 0 " + P),
    ("split on, K = 96", plan_query(131072, 96, 240, split=1), "wide_256x240 0 0 0 0 512 1 " + W543),
    ("split on, K = 128", plan_query(131072, 128, 240, split=1), "split 0 0 0 0 0 0 " + S),
    # N = 480 / 960 / 1200 (the bias table of k_gemm32p and k_gemm_split holds 960)
    ("N = 480", plan_query(131072, 240, 480), "dma 0 0 0 0 0 0 " + P),
    ("N = 960", plan_query(131072, 240, 960), "dma 0 0 0 0 0 0 " + P),
    ("N = 1200", plan_query(131072, 240, 1200), "wide_256x240 0 0 0 0 512 5 " + W543),
    ("split on, N = 960", plan_query(131072, 240, 960, split=1), "split 0 0 0 0 0 0 " + S),
    ("split on, N = 1200", plan_query(131072, 240, 1200, split=1), "wide_256x240 0 0 0 0 512 5 " + W543),
    # ldc / coff not a multiple of 4: no 16-byte stores
    ("split on, ldc 258", plan_query(1230432, 240, 240, split=1, ldc=258), "dma 0 0 0 0 0 0 " + P),
    ("split on, coff 2", plan_query(1230432, 240, 240, split=1, coff=2), "dma 0 0 0 0 0 0 " + P),
    ("k_gemm32w, ldc 130", plan_query(2456736, 128, 128, ldc=130), "narrow 8 0 1 0 19194 1 " + TH),
    ("residual: no persistent kernel", plan_query(131072, 240, 240, residual=1, split=1), "wide_256x240 0 0 0 0 512 1 " + W543),
    # squeeze-excite scale, both table forms, split kernel off and on
    ("se 3-int table", plan_query(615216, 480, 480, se=3), "dma 0 0 0 1 0 0 " + PSE),
    ("se 3-int table, split on", plan_query(615216, 480, 480, se=3, split=1), "split 0 0 0 1 0 0 " + SSE),
    ("se 3-int table, LDS-DMA off", plan_query(615216, 480, 480, se=3, dma=0), "invalid 0 0 0 0 0 0 gemm: a 3-int a_tab is only understood by k_gemm32p (gemm_se_rows() == 256)"),
    ("se 3-int table, relu", plan_query(615216, 480, 480, se=3, act=RELU), "invalid 0 0 0 0 0 0 gemm: a 3-int a_tab is only understood by k_gemm32p (gemm_se_rows() == 256)"),
    ("se 2-int table at 256 x 240 size", plan_query(615216, 480, 480, se=2), "wide_128x240 0 0 0 1 4807 2 " + W443 + "+se"),
    ("se 2-int table, split on", plan_query(615216, 480, 480, se=2, split=1), "split 0 0 0 1 0 0 " + SSE),
    ("se 2-int table, split on, ld_scale < K", plan_query(615216, 480, 480, se=2, split=1, ld_scale=240), "wide_128x240 0 0 0 1 4807 2 " + W443 + "+se"),
    ("se 2-int table, narrow size", plan_query(100000, 128, 128, se=2), "wide_128x128 0 0 0 1 782 1 " + W442 + "+se"),
    ("se 2-int table, narrow size, 8191 rows", plan_query(8191, 128, 128, se=2), "invalid 0 0 0 0 0 0 gemm: a_scale is only implemented for the wide tiles"),
    ("se 2-int table, K = 544", plan_query(615216, 544, 480, se=2), "invalid 0 0 0 0 0 0 gemm: a_scale needs K <= 512 and a row-tile table"),
    # the CTC head's three forms
    ("argmax, narrow kernel", plan_query(5000, 120, 6625, am=1), "argmax_narrow 8 0 1 0 40 52 gemm_ctc_fc"),
    ("argmax, 128 x 128 tile", plan_query(5000, 120, 6625, am=1, amw=2), "argmax_128x128 0 0 0 0 40 52 gemm_ctc_fc"),
    ("argmax, 256 x 240 tile", plan_query(5000, 120, 6625, am=1, amw=1), "argmax_256x240 0 0 0 0 20 28 gemm_ctc_fc"),
    # forced variants of rt_bench_gemm and their fallbacks
    ("variant 1", plan_query(131072, 240, 240, variant=1), "narrow 5 0 1 0 1024 3 " + TH),
    ("variant 1, K = N = 128: no k_gemm32w", plan_query(131072, 128, 128, variant=1), "narrow 8 0 1 0 1024 1 " + TH),
    ("variant 8", plan_query(131072, 240, 240, variant=8), "wide_128x128 0 0 0 0 1024 2 " + W442),
    ("variant 10", plan_query(131072, 240, 240, variant=10), "wide_128x240 0 0 0 0 1024 1 " + W443),
    ("variant 15: no LDS-DMA", plan_query(131072, 240, 240, variant=15), "wide_256x240 0 0 0 0 512 1 " + W543),
    ("variant 20", plan_query(131072, 120, 120, variant=20), "stream 8 8 0 0 1024 1 " + TH),
    ("variant 20, N = 240 -> narrow", plan_query(131072, 240, 240, variant=20), "narrow 5 0 1 0 1024 3 " + TH),
    ("variant 30", plan_query(131072, 240, 240, variant=30), "dma 0 0 0 0 0 0 " + P),
    ("variant 30, K = 96 -> 15", plan_query(131072, 96, 240, variant=30), "wide_256x240 0 0 0 0 512 1 " + W543),
    ("variant 40", plan_query(131072, 240, 240, variant=40), "split 0 0 0 0 0 0 " + S),
    ("variant 40, ldc 258 -> 30", plan_query(131072, 240, 240, variant=40, ldc=258), "dma 0 0 0 0 0 0 " + P),
    ("variant 40, K = 96 -> 30 -> 15", plan_query(131072, 96, 240, variant=40), "wide_256x240 0 0 0 0 512 1 " + W543),
    ("variant 15 with a_scale -> 10", plan_query(131072, 240, 240, variant=15, se=2), "wide_128x240 0 0 0 1 1024 1 " + W443 + "+se"),
    ("variant 0 with a_scale -> 8", plan_query(131072, 128, 128, se=2), "wide_128x128 0 0 0 1 1024 1 " + W442 + "+se"),
    ("variant 1 with a_scale", plan_query(131072, 240, 240, variant=1, se=2), "invalid 0 0 0 0 0 0 gemm: a_scale is only implemented for the wide tiles"),
    ("no rows", plan_query(0, 240, 240), "none 0 0 0 0 0 0 gemm_pw/none"),
]

SE_TABLE = [  # (what it pins, query, row-table height)
    ("k_gemm32p size", se_query(615216, 480, 480), 256),
    ("k_gemm32p size, split on: the fp32 kernels' form", se_query(615216, 480, 480, split=1), 256),
    ("k_gemm32p size, LDS-DMA off", se_query(615216, 480, 480, dma=0), 128),
    ("K = 512", se_query(615216, 512, 480), 256),
    ("K = 544", se_query(615216, 544, 480), 0),
    ("K = 96 at 256 x 240 size", se_query(615216, 96, 480), 128),
    ("128 x 240 size", se_query(65409, 240, 240), 128),
    ("narrow size, 8191 rows", se_query(8191, 128, 128), 0),
    ("narrow size, 8192 rows", se_query(8192, 128, 128), 128),
    ("narrow size, N = 96", se_query(100000, 96, 96), 0),
    ("an image of 127 rows", se_query(615216, 480, 480, min_pix=127), 0),
    ("images of 128 rows", se_query(615216, 480, 480, min_pix=128), 256),
    ("relu epilogue", se_query(615216, 480, 480, act=RELU), 128),
    ("forced variant", se_query(615216, 480, 480, variant=30), 0),
]


def test_plan_table(driver):
    got = _run(driver, [q for _, q, _ in PLAN_TABLE])
    bad = ["%s: %s, expected %s" % (what, g, want) for (what, _, want), g in zip(PLAN_TABLE, got) if g != want]
    assert not bad, "\n".join(bad)
    kernels = {g.split()[0] for g in got}
    assert kernels == {"none", "invalid", "split", "w", "dma", "wide_256x240", "wide_128x240", "wide_128x128", "stream", "narrow",
                       "argmax_256x240", "argmax_128x128", "argmax_narrow"}


def test_se_row_table_form(driver):
    got = _run(driver, [q for _, q, _ in SE_TABLE])
    bad = ["%s: %s, expected %d" % (what, g, want) for (what, _, want), g in zip(SE_TABLE, got) if int(g) != want]
    assert not bad, "\n".join(bad)


def test_environment_switches(driver):
    """RT_GEMM_MID=0: the 128 x 240 tile from 16384 rows; RT_GEMM_W=0: no k_gemm32w; RT_GEMM_OCC / RT_GEMM_BF: the narrow kernel."""
    q = [plan_query(16384, 480, 480), plan_query(65536, 128, 128), plan_query(3600, 480, 480)]
    assert _run(driver, q, {"RT_GEMM_MID": "0"})[0] == "wide_128x240 0 0 0 0 128 2 " + W443
    assert _run(driver, q, {"RT_GEMM_W": "0"})[1] == "narrow 8 0 1 0 512 1 " + TH
    assert _run(driver, q, {"RT_GEMM_OCC": "1", "RT_GEMM_BF": "0"})[2] == "narrow 3 0 0 0 29 10 " + TH
    split_q = [plan_query(131072, 240, 240, split=1), plan_query(615216, 480, 480, se=3, split=1)]
    assert [g.split()[0] for g in _run(driver, split_q, {"RT_GS_ONLY": "1"})] == ["split", "dma"]
    assert [g.split()[0] for g in _run(driver, split_q, {"RT_GS_ONLY": "2"})] == ["dma", "split"]


def _pointwise_layers():
    """(M, K, N, se, min_pix) of every pointwise GEMM the work model prices for C3 (32 pages of 960 x 960, 1024 lines) and C4-like
    mixed pages and line widths (C5 runs the fp16 networks: no fp32 pointwise GEMMs)."""
    seen = []
    orig = workmodel.gemm_pw_label

    def rec(M, K, N, se=False, min_pix=1 << 30):
        seen.append((M, K, N, se, min_pix))
        return orig(M, K, N, se, min_pix)

    workmodel.gemm_pw_label = rec
    try:
        workmodel.det_work([(960, 960)] * 32)
        workmodel.rec_work([320] * 1024)
        workmodel.det_work([(640, 640), (960, 960), (736, 1280), (1088, 1920), (1760, 1248), (3520, 2496), (960, 960), (640, 640)])
        workmodel.rec_work([96, 160, 320, 480, 800, 1280, 3648] * 40 + [320] * 600)
        workmodel.rec_work([320, 480])
        workmodel.det_work([(960, 960)])
    finally:
        workmodel.gemm_pw_label = orig
    return sorted(set(seen))


def test_workmodel_labels_match_the_plan(driver):
    layers = _pointwise_layers()
    labels = [workmodel.gemm_pw_label(*l) for l in layers]
    assert len(layers) > 30 and GW in labels and PSE in labels and P in labels
    # nets.cpp run_lc: the row-table form first (gemm_se_rows), then the plan of the call it builds
    se_layers = [l for l in layers if l[3]]
    rows = dict(zip(se_layers, (int(g) for g in _run(driver, [se_query(M, K, N, min_pix=mp) for M, K, N, _, mp in se_layers]))))
    plans = _run(driver, [plan_query(M, (K + 3) // 4 * 4, N, se={256: 3, 128: 2}.get(rows.get(l, 0), 0))
                          for l in layers for M, K, N, _, _ in [l]])
    bad = ["%s: plan %s, work model %s" % (l, p.split(" ", 7)[7], lab) for l, p, lab in zip(layers, plans, labels) if p.split(" ", 7)[7] != lab]
    assert not bad, "\n".join(bad)
