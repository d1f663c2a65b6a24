"""The kernels of an LCNetV3 block (retto_amd/csrc/lc_plan.cpp: nn::dw_plan, nn::lc_plan) on the host: a pinned table of shapes ->
(route, kernel instance, tile rows, grid, strip layout), and the work model's mirror (retto_amd/workmodel.py lc_thin_fused) against
the plan.  The expected column was read off the decision functions the plan replaced (lc_route / lc_thin / lc_wave and
dw_strip_rows / dw_lanes_per_pixel / dw_sweep_form / dwconv / dwconv_pool_layout of nn_kernels.hip and nn_lcwave.hip, and run_lc's
squeeze-excite rule), not off the plan.  Compiled with g++ into tests/native/gemm_plan_driver.cpp (tests/plan_driver.py): no GPU.

Answers: "thin | wave | lds <instance> <tile rows> <grid_x>" or "unfused <squeeze-excite table rows, 0: not folded> <dw answer>";
dw answer: "<rows32 | rows64 | sweep> <sweep instance> <strip rows R> <lanes per pixel> <strips per block> <chunks> <grid_x> <grid_z>"."""
import pytest

import plan_driver
from retto_amd import synth, workmodel

NONE, RELU, HSWISH = 0, 1, 2
SWITCHES = [(3, 4), (1, 4), (0, 4), (3, 0), (1, 0), (0, 0)]   # (g_lc_wave, g_dw_sweep)


def _pitch(c):
    return (c + 31) // 32 * 32 if c >= 128 else (c + 3) // 4 * 4


def dw_q(K, sh, sw, Cp, maxHo, maxWo, pooled=0, sweep=4):
    return "dw %d %d %d %d %d %d %d %d" % (sweep, K, sh, sw, Cp, maxHo, maxWo, pooled)


def lc_q(K, sh, sw, cin, cout, maxHo, maxWo, n=1, se=0, lc_wave=3, sweep=4, Cp=None, npad=None, dw_tail=None, pw_act=HSWISH, pw_lab=1,
         bias=1, min_pix=None):
    """A block as run_lc plans it: Cp = chan_pitch(cin), Npad16 = cout rounded to 16, n images of maxHo x maxWo output pixels; the
    depthwise tail of the LCNetV3 blocks (hardswish + LAB unless the stride is (2, 2)) unless dw_tail = (act, has_lab) is given."""
    Cp = _pitch(cin) if Cp is None else Cp
    npad = (cout + 15) // 16 * 16 if npad is None else npad
    act, lab = dw_tail if dw_tail is not None else ((NONE, 0) if (sh, sw) == (2, 2) else (HSWISH, 1))
    pix = maxHo * maxWo
    return "lc %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (
        lc_wave, sweep, K, sh, sw, Cp, cin, cout, npad, act, lab, se, maxHo, maxWo, n * pix, pix if min_pix is None else min_pix,
        pw_act, pw_lab, bias)


def net_blocks():
    """(what, lc_q keyword arguments) of every LCNetV3 block of the det net on a 960 x 960 page and of the rec net on a 48-high line
    of width 8, 320 and 3200, and of the squeeze-excite blocks on the 32 pages of a launch group and on 1024 lines of 320."""
    out = []
    for net, blocks, H, W, n in [("det", synth.DET_BLOCKS, 960, 960, 1), ("det", synth.DET_BLOCKS, 960, 960, 32),
                                 ("rec", synth.REC_BLOCKS, 48, 8, 1), ("rec", synth.REC_BLOCKS, 48, 320, 1),
                                 ("rec", synth.REC_BLOCKS, 48, 3200, 1), ("rec", synth.REC_BLOCKS, 48, 320, 1024)]:
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1   # the stem has stride 2
        for name, k, cin, cout, sh, sw, se in blocks:
            h, w = (h - 1) // sh + 1, (w - 1) // sw + 1
            if n > 1 and not se:   # (the batch moves the squeeze-excite form only)
                continue
            out.append(("%s %s, %d x %d x %d" % (net, name, n, H, W), dict(K=k, sh=sh, sw=sw, cin=cin, cout=cout, maxHo=h, maxWo=w, n=n, se=int(se))))
    return out


EDGES = [  # (what it pins, query, the driver's answer)
    # the pointwise epilogue: k_lc_lds / k_lc_wave need bias + hardswish + LAB
    ("64 -> 64 without the pointwise LAB: k_lc_thin", lc_q(3, 1, 1, 64, 64, 24, 160, pw_lab=0), "thin 4 4 8"),
    ("(2, 1) 64 -> 128 without the pointwise LAB: no k_lc_thin instance", lc_q(3, 2, 1, 64, 128, 12, 160, pw_lab=0), "unfused 0 rows32 0 2 8 32 8 8 2"),
    ("64 -> 64 with a relu epilogue", lc_q(3, 1, 1, 64, 64, 24, 160, pw_act=RELU), "thin 4 4 8"),
    ("64 -> 64 without a bias", lc_q(3, 1, 1, 64, 64, 24, 160, bias=0), "thin 4 4 8"),
    ("64 -> 64, depthwise tail without the LAB", lc_q(3, 1, 1, 64, 64, 24, 160, dw_tail=(HSWISH, 0)), "thin 4 4 8"),
    ("(2, 2) 32 -> 48 with a depthwise activation", lc_q(3, 2, 2, 32, 48, 240, 240, dw_tail=(HSWISH, 1)), "thin 6 4 113"),
    ("a 5x5 block of 64 channels", lc_q(5, 1, 1, 64, 64, 24, 160), "unfused 0 rows32 0 4 8 32 8 8 2"),
    ("64 -> 64 with a squeeze-excite", lc_q(3, 1, 1, 64, 64, 24, 160, se=1, n=64), "unfused 0 rows32 0 4 8 32 8 8 2"),
    # Cp != C, N != Npad16
    ("63 of 64 channels: k_lc_thin", lc_q(3, 1, 1, 63, 64, 24, 160), "thin 4 4 8"),
    ("60 channels on pitch 64 (Cp != round_up(C, 4)): the unfused pair", lc_q(3, 1, 1, 60, 64, 24, 160, Cp=64), "unfused 0 rows32 0 4 8 32 8 8 2"),
    ("64 -> 60 (N != Npad16): k_lc_thin", lc_q(3, 1, 1, 64, 60, 24, 160), "thin 4 4 8"),
    ("32 -> 48 at stride 1: k_lc_thin only", lc_q(3, 1, 1, 32, 48, 24, 160), "thin 2 8 4"),
    ("48 -> 80 at stride (2, 2): k_lc_thin only", lc_q(3, 2, 2, 48, 80, 120, 120, dw_tail=(NONE, 0)), "thin 7 4 30"),
    # 32-bit image offsets of k_lc_lds / k_lc_wave: images below 1 GB, input (with halo) and output
    ("16 -> 32, output image one row below 1 GB", lc_q(3, 1, 1, 16, 32, 2047, 4096), "lds 1 4 8192"),
    ("16 -> 32, output image of 1 GB", lc_q(3, 1, 1, 16, 32, 2048, 4096), "thin 1 8 8192"),
    ("64 -> 64, input image with halo below 1 GB", lc_q(3, 1, 1, 64, 64, 1021, 4094), "lds 4 4 4096"),
    ("64 -> 64, input image with halo of 1 GB", lc_q(3, 1, 1, 64, 64, 1022, 4094), "thin 4 4 8192"),
    ("16 -> 32 at 1 GB, direct-load form asked for", lc_q(3, 1, 1, 16, 32, 2048, 4096, lc_wave=1), "thin 1 8 8192"),
    # column sweep: at most 24 input rows
    ("5x5 stride 1, 24 rows", dw_q(5, 1, 1, 256, 24, 800), "sweep 1 4 16 16 75 13 4"),
    ("5x5 stride 1, 25 rows", dw_q(5, 1, 1, 256, 25, 800), "rows64 0 4 16 16 88 88 4"),
    ("5x5 stride (2, 1), 12 output rows = 24 input rows", dw_q(5, 2, 1, 256, 12, 800), "sweep 4 2 16 16 75 13 4"),
    ("5x5 stride (2, 1), 13 output rows", dw_q(5, 2, 1, 256, 13, 800), "rows64 0 2 16 16 88 88 4"),
    ("3x3 stride (1, 2), 24 rows", dw_q(3, 1, 2, 128, 24, 800), "sweep 6 4 16 16 75 13 2"),
    ("3x3 stride (1, 2), 25 rows", dw_q(3, 1, 2, 128, 25, 800), "rows64 0 4 16 16 88 88 2"),
    # ... and its lower height bounds
    ("5x5 stride 1, 5 rows", dw_q(5, 1, 1, 256, 5, 800), "sweep 1 4 16 16 25 13 4"),
    ("5x5 stride 1, 4 rows", dw_q(5, 1, 1, 256, 4, 800), "rows64 0 4 16 16 13 13 4"),
    ("3x3 stride 1, 4 rows", dw_q(3, 1, 1, 128, 4, 800), "sweep 2 4 16 16 13 13 2"),
    ("3x3 stride 1, 3 rows: 3-row strips, 32-channel slabs", dw_q(3, 1, 1, 128, 3, 800), "rows32 0 3 8 32 7 7 4"),
    ("3x3 stride 1, 2 rows", dw_q(3, 1, 1, 128, 2, 800), "rows64 0 4 16 16 13 13 2"),
    ("5x5 stride (2, 1), 3 output rows", dw_q(5, 2, 1, 480, 3, 800), "sweep 4 2 16 16 25 13 8"),
    ("5x5 stride (2, 1), 2 output rows", dw_q(5, 2, 1, 480, 2, 800), "rows64 0 2 16 16 13 13 8"),
    ("3x3 stride (1, 2), 4 rows", dw_q(3, 1, 2, 128, 4, 800), "sweep 6 4 16 16 13 13 2"),
    ("3x3 stride (1, 2), 2 rows", dw_q(3, 1, 2, 128, 2, 800), "rows64 0 4 16 16 13 13 2"),
    ("5x5 stride (2, 2): no sweep instance", dw_q(5, 2, 2, 384, 12, 800), "rows64 0 2 16 16 75 75 6"),
    # pooled sweep: 3-row strips only, at most DW_SWEEP_POOL_STRIPS = 4 of them in a column (3-row strips come with 3 and 6 rows only,
    # so the strip limit never binds; maps of 4 and of 5 strips run on the row kernel either way)
    ("pooled 5x5, 6 rows", dw_q(5, 1, 1, 480, 6, 800, pooled=1), "sweep 3 3 16 16 25 13 8"),
    ("pooled 5x5, 3 rows: below the sweep's 5", dw_q(5, 1, 1, 480, 3, 800, pooled=1), "rows64 0 3 16 16 13 13 8"),
    ("pooled 5x5, 12 rows = 4 strips of 3 but 4-row strips", dw_q(5, 1, 1, 480, 12, 800, pooled=1), "rows64 0 4 16 16 38 38 8"),
    ("pooled 5x5, 15 rows = 5 strips of 3 but 4-row strips", dw_q(5, 1, 1, 480, 15, 800, pooled=1), "rows64 0 4 16 16 50 50 8"),
    ("pooled 5x5 stride (2, 1), 6 output rows", dw_q(5, 2, 1, 256, 6, 800, pooled=1), "sweep 5 3 16 16 25 13 4"),
    ("pooled 5x5 stride (2, 1), 3 output rows: 2-row strips", dw_q(5, 2, 1, 256, 3, 800, pooled=1), "rows64 0 2 16 16 25 25 4"),
    ("pooled 5x5 stride (2, 1), 12 output rows", dw_q(5, 2, 1, 256, 12, 800, pooled=1), "rows64 0 2 16 16 75 75 4"),
    ("pooled 5x5, 6 rows, sweep off", dw_q(5, 1, 1, 480, 6, 800, pooled=1, sweep=0), "rows64 0 3 16 16 25 25 8"),
    # strip rows R: maps of 6 and of 3 rows
    ("stride 1, 6 rows", dw_q(5, 1, 1, 96, 6, 203), "rows32 0 3 8 32 4 4 3"),
    ("stride 1, 3 rows", dw_q(5, 1, 1, 96, 3, 203), "rows32 0 3 8 32 2 2 3"),
    ("stride 1, 5 rows", dw_q(5, 1, 1, 96, 5, 203), "rows32 0 4 8 32 4 4 3"),
    ("stride 2, 6 rows", dw_q(5, 2, 2, 96, 6, 203), "rows32 0 3 8 32 4 4 3"),
    ("stride 2, 3 rows: 2-row strips", dw_q(5, 2, 2, 96, 3, 203), "rows32 0 2 8 32 4 4 3"),
    ("stride 2, 6 rows, 384 channels: no 64-channel instance with 3-row strips", dw_q(5, 2, 2, 384, 6, 203), "rows32 0 3 8 32 4 4 12"),
    ("stride 2, 7 rows, 384 channels", dw_q(5, 2, 2, 384, 7, 203), "rows64 0 2 16 16 13 13 6"),
    # 64-channel slabs: from 192 channels (5x5) and 128 channels (3x3)
    ("5x5, 192 channels", dw_q(5, 1, 1, 192, 30, 30), "rows64 0 4 16 16 4 4 3"),
    ("5x5, 188 channels", dw_q(5, 1, 1, 188, 30, 30), "rows32 0 4 8 32 2 2 6"),
    ("5x5 stride (1, 2), 192 channels: no instance", dw_q(5, 1, 2, 192, 30, 30), "rows32 0 4 8 32 2 2 6"),
    ("3x3, 128 channels", dw_q(3, 1, 1, 128, 30, 30), "rows64 0 4 16 16 4 4 2"),
    ("3x3, 124 channels", dw_q(3, 1, 1, 124, 30, 30), "rows32 0 4 8 32 2 2 4"),
    ("3x3 stride (2, 1), 128 channels: no instance", dw_q(3, 2, 1, 128, 30, 30), "rows32 0 2 8 32 4 4 4"),
    ("pooled 3x3, 128 channels: 32-channel slabs", dw_q(3, 1, 1, 128, 30, 30, pooled=1), "rows32 0 4 8 32 2 2 4"),
    ("pooled 3x3, 12 rows: no sweep", dw_q(3, 1, 1, 128, 12, 800, pooled=1), "rows32 0 4 8 32 19 19 4"),
    ("7x7: no kernel", dw_q(7, 1, 1, 128, 30, 30), "invalid 0 0 0 0 0 0 0"),
    # the squeeze-excite form: every image must cover a 128-row block
    ("rec s6.1, lines of 127 pixels", lc_q(5, 1, 1, 480, 480, 6, 160, n=1024, se=1, min_pix=127), "unfused 0 sweep 1 3 16 16 5 3 8"),
    ("rec s6.1, lines of 128 pixels", lc_q(5, 1, 1, 480, 480, 6, 160, n=1024, se=1, min_pix=128), "unfused 256 sweep 3 3 16 16 5 3 8"),
    ("rec s6.1, LDS-DMA size, sweep off", lc_q(5, 1, 1, 480, 480, 6, 160, n=1024, se=1, sweep=0), "unfused 256 rows64 0 3 16 16 5 5 8"),
    ("det s6.1 on one page: no folded form", lc_q(5, 1, 1, 384, 384, 30, 30, n=1, se=1), "unfused 0 rows64 0 4 16 16 4 4 6"),
]
NET_EXPECTED = [  # per block of net_blocks(): the answers under SWITCHES; "=": as the entry before it
    ("lds 1 4 225", "wave 1 2 450", "thin 1 8 225", "lds 1 4 225", "wave 1 2 450", "thin 1 8 225"),   # det s2.0, 1 x 960 x 960
    ("lds 6 2 113", "=", "thin 6 4 113", "lds 6 2 113", "=", "thin 6 4 113"),   # det s3.0, 1 x 960 x 960
    ("lds 3 4 57", "wave 3 2 113", "thin 3 4 113", "lds 3 4 57", "wave 3 2 113", "thin 3 4 113"),   # det s3.1, 1 x 960 x 960
    ("lds 7 2 30", "=", "thin 7 4 30", "lds 7 2 30", "=", "thin 7 4 30"),   # det s4.0, 1 x 960 x 960
    ("unfused 0 rows32 0 4 8 32 29 29 3", "=", "=", "=", "=", "="),   # det s4.1, 1 x 960 x 960
    ("unfused 0 rows32 0 2 8 32 15 15 3", "=", "=", "=", "=", "="),   # det s5.0, 1 x 960 x 960
    ("unfused 0 rows64 0 4 16 16 15 15 3", "=", "=", "=", "=", "="),   # det s5.1, 1 x 960 x 960
    ("unfused 0 rows64 0 4 16 16 15 15 3", "=", "=", "=", "=", "="),   # det s5.2, 1 x 960 x 960
    ("unfused 0 rows64 0 4 16 16 15 15 3", "=", "=", "=", "=", "="),   # det s5.3, 1 x 960 x 960
    ("unfused 0 rows64 0 4 16 16 15 15 3", "=", "=", "=", "=", "="),   # det s5.4, 1 x 960 x 960
    ("unfused 0 rows64 0 2 16 16 8 8 3", "=", "=", "=", "=", "="),   # det s6.0, 1 x 960 x 960
    ("unfused 0 rows64 0 4 16 16 4 4 6", "=", "=", "=", "=", "="),   # det s6.1, 1 x 960 x 960
    ("unfused 0 rows64 0 4 16 16 4 4 6", "=", "=", "=", "=", "="),   # det s6.2, 1 x 960 x 960
    ("unfused 0 rows64 0 4 16 16 4 4 6", "=", "=", "=", "=", "="),   # det s6.3, 1 x 960 x 960
    ("unfused 128 rows64 0 2 16 16 8 8 3", "=", "=", "=", "=", "="),   # det s6.0, 32 x 960 x 960
    ("unfused 128 rows64 0 4 16 16 4 4 6", "=", "=", "=", "=", "="),   # det s6.1, 32 x 960 x 960
    ("lds 1 4 1", "wave 1 2 1", "thin 1 8 1", "lds 1 4 1", "wave 1 2 1", "thin 1 8 1"),   # rec s2.0, 1 x 48 x 8
    ("lds 2 4 1", "wave 2 2 1", "thin 2 8 1", "lds 2 4 1", "wave 2 2 1", "thin 2 8 1"),   # rec s3.0, 1 x 48 x 8
    ("lds 4 4 1", "wave 4 2 1", "thin 4 4 1", "lds 4 4 1", "wave 4 2 1", "thin 4 4 1"),   # rec s3.1, 1 x 48 x 8
    ("lds 8 2 1", "=", "unfused 0 rows32 0 2 8 32 1 1 2", "lds 8 2 1", "=", "unfused 0 rows32 0 2 8 32 1 1 2"),   # rec s4.0, 1 x 48 x 8
    ("unfused 0 sweep 2 4 16 16 1 1 2", "=", "=", "unfused 0 rows64 0 4 16 16 1 1 2", "=", "="),   # rec s4.1, 1 x 48 x 8
    ("unfused 0 sweep 6 4 16 16 1 1 2", "=", "=", "unfused 0 rows64 0 4 16 16 1 1 2", "=", "="),   # rec s5.0, 1 x 48 x 8
    ("unfused 0 sweep 1 4 16 16 1 1 4", "=", "=", "unfused 0 rows64 0 4 16 16 1 1 4", "=", "="),   # rec s5.1, 1 x 48 x 8
    ("unfused 0 sweep 1 4 16 16 1 1 4", "=", "=", "unfused 0 rows64 0 4 16 16 1 1 4", "=", "="),   # rec s5.2, 1 x 48 x 8
    ("unfused 0 sweep 1 4 16 16 1 1 4", "=", "=", "unfused 0 rows64 0 4 16 16 1 1 4", "=", "="),   # rec s5.3, 1 x 48 x 8
    ("unfused 0 sweep 1 4 16 16 1 1 4", "=", "=", "unfused 0 rows64 0 4 16 16 1 1 4", "=", "="),   # rec s5.4, 1 x 48 x 8
    ("unfused 0 sweep 4 3 16 16 1 1 4", "=", "=", "unfused 0 rows64 0 3 16 16 1 1 4", "=", "="),   # rec s6.0, 1 x 48 x 8
    ("unfused 0 sweep 1 3 16 16 1 1 8", "=", "=", "unfused 0 rows64 0 3 16 16 1 1 8", "=", "="),   # rec s6.1, 1 x 48 x 8
    ("unfused 0 sweep 4 2 16 16 1 1 8", "=", "=", "unfused 0 rows64 0 2 16 16 1 1 8", "=", "="),   # rec s6.2, 1 x 48 x 8
    ("unfused 0 rows64 0 3 16 16 1 1 8", "=", "=", "=", "=", "="),   # rec s6.3, 1 x 48 x 8
    ("lds 1 4 4", "wave 1 2 8", "thin 1 8 4", "lds 1 4 4", "wave 1 2 8", "thin 1 8 4"),   # rec s2.0, 1 x 48 x 320
    ("lds 2 4 4", "wave 2 2 8", "thin 2 8 4", "lds 2 4 4", "wave 2 2 8", "thin 2 8 4"),   # rec s3.0, 1 x 48 x 320
    ("lds 4 4 4", "wave 4 2 8", "thin 4 4 8", "lds 4 4 4", "wave 4 2 8", "thin 4 4 8"),   # rec s3.1, 1 x 48 x 320
    ("lds 8 2 4", "=", "unfused 0 rows32 0 2 8 32 8 8 2", "lds 8 2 4", "=", "unfused 0 rows32 0 2 8 32 8 8 2"),   # rec s4.0, 1 x 48 x 320
    ("unfused 0 sweep 2 4 16 16 8 3 2", "=", "=", "unfused 0 rows64 0 4 16 16 8 8 2", "=", "="),   # rec s4.1, 1 x 48 x 320
    ("unfused 0 sweep 6 4 16 16 4 2 2", "=", "=", "unfused 0 rows64 0 4 16 16 4 4 2", "=", "="),   # rec s5.0, 1 x 48 x 320
    ("unfused 0 sweep 1 4 16 16 4 2 4", "=", "=", "unfused 0 rows64 0 4 16 16 4 4 4", "=", "="),   # rec s5.1, 1 x 48 x 320
    ("unfused 0 sweep 1 4 16 16 4 2 4", "=", "=", "unfused 0 rows64 0 4 16 16 4 4 4", "=", "="),   # rec s5.2, 1 x 48 x 320
    ("unfused 0 sweep 1 4 16 16 4 2 4", "=", "=", "unfused 0 rows64 0 4 16 16 4 4 4", "=", "="),   # rec s5.3, 1 x 48 x 320
    ("unfused 0 sweep 1 4 16 16 4 2 4", "=", "=", "unfused 0 rows64 0 4 16 16 4 4 4", "=", "="),   # rec s5.4, 1 x 48 x 320
    ("unfused 0 sweep 4 3 16 16 3 2 4", "=", "=", "unfused 0 rows64 0 3 16 16 3 3 4", "=", "="),   # rec s6.0, 1 x 48 x 320
    ("unfused 0 sweep 1 3 16 16 3 2 8", "=", "=", "unfused 0 rows64 0 3 16 16 3 3 8", "=", "="),   # rec s6.1, 1 x 48 x 320
    ("unfused 0 sweep 4 2 16 16 3 2 8", "=", "=", "unfused 0 rows64 0 2 16 16 3 3 8", "=", "="),   # rec s6.2, 1 x 48 x 320
    ("unfused 0 rows64 0 3 16 16 2 2 8", "=", "=", "=", "=", "="),   # rec s6.3, 1 x 48 x 320
    ("lds 1 4 38", "wave 1 2 75", "thin 1 8 38", "lds 1 4 38", "wave 1 2 75", "thin 1 8 38"),   # rec s2.0, 1 x 48 x 3200
    ("lds 2 4 38", "wave 2 2 75", "thin 2 8 38", "lds 2 4 38", "wave 2 2 75", "thin 2 8 38"),   # rec s3.0, 1 x 48 x 3200
    ("lds 4 4 38", "wave 4 2 75", "thin 4 4 75", "lds 4 4 38", "wave 4 2 75", "thin 4 4 75"),   # rec s3.1, 1 x 48 x 3200
    ("lds 8 2 38", "=", "unfused 0 rows32 0 2 8 32 75 75 2", "lds 8 2 38", "=", "unfused 0 rows32 0 2 8 32 75 75 2"),   # rec s4.0, 1 x 48 x 3200
    ("unfused 0 sweep 2 4 16 16 75 25 2", "=", "=", "unfused 0 rows64 0 4 16 16 75 75 2", "=", "="),   # rec s4.1, 1 x 48 x 3200
    ("unfused 0 sweep 6 4 16 16 38 13 2", "=", "=", "unfused 0 rows64 0 4 16 16 38 38 2", "=", "="),   # rec s5.0, 1 x 48 x 3200
    ("unfused 0 sweep 1 4 16 16 38 13 4", "=", "=", "unfused 0 rows64 0 4 16 16 38 38 4", "=", "="),   # rec s5.1, 1 x 48 x 3200
    ("unfused 0 sweep 1 4 16 16 38 13 4", "=", "=", "unfused 0 rows64 0 4 16 16 38 38 4", "=", "="),   # rec s5.2, 1 x 48 x 3200
    ("unfused 0 sweep 1 4 16 16 38 13 4", "=", "=", "unfused 0 rows64 0 4 16 16 38 38 4", "=", "="),   # rec s5.3, 1 x 48 x 3200
    ("unfused 0 sweep 1 4 16 16 38 13 4", "=", "=", "unfused 0 rows64 0 4 16 16 38 38 4", "=", "="),   # rec s5.4, 1 x 48 x 3200
    ("unfused 0 sweep 4 3 16 16 25 13 4", "=", "=", "unfused 0 rows64 0 3 16 16 25 25 4", "=", "="),   # rec s6.0, 1 x 48 x 3200
    ("unfused 0 sweep 1 3 16 16 25 13 8", "=", "=", "unfused 0 rows64 0 3 16 16 25 25 8", "=", "="),   # rec s6.1, 1 x 48 x 3200
    ("unfused 0 sweep 4 2 16 16 25 13 8", "=", "=", "unfused 0 rows64 0 2 16 16 25 25 8", "=", "="),   # rec s6.2, 1 x 48 x 3200
    ("unfused 0 rows64 0 3 16 16 13 13 8", "=", "=", "=", "=", "="),   # rec s6.3, 1 x 48 x 3200
    ("unfused 256 sweep 5 3 16 16 3 2 4", "=", "=", "unfused 256 rows64 0 3 16 16 3 3 4", "=", "="),   # rec s6.0, 1024 x 48 x 320
    ("unfused 256 sweep 3 3 16 16 3 2 8", "=", "=", "unfused 256 rows64 0 3 16 16 3 3 8", "=", "="),   # rec s6.1, 1024 x 48 x 320
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return plan_driver.build(tmp_path_factory)


def test_edges(driver):
    got = plan_driver.run(driver, [q for _, q, _ in EDGES])
    bad = ["%s: %s, expected %s" % (what, g, want) for (what, _, want), g in zip(EDGES, got) if g != want]
    assert not bad, "\n".join(bad)


def test_network_blocks_under_every_switch(driver):
    blocks = net_blocks()
    assert len(blocks) == len(NET_EXPECTED) == 4 * 14 + 2 * 2
    queries, want = [], []
    for (what, kw), row in zip(blocks, NET_EXPECTED):
        assert len(row) == len(SWITCHES)
        for i, (lw, ds) in enumerate(SWITCHES):
            queries.append(lc_q(lc_wave=lw, sweep=ds, **kw))
            want.append((what, lw, ds, want[-1][3] if row[i] == "=" else row[i]))
    got = plan_driver.run(driver, queries)
    bad = ["%s (lc_wave %d, dw_sweep %d): %s, expected %s" % (w[0], w[1], w[2], g, w[3]) for w, g in zip(want, got) if g != w[3]]
    assert not bad, "\n".join(bad)
    # every route, every depthwise kernel and both squeeze-excite table forms occur
    assert {g.split()[0] for g in got} == {"thin", "wave", "lds", "unfused"}
    assert {g.split()[2] for g in got if g.startswith("unfused")} == {"rows32", "rows64", "sweep"}
    assert {g.split()[1] for g in got if g.startswith("unfused")} == {"0", "128", "256"}


def test_environment_switches(driver):
    """RT_LC_WAVE and RT_DW_SWEEP are read once, when the library loads; a query with switch -1 keeps what they selected."""
    q = [lc_q(3, 1, 1, 64, 64, 24, 160, lc_wave=-1, sweep=-1), lc_q(5, 1, 1, 240, 240, 12, 800, lc_wave=-1, sweep=-1)]
    assert plan_driver.run(driver, q) == ["lds 4 4 4", "unfused 0 sweep 1 4 16 16 38 13 4"]
    assert plan_driver.run(driver, q, {"RT_LC_WAVE": "1"})[0] == "wave 4 2 8"
    assert plan_driver.run(driver, q, {"RT_LC_WAVE": "0"})[0] == "thin 4 4 8"
    assert plan_driver.run(driver, q, {"RT_DW_SWEEP": "0"})[1] == "unfused 0 rows64 0 4 16 16 38 38 4"


@pytest.mark.parametrize("lc_wave", [None, "0", "1"])
def test_workmodel_mirror_matches_the_plan(driver, monkeypatch, lc_wave):
    """workmodel.lc_thin_fused() == the plan takes a fused route, for every block of both networks."""
    if lc_wave is None:
        monkeypatch.delenv("RT_LC_WAVE", raising=False)
    else:
        monkeypatch.setenv("RT_LC_WAVE", lc_wave)
    blocks = [(name, kw) for name, kw in net_blocks() if kw["n"] == 1]
    got = plan_driver.run(driver, [lc_q(lc_wave=-1, sweep=-1, **kw) for _, kw in blocks])   # (run() passes os.environ on)
    for (name, kw), g in zip(blocks, got):
        mirror = workmodel.lc_thin_fused(kw["K"], kw["sh"], kw["sw"], kw["cin"], kw["cout"], bool(kw["se"]))
        assert mirror == (g.split()[0] != "unfused"), "%s under RT_LC_WAVE=%s: work model %s, plan %s" % (name, lc_wave, mirror, g)
    assert sum(g.split()[0] != "unfused" for g in got) == (4 + 3 * 4 if lc_wave != "0" else 4 + 3 * 3)
