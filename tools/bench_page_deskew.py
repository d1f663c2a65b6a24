"""Cost of page deskew (rt_set_page_deskew) on the C3 pages: 32 seeded synthetic pages of 960 x 960 with 32 planted lines each,
slanted by 12 / 512, resident in HBM, the DB post-processing fed by planted maps in HBM (the det network still runs), one lane, so that a lane part is
all 32 pages and the four launches run once per call.

Settings: deskew off, range 16 and range 128 at min_gain 0 (so that a page whose best slope is not 0 is really turned; how many
pages were turned is reported).  Per setting, after warm-up calls, `--steps` profiled calls (per-launch HIP events on the lane's
stream, the calls serial), and per call the device time of `page_deskew_cells`, `page_deskew_profile`, `page_deskew_pick` and
`page_deskew_rotate`; reported: the median, min and max over the calls and the four medians' sum.  For scale: a device-to-device
hipMemcpyAsync of the pages' bytes (32 x 960 x 960 x 3), timed in the same run -- the floor for one read plus one write of the
pages, what cells and rotate are held against -- and, for the profile kernel, the bytes it reads from LDS, counted from the shapes
(pages x slopes x grid cells, one byte each), and the rate that time makes of them.  One JSON line on stdout.

    python tools/bench_page_deskew.py --steps 20 --warmup 5
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import retto_amd  # noqa: E402
from retto_amd import workload  # noqa: E402

SLOPE = 12   # of the bench pages, in 1 / 512: inside both ranges
SETTINGS = (("off", 0, 0), ("k16", 16, 0), ("k128", 128, 0))
FAMILIES = ("page_deskew_cells", "page_deskew_profile", "page_deskew_pick", "page_deskew_rotate")


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--size", type=int, default=960)
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    S, n = a.size, a.pages
    planted = [workload.planted_page(S, S, a.lines, seed=i) for i in range(n)]
    # dark lines on white paper (the planted pages are bright lines on black, which the rule reads as one block of ink), slanted
    # (a shear: column x moves up by SLOPE (x - S / 2) / 512 pixels, wrapping), so that rotate is not the copy
    shift = (SLOPE * (np.arange(S) - S // 2) + 256) // 512
    rows = (np.arange(S)[:, None] + shift[None, :]) % S
    planted = [(np.ascontiguousarray(255 - p[rows, np.arange(S)[None, :]]), rects) for p, rects in planted]
    result ={"tool": "bench_page_deskew", "pages": n, "page": [S, S], "lines": a.lines, "steps": a.steps, "warmup": a.warmup,
              "source_digest": retto_amd._lib.source_digest(), "settings": {}}
    s = retto_amd.RettoSession(retto_amd.synthetic_session_config(0, lanes=1))
    lib, h = s._hd.lib, s._hd.h
    dh, dw = C.c_int(), C.c_int()
    assert lib.rt_det_input_dims(h, S, S, C.byref(dh), C.byref(dw)) == 0
    pages = [upload(lib, h, p) for p, _ in planted]
    maps = [upload(lib, h, workload.planted_map(dh.value, dw.value, S, S, rects)) for _, rects in planted]
    cell = 4
    while -(-S // cell) > 512:
        cell *= 2
    grid_cells = (-(-S // cell)) ** 2

    def step():
        r = s.run_batch_raw(pages, [S] * n, [S] * n, retto_amd.RT_MEM_DEVICE, det_map_override=maps)
        lines = sum(lib.rt_results_count(r, i) for i in range(n))
        k = C.c_int(); turned = 0
        for i in range(n):
            lib.rt_results_page_deskew(r, i, C.byref(k), None)
            turned += k.value != 0
        lib.rt_results_free(r)
        return lines, turned

    try:
        ms = C.c_float()
        assert lib.rt_bench_memcpy_d2d(h, n * S * S * 3, 20, C.byref(ms)) == 0
        result["memcpy_d2d_ms"] = ms.value; result["memcpy_d2d_bytes"] = n * S * S * 3
        for name, K, gain in SETTINGS:
            s.set_page_deskew(K, gain)
            for _ in range(a.warmup):
                step()
            e = result["settings"][name] = {"range": K, "min_gain": gain}
            per_call = {fam: [] for fam in FAMILIES}
            for _ in range(a.steps):
                s.profile_enable(True)
                e["lines"], e["pages_turned"] = step()
                prof = s.profile_get()
                s.profile_enable(False)
                for fam in FAMILIES:
                    fam_ms, calls = prof.get(fam, (0.0, 0))
                    per_call[fam].append(fam_ms); e[fam + "_launches"] = calls
            for fam in FAMILIES:
                e[fam + "_ms"] = statistics.median(per_call[fam]); e[fam + "_ms_min"] = min(per_call[fam]); e[fam + "_ms_max"] = max(per_call[fam])
            e["sum_ms"] = sum(e[fam + "_ms"] for fam in FAMILIES)
            if K:
                e["cells_over_memcpy"] = e["page_deskew_cells_ms"] / ms.value
                e["rotate_over_memcpy"] = e["page_deskew_rotate_ms"] / ms.value
                e["profile_lds_bytes"] = n * (2 * K + 1) * grid_cells
                e["profile_lds_gbytes_per_s"] = e["profile_lds_bytes"] / (e["page_deskew_profile_ms"] * 1e-3) / 1e9
    finally:
        for p in pages + maps:
            lib.rt_device_free(h, p)
        s.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
