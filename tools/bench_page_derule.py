"""Cost of page derule (rt_set_page_derule) on the C3 pages: 32 seeded synthetic pages of 960 x 960 with 32 planted lines each, dark on
white, under a grid of 2-pixel rules every 60 pixels both ways, resident in HBM, the DB post-processing fed by planted maps in HBM
(the det network still runs), one lane, so that a lane part is all 32 pages and the seven launches run once per call.

Settings: derule off, min_len 64 and min_len 512 (max_thick 4, ink 96).  Per setting, after warm-up calls, `--steps` profiled calls
(per-launch HIP events on the lane's stream, the calls serial), and per call the device time of the families `page_derule_bits`
(two launches), `page_derule_hlong` (one), `page_derule_vsweep` (two) and `page_derule_fill` (two); reported: the median, min and
max over the calls, the medians' sum, and each family's median over the yardstick: a device-to-device hipMemcpyAsync of the pages'
bytes (32 x 960 x 960 x 3), timed in the same run -- one read plus one write of the pages.  One JSON line on stdout.

    python tools/bench_page_derule.py --steps 20 --warmup 5
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

SETTINGS = (("off", 0, 0, 0), ("l64", 64, 4, 96), ("l512", 512, 4, 96))
FAMILIES = ("page_derule_bits", "page_derule_hlong", "page_derule_vsweep", "page_derule_fill")


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
    planted = []
    for i in range(n):
        p, rects = workload.planted_page(S, S, a.lines, seed=i)
        p = np.ascontiguousarray(255 - p)   # dark lines on white paper
        for k in (0, 1):                    # the rules: 896 pixels long, so both settings find them
            p[30 + k::60, 32:S - 32] = 10; p[32:S - 32, 30 + k::60] = 10
        planted.append((p, rects))
    result = {"tool": "bench_page_derule", "pages": n, "page": [S, S], "lines": a.lines, "steps": a.steps, "warmup": a.warmup,
              "source_digest": retto_amd._lib.source_digest(), "settings": {}}
    s = retto_amd.RettoSession(retto_amd.synthetic_session_config(0, lanes=1))
    lib, h = s._hd.lib, s._hd.h
    dh, dw = C.c_int(), C.c_int()
    assert lib.rt_det_input_dims(h, S, S, C.byref(dh), C.byref(dw)) == 0
    pages = [upload(lib, h, p) for p, _ in planted]
    maps = [upload(lib, h, workload.planted_map(dh.value, dw.value, S, S, rects)) for _, rects in planted]

    def step():
        r = s.run_batch_raw(pages, [S] * n, [S] * n, retto_amd.RT_MEM_DEVICE, det_map_override=maps)
        lines = sum(lib.rt_results_count(r, i) for i in range(n))
        lib.rt_results_free(r)
        return lines

    try:
        ms = C.c_float()
        assert lib.rt_bench_memcpy_d2d(h, n * S * S * 3, 20, C.byref(ms)) == 0
        result["memcpy_d2d_ms"] = ms.value; result["memcpy_d2d_bytes"] = n * S * S * 3
        for name, L, T, I in SETTINGS:
            s.set_page_derule(L, T, I)
            for _ in range(a.warmup):
                step()
            e = result["settings"][name] = {"min_len": L, "max_thick": T, "ink": I}
            per_call = {fam: [] for fam in FAMILIES}
            for _ in range(a.steps):
                s.profile_enable(True)
                e["lines"] = step()
                prof = s.profile_get()
                s.profile_enable(False)
                for fam in FAMILIES:
                    fam_ms, calls = prof.get(fam, (0.0, 0))
                    per_call[fam].append(fam_ms); e[fam + "_launches"] = calls
            for fam in FAMILIES:
                e[fam + "_ms"] = statistics.median(per_call[fam]); e[fam + "_ms_min"] = min(per_call[fam]); e[fam + "_ms_max"] = max(per_call[fam])
                if L:
                    e[fam + "_over_memcpy"] = e[fam + "_ms"] / ms.value
            e["sum_ms"] = sum(e[fam + "_ms"] for fam in FAMILIES)
    finally:
        for p in pages + maps:
            lib.rt_device_free(h, p)
        s.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
