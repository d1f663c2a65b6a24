"""Cost of rec windows (rt_set_rec_windows) on long lines: seeded synthetic pages of 1024 x 3072 whose planted lines are 24 .. 64
times as wide as high (rec tensors of 1152 .. 3072 columns, 144 .. 384 time steps), resident in HBM, read through rt_run_regions
(the lines' rectangles are the regions: no detector in the way) on one lane of one session.

Settings, alternating in one run, `--repeats` times each: windows off (every line one image), windows (640, 128).  Reported per
setting: the median and spread of the time of one rt_run_regions call over the pages (host clock around the call, which ends in
a device synchronise; profiler off), and from a separate profiled pass (per-launch events) the device time per call of `net/rec`,
`attention`, `rec_window_cut` and `rec_window_stitch`, with the units per call.  For scale: a device-to-device hipMemcpyAsync of
the bytes each kernel writes (cut: the unit tensors, 48 x columns x 16 bytes; stitch: (120 + 2) floats per line time step), timed
in the same run, and each kernel as a multiple of it.  Synthetic weights: nothing here says anything about accuracy.  One JSON
line on stdout.

    python tools/bench_rec_windows.py --steps 10 --warmup 3 --repeats 3
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import retto_amd  # noqa: E402
from retto_amd import workload  # noqa: E402

SETTINGS = (("off", 0, 0), ("640/128", 640, 128))
FAMILIES = ("net/rec", "attention", "rec_window_cut", "rec_window_stitch")


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3072)
    ap.add_argument("--lines", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=2)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1:
        ap.error("--steps, --repeats and --profile-steps must be at least 1")
    H, W, n = a.height, a.width, a.pages
    planted = [workload.planted_page(H, W, a.lines, seed=100 + i, ratio_range=(24.0, 64.0)) for i in range(n)]
    quads = [np.array([[x0, y0, x1, y0, x1, y1, x0, y1] for (x0, y0, x1, y1) in rects], np.float32) for _, rects in planted]
    ratios = [(x1 - x0) / (y1 - y0) for _, rects in planted for (x0, y0, x1, y1) in rects]
    sess = retto_amd.RettoSession(retto_amd.synthetic_session_config(0, lanes=1))
    lib, h = sess._hd.lib, sess._hd.h
    result = {"tool": "bench_rec_windows", "pages": n, "page": [H, W], "lines_per_page": a.lines,
              "line_ratio_min": round(min(ratios), 2), "line_ratio_max": round(max(ratios), 2), "steps": a.steps, "warmup": a.warmup,
              "repeats": a.repeats, "source_digest": retto_amd._lib.source_digest(), "settings": {}}
    d_pages = [upload(lib, h, p) for p, _ in planted]

    def pass_on(steps):
        t, units = [], 0
        for _ in range(steps):
            t0 = time.perf_counter()
            r = sess.run_regions_raw(d_pages, [H] * n, [W] * n, quads, mem=retto_amd.RT_MEM_DEVICE)
            t.append((time.perf_counter() - t0) * 1e3)
            units = sum(lib.rt_results_rec_windows(r, i, k) for i in range(n) for k in range(lib.rt_results_count(r, i)))
            lib.rt_results_free(r)
        return t, units

    try:
        times = {name: [] for name, _, _ in SETTINGS}
        for rep in range(a.repeats):
            for name, win, ov in SETTINGS:
                sess.set_rec_windows(win, ov)
                pass_on(a.warmup)
                t, units = pass_on(a.steps)
                times[name].append(statistics.median(t))
                result["settings"].setdefault(name, {"window": win, "overlap": ov})["units_per_call"] = units
        for name, win, ov in SETTINGS:
            sess.set_rec_windows(win, ov)
            pass_on(1)
            sess.profile_enable(True)
            pass_on(a.profile_steps)
            prof = sess.profile_get()
            sess.profile_enable(False)
            e = result["settings"][name]
            e["call_ms_median"] = statistics.median(times[name]); e["call_ms_min"] = min(times[name]); e["call_ms_max"] = max(times[name])
            e["call_ms_repeats"] = times[name]
            for fam in FAMILIES:
                ms, calls = prof.get(fam, (0.0, 0))
                e[fam + "_ms"] = ms / a.profile_steps; e[fam + "_launches"] = calls // a.profile_steps
        # the bytes the two kernels write in one call, from the plan of every line at the width rec_plan gives it
        on = result["settings"][SETTINGS[1][0]]
        win, ov = SETTINGS[1][1], SETTINGS[1][2]
        cut_bytes = stitch_bytes = 0
        for q in quads:
            ws, hs = (q[:, 2] - q[:, 0]).astype(np.float32), (q[:, 5] - q[:, 1]).astype(np.float32)
            order = sorted(range(len(q)), key=lambda i: -(float(hs[i]) / float(ws[i])))
            for s0 in range(0, len(q), 6):
                ratio = max([np.float32(320) / np.float32(48)] + [ws[i] / hs[i] for i in order[s0:s0 + 6]])
                Wl = lib.rt_resize_norm_width(48, 320, C.c_float(float(ratio)))
                p = retto_amd.rec_window_plan(Wl, win, ov)
                for _ in order[s0:s0 + 6]:
                    cut_bytes += 48 * sum(p["widths"]) * 16
                    stitch_bytes += p["T"] * (120 + 2) * 4
        for fam, nbytes in (("rec_window_cut", cut_bytes), ("rec_window_stitch", stitch_bytes)):
            ms = C.c_float()
            assert lib.rt_bench_memcpy_d2d(h, nbytes, 20, C.byref(ms)) == 0
            on[fam + "_bytes"] = nbytes; on[fam + "_memcpy_d2d_ms"] = ms.value
            on[fam + "_over_memcpy"] = on[fam + "_ms"] / ms.value if ms.value else None
        on["cut_plus_stitch_share_of_net_rec"] = (on["rec_window_cut_ms"] + on["rec_window_stitch_ms"]) / on["net/rec_ms"]
        off = result["settings"][SETTINGS[0][0]]
        result["call_ms_on_over_off"] = on["call_ms_median"] / off["call_ms_median"]
        result["net_rec_ms_on_over_off"] = on["net/rec_ms"] / off["net/rec_ms"]
        result["attention_ms_on_over_off"] = on["attention_ms"] / off["attention_ms"] if off["attention_ms"] else None
    finally:
        for p in d_pages:
            lib.rt_device_free(h, p)
        sess.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
