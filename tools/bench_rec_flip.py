"""Cost of rec flip (rt_set_rec_flip): seeded synthetic pages with planted lines, resident in HBM, read through rt_run_regions
(the lines' rectangles are the regions: no detector in the way) on one lane of one session.

Settings, alternating in one run, `--repeats` times each: flip off; cls_below = 2.0 (every line read both ways); cls_below = the
median classifier score of the flip-off call (about half the lines, and the extra lane sync for the scores); cls_below = 1e-30
(on, no line flagged: the flip-off work plus that sync alone, which is how the cls-score round trip is measured).  Reported per
setting: the median and spread of the time of one rt_run_regions call over the pages (host clock around the call, which ends in
a device synchronise; profiler off), the lines read both ways, the rec pixels the network ran on, and from a separate profiled
pass (per-launch events) the device time per call of `net/rec`, `rec_flip_rotate`, `rec_flip_score` and `rec_flip_select`.  For
scale: a device-to-device hipMemcpyAsync of the bytes each kernel writes (rotate: the flagged crops, 3 bytes a pixel; select: an
int and a float per time step of a both-ways line -- z5 rows only move when the tail needs them, which it does not here), timed
in the same run, and each kernel as a multiple of it.  Synthetic weights: nothing here says anything about accuracy.  One JSON
line on stdout.

    python tools/bench_rec_flip.py --steps 10 --warmup 3 --repeats 3
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

FAMILIES = ("net/rec", "net/cls", "rec_flip_rotate", "rec_flip_score", "rec_flip_select")


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--lines", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=2)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1:
        ap.error("--steps, --repeats and --profile-steps must be at least 1")
    H, W, n = a.height, a.width, a.pages
    planted = [workload.planted_page(H, W, a.lines, seed=100 + i, ratio_range=(3.0, 12.0)) for i in range(n)]
    quads = [np.array([[x0, y0, x1, y0, x1, y1, x0, y1] for (x0, y0, x1, y1) in rects], np.float32) for _, rects in planted]
    sess = retto_amd.RettoSession(retto_amd.synthetic_session_config(0, lanes=1))
    lib, h = sess._hd.lib, sess._hd.h
    result = {"tool": "bench_rec_flip", "pages": n, "page": [H, W], "lines_per_page": a.lines, "steps": a.steps, "warmup": a.warmup,
              "repeats": a.repeats, "source_digest": retto_amd._lib.source_digest(), "settings": {}}
    d_pages = [upload(lib, h, p) for p, _ in planted]

    def pass_on(steps):
        t, both, cls = [], [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = sess.run_regions_raw(d_pages, [H] * n, [W] * n, quads, mem=retto_amd.RT_MEM_DEVICE)
            t.append((time.perf_counter() - t0) * 1e3)
            both = [[lib.rt_results_rec_flip(r, i, k, None, None) != 0 for k in range(lib.rt_results_count(r, i))] for i in range(n)]
            cls = [float(v) for i in range(n) for v in np.ctypeslib.as_array(lib.rt_results_cls_scores(r, i), (lib.rt_results_count(r, i),))]
            lib.rt_results_free(r)
        return t, both, cls

    try:
        _, _, cls = pass_on(1)
        mid = float(np.median(np.array(cls, np.float32)))
        settings = (("off", 0.0), ("2.0", 2.0), ("mid", mid), ("sync-only", 1e-30))
        # per line its crop's pixels and the width / time steps rec_plan gives it (batches of 6 by descending h / w)
        pix, width = [], []
        for q in quads:
            ws, hs = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
            assert lib.rt_crop_dims(q.ctypes.data_as(C.c_void_p), len(q), ws.ctypes.data_as(C.c_void_p), hs.ctypes.data_as(C.c_void_p)) == 0
            order = sorted(range(len(q)), key=lambda i: -(float(hs[i]) / float(ws[i])))
            wl = [0] * len(q)
            for s0 in range(0, len(q), 6):
                ratio = max([np.float32(320) / np.float32(48)] + [np.float32(ws[i]) / np.float32(hs[i]) for i in order[s0:s0 + 6]])
                for i in order[s0:s0 + 6]:
                    wl[i] = lib.rt_resize_norm_width(48, 320, float(ratio))
            pix.append([int(ws[i]) * int(hs[i]) for i in range(len(q))]); width.append(wl)
        times = {name: [] for name, _ in settings}
        flagged = {}
        for rep in range(a.repeats):
            for name, below in settings:
                sess.set_rec_flip(below)
                pass_on(a.warmup)
                t, both, _ = pass_on(a.steps)
                times[name].append(statistics.median(t)); flagged[name] = both
        for name, below in settings:
            sess.set_rec_flip(below)
            pass_on(1)
            sess.profile_enable(True)
            pass_on(a.profile_steps)
            prof = sess.profile_get()
            sess.profile_enable(False)
            e = result["settings"].setdefault(name, {"cls_below": below})
            e["call_ms_median"] = statistics.median(times[name]); e["call_ms_min"] = min(times[name]); e["call_ms_max"] = max(times[name])
            e["call_ms_repeats"] = times[name]
            both = flagged[name]
            e["lines"] = sum(len(b) for b in both); e["lines_both_ways"] = sum(sum(b) for b in both)
            lines_px = sum(48 * wl for ws in width for wl in ws)
            e["rec_pixels"] = lines_px + sum(48 * width[i][k] for i in range(n) for k in range(len(both[i])) if both[i][k])
            for fam in FAMILIES:
                ms, calls = prof.get(fam, (0.0, 0))
                e[fam + "_ms"] = ms / a.profile_steps; e[fam + "_launches"] = calls // a.profile_steps
            rot_bytes = sum(3 * pix[i][k] for i in range(n) for k in range(len(both[i])) if both[i][k])
            sel_bytes = sum(8 * retto_amd.rec_window_plan(width[i][k], 0, 0)["T"] + 12 for i in range(n) for k in range(len(both[i])) if both[i][k])
            for fam, nbytes in (("rec_flip_rotate", rot_bytes), ("rec_flip_select", sel_bytes)):
                if not nbytes:
                    continue
                ms = C.c_float()
                assert lib.rt_bench_memcpy_d2d(h, nbytes, 20, C.byref(ms)) == 0
                e[fam + "_bytes"] = nbytes; e[fam + "_memcpy_d2d_ms"] = ms.value
                e[fam + "_over_memcpy"] = e[fam + "_ms"] / ms.value if ms.value else None
        S = result["settings"]
        for name in ("2.0", "mid"):
            result["call_ms_%s_over_off" % name] = S[name]["call_ms_median"] / S["off"]["call_ms_median"]
            result["net_rec_ms_%s_over_off" % name] = S[name]["net/rec_ms"] / S["off"]["net/rec_ms"]
            result["rec_pixels_%s_over_off" % name] = S[name]["rec_pixels"] / S["off"]["rec_pixels"]
        # the cls-score round trip: a call that is on and flags no line does the flip-off work plus the copy and the sync
        result["cls_score_round_trip_ms"] = S["sync-only"]["call_ms_median"] - S["off"]["call_ms_median"]
    finally:
        sess.set_rec_flip(0.0)
        for p in d_pages:
            lib.rt_device_free(h, p)
        sess.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
