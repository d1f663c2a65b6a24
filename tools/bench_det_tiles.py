"""Cost of det tiles (rt_set_det_tiles) on large pages: four seeded synthetic pages of 2176 x 3840 with planted lines, resident
in HBM, one session with max_side_len 4096 (so the pages reach the detector at their own size) on one lane, the DB
post-processing fed by planted maps (the det network still runs; its map is what the checksum sums).

Settings, alternating in one run, `--repeats` times each: tiles off (the whole-page det path), tiles (960, 64), tiles (960, 128).
Reported per setting: the median and spread of the time of one rt_run_batch call over the four pages (host clock around the
call, which ends in a device synchronise; profiler off), and from a separate profiled pass (per-launch events) the device time
per call of `net/det`, `det_tile_cut` and `det_tile_stitch`, plus the scratch arena's high-water mark (each setting on a session
of its own for that figure: an arena never shrinks).  For scale: a device-to-device hipMemcpyAsync of the stitched maps' bytes
(4 x 2176 x 3840 floats), timed in the same run, and cut + stitch as a multiple of it.  One JSON line on stdout.

    python tools/bench_det_tiles.py --steps 5 --warmup 2 --repeats 3
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

SETTINGS = (("off", 0, 0), ("960/64", 960, 64), ("960/128", 960, 128))
FAMILIES = ("net/det", "det_tile_cut", "det_tile_stitch")


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


def new_session():
    return retto_amd.RettoSession(retto_amd.synthetic_session_config(0, max_side_len=4096, lanes=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--height", type=int, default=2176)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--lines", type=int, default=48)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=2)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1:
        ap.error("--steps, --repeats and --profile-steps must be at least 1")
    H, W, n = a.height, a.width, a.pages
    planted = [workload.planted_page(H, W, a.lines, seed=i) for i in range(n)]
    sess = new_session()
    lib, h = sess._hd.lib, sess._hd.h
    dh, dw = C.c_int(), C.c_int()
    assert lib.rt_det_input_dims(h, H, W, C.byref(dh), C.byref(dw)) == 0
    assert (dh.value, dw.value) == (H, W), "the pages must reach the detector at their own size"
    maps = [workload.planted_map(H, W, H, W, rects) for _, rects in planted]
    result = {"tool": "bench_det_tiles", "pages": n, "page": [H, W], "lines": a.lines, "steps": a.steps, "warmup": a.warmup,
              "repeats": a.repeats, "source_digest": retto_amd._lib.source_digest(), "settings": {}}

    def pass_on(s, bufs, steps):
        d_pages, d_maps = bufs
        t = []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = s.run_batch_raw(d_pages, [H] * n, [W] * n, retto_amd.RT_MEM_DEVICE, det_map_override=d_maps)
            t.append((time.perf_counter() - t0) * 1e3)
            lines = sum(s._hd.lib.rt_results_count(r, i) for i in range(n))
            s._hd.lib.rt_results_free(r)
        return t, lines

    bufs = ([upload(lib, h, p) for p, _ in planted], [upload(lib, h, m) for m in maps])
    try:
        times = {name: [] for name, _, _ in SETTINGS}
        for rep in range(a.repeats):
            for name, T, O in SETTINGS:
                sess.set_det_tiles(T, O)
                pass_on(sess, bufs, a.warmup)
                t, lines = pass_on(sess, bufs, a.steps)
                times[name].append(statistics.median(t))
                result["settings"].setdefault(name, {"tile": T, "overlap": O})["lines"] = lines
        for name, T, O in SETTINGS:
            sess.set_det_tiles(T, O)
            pass_on(sess, bufs, 1)
            sess.profile_enable(True)
            pass_on(sess, bufs, a.profile_steps)
            prof = sess.profile_get()
            sess.profile_enable(False)
            e = result["settings"][name]
            e["step_ms_median"] = statistics.median(times[name]); e["step_ms_min"] = min(times[name]); e["step_ms_max"] = max(times[name])
            e["step_ms_repeats"] = times[name]
            for fam in FAMILIES:
                ms, calls = prof.get(fam, (0.0, 0))
                e[fam + "_ms"] = ms / a.profile_steps; e[fam + "_launches"] = calls // a.profile_steps
            p = retto_amd.det_tile_plan(H, W, T, O)
            e["tiles_per_page"] = len(p["row_origins"]) * len(p["col_origins"])
        ms = C.c_float()
        assert lib.rt_bench_memcpy_d2d(h, n * H * W * 4, 20, C.byref(ms)) == 0
        result["memcpy_d2d_ms"] = ms.value; result["memcpy_d2d_bytes"] = n * H * W * 4
        for name, T, O in SETTINGS[1:]:
            e = result["settings"][name]
            e["cut_plus_stitch_over_memcpy"] = (e["det_tile_cut_ms"] + e["det_tile_stitch_ms"]) / ms.value
    finally:
        for p in bufs[0] + bufs[1]:
            lib.rt_device_free(h, p)
        sess.close()
    # the scratch arena's high-water mark: a session of its own per setting
    for name, T, O in SETTINGS:
        s = new_session()
        try:
            b = ([upload(s._hd.lib, s._hd.h, p) for p, _ in planted], [upload(s._hd.lib, s._hd.h, m) for m in maps])
            s.set_det_tiles(T, O)
            pass_on(s, b, 1)
            hw = (C.c_longlong * 3)()
            assert s._hd.lib.rt_debug_arena_high_water(s._hd.h, hw) == 0
            result["settings"][name]["arena_mib"] = hw[0] / 2**20
            result["settings"][name]["scratch_mib"] = hw[1] / 2**20
            result["settings"][name]["dbws_mib"] = hw[2] / 2**20
            for p in b[0] + b[1]:
                s._hd.lib.rt_device_free(s._hd.h, p)
        finally:
            s.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
