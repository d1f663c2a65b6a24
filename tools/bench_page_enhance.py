"""Cost of page enhance (rt_set_page_enhance) on the C3 pages: 32 seeded synthetic pages of 960 x 960 with 32 planted lines each,
resident in HBM, the DB post-processing fed by planted maps in HBM (the det network still runs), the library's default lanes.

Settings: enhance off, tile 64 and tile 128 at clip 2.5.  Every (repeat, setting) is a session of its own, the settings
alternating inside a repeat, so the spread between sessions of one setting is in the numbers.  Reported per setting: the median,
min and max over the sessions of the median time of one rt_run_batch call over the 32 pages (host clock around the call, which
ends in a device synchronise; profiler off), the on-cost against off, and from a separate serial profiled pass (one lane,
per-launch events) the device time per call -- one lane part of 32 pages -- of `page_enhance_lut` and `page_enhance_apply`.  For
scale: a device-to-device hipMemcpyAsync of the pages' bytes (32 x 960 x 960 x 3), timed in the same run, and the apply kernel
as a multiple of it: both read and write every page byte once.  One JSON line on stdout.

    python tools/bench_page_enhance.py --steps 10 --warmup 3 --repeats 3
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

import retto_amd  # noqa: E402
from retto_amd import workload  # noqa: E402

SETTINGS = (("off", 0, 0.0), ("64/2.5", 64, 2.5), ("128/2.5", 128, 2.5))
FAMILIES = ("page_enhance_lut", "page_enhance_apply")


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=3)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1:
        ap.error("--steps, --repeats and --profile-steps must be at least 1")
    S, n = a.size, a.pages
    planted = [workload.planted_page(S, S, a.lines, seed=i) for i in range(n)]
    result = {"tool": "bench_page_enhance", "pages": n, "page": [S, S], "lines": a.lines, "steps": a.steps, "warmup": a.warmup,
              "repeats": a.repeats, "source_digest": retto_amd._lib.source_digest(), "settings": {}}

    class Run:
        """a session with the pages and their planted maps in its device's memory"""
        def __init__(self, lanes=0):
            self.s = retto_amd.RettoSession(retto_amd.synthetic_session_config(0, lanes=lanes))
            self.lib, self.h = self.s._hd.lib, self.s._hd.h
            dh, dw = C.c_int(), C.c_int()
            assert self.lib.rt_det_input_dims(self.h, S, S, C.byref(dh), C.byref(dw)) == 0
            self.pages = [upload(self.lib, self.h, p) for p, _ in planted]
            self.maps = [upload(self.lib, self.h, workload.planted_map(dh.value, dw.value, S, S, rects)) for _, rects in planted]

        def steps(self, k):
            t, lines = [], 0
            for _ in range(k):
                t0 = time.perf_counter()
                r = self.s.run_batch_raw(self.pages, [S] * n, [S] * n, retto_amd.RT_MEM_DEVICE, det_map_override=self.maps)
                t.append((time.perf_counter() - t0) * 1e3)
                lines = sum(self.lib.rt_results_count(r, i) for i in range(n))
                self.lib.rt_results_free(r)
            return t, lines

        def close(self):
            for p in self.pages + self.maps:
                self.lib.rt_device_free(self.h, p)
            self.s.close()

    times = {name: [] for name, _, _ in SETTINGS}
    for rep in range(a.repeats):
        for name, T, clip in SETTINGS:
            run = Run()
            try:
                run.s.set_page_enhance(T, clip)
                run.steps(a.warmup)
                t, lines = run.steps(a.steps)
                times[name].append(statistics.median(t))
                result["settings"].setdefault(name, {"tile": T, "clip": clip})["lines"] = lines
            finally:
                run.close()
    for name, _, _ in SETTINGS:
        e = result["settings"][name]
        e["step_ms_median"] = statistics.median(times[name]); e["step_ms_min"] = min(times[name]); e["step_ms_max"] = max(times[name])
        e["step_ms_sessions"] = times[name]
        e["on_cost_ms"] = e["step_ms_median"] - statistics.median(times["off"])
    # the kernels' device times: a serial pass on one lane with per-launch events, and the copy they are stated against
    run = Run(lanes=1)
    try:
        ms = C.c_float()
        assert run.lib.rt_bench_memcpy_d2d(run.h, n * S * S * 3, 20, C.byref(ms)) == 0
        result["memcpy_d2d_ms"] = ms.value; result["memcpy_d2d_bytes"] = n * S * S * 3
        for name, T, clip in SETTINGS:
            run.s.set_page_enhance(T, clip)
            run.steps(1)
            run.s.profile_enable(True)
            run.steps(a.profile_steps)
            prof = run.s.profile_get()
            run.s.profile_enable(False)
            e = result["settings"][name]
            for fam in FAMILIES:
                fam_ms, calls = prof.get(fam, (0.0, 0))
                e[fam + "_ms"] = fam_ms / a.profile_steps; e[fam + "_launches"] = calls // a.profile_steps
            e["apply_over_memcpy"] = e["page_enhance_apply_ms"] / ms.value
    finally:
        run.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
