"""Cost of rec_return_word_box on C3: 32 synthetic 960 x 960 pages with 32 planted lines each (bench.py's C3 pages), pages and
planted maps resident in HBM, one session with the option on and one with it off.

Reported: images/s of both sessions (batches submitted ahead, two in flight, the two sessions alternating `--repeats` times,
median and spread), and from a serial profiled pass (one lane, per-launch events) the device time per batch of the
`word_boxes` scope next to `ctc_decode` and `net/rec`, with the lines and words of one batch.

    python tools/bench_word_boxes.py --steps 20 --warmup 3 --repeats 3
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import retto_amd  # noqa: E402
from retto_amd import workload  # noqa: E402


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


class C3:
    """one session with its own HBM copies of the pages and maps"""

    def __init__(self, words, n_pages, lines):
        cfg = retto_amd.synthetic_session_config(0)
        cfg.rec_processor_config.return_word_box = words
        self.sess = retto_amd.RettoSession(cfg)
        lib, h = self.sess._hd.lib, self.sess._hd.h
        self.lib, self.h = lib, h
        self.d_pages, self.d_maps, self.bufs = [], [], []
        for i in range(n_pages):
            page, rects = workload.planted_page(960, 960, lines, seed=i)
            rh, rw, dh, dw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert lib.rt_resize_both_dims(h, 960, 960, C.byref(rh), C.byref(rw)) == 0
            assert lib.rt_det_input_dims(h, rh.value, rw.value, C.byref(dh), C.byref(dw)) == 0
            m = workload.planted_map(dh.value, dw.value, 960, 960, rects)
            self.d_pages.append(upload(lib, h, page)); self.d_maps.append(upload(lib, h, m))
        self.n = n_pages

    def submit(self):
        return self.sess.submit_batch_raw(self.d_pages, [960] * self.n, [960] * self.n, retto_amd.RT_MEM_DEVICE, self.d_maps)

    def steps(self, k, inflight=2):
        q = []
        for _ in range(k):
            q.append(self.submit())
            if len(q) >= inflight:
                self.lib.rt_results_free(self.sess.wait_batch_raw(q.pop(0)))
        while q:
            self.lib.rt_results_free(self.sess.wait_batch_raw(q.pop(0)))

    def rate(self, k):
        self.lib.rt_synchronize(self.h)
        t0 = time.perf_counter()
        self.steps(k)
        return k * self.n / (time.perf_counter() - t0)

    def counts(self):
        r = self.sess.run_batch_raw(self.d_pages, [960] * self.n, [960] * self.n, retto_amd.RT_MEM_DEVICE, self.d_maps)
        try:
            lines = sum(self.lib.rt_results_count(r, i) for i in range(self.n))
            wp = C.POINTER(retto_amd._lib.Word)()
            words = sum(self.lib.rt_results_rec_words(r, i, k, C.byref(wp)) for i in range(self.n)
                        for k in range(self.lib.rt_results_count(r, i)))
            texts = [self.lib.rt_results_rec_text(r, i, k) for i in range(self.n) for k in range(self.lib.rt_results_count(r, i))]
        finally:
            self.lib.rt_results_free(r)
        return lines, words, texts

    def profile(self, k):
        """device ms per batch of the scopes of interest, from a serial pass with per-launch events"""
        self.lib.rt_set_lanes(self.h, 1)
        for _ in range(2):
            self.lib.rt_results_free(self.sess.run_batch_raw(self.d_pages, [960] * self.n, [960] * self.n, retto_amd.RT_MEM_DEVICE, self.d_maps))
        self.sess.profile_enable(True)
        for _ in range(k):
            self.lib.rt_results_free(self.sess.run_batch_raw(self.d_pages, [960] * self.n, [960] * self.n, retto_amd.RT_MEM_DEVICE, self.d_maps))
        prof = self.sess.profile_get()
        self.sess.profile_enable(False)
        self.lib.rt_set_lanes(self.h, 1 << 20)
        keep = ("word_boxes", "ctc_decode", "net/rec", "net/det", "net/cls")
        return {name: {"ms_per_batch": v[0] / k, "launches_per_batch": v[1] / k} for name, v in prof.items() if name in keep}

    def close(self):
        for p in self.d_pages + self.d_maps:
            self.lib.rt_device_free(self.h, C.c_void_p(p))
        self.sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1:
        ap.error("--steps, --repeats and --profile-steps must be at least 1")
    on, off = C3(True, a.pages, a.lines), C3(False, a.pages, a.lines)
    try:
        lines, words, texts_on = on.counts()
        _, words_off, texts_off = off.counts()
        for s in (on, off):
            s.steps(a.warmup)
        rates = {"on": [], "off": []}
        for _ in range(a.repeats):
            rates["off"].append(off.rate(a.steps))
            rates["on"].append(on.rate(a.steps))
        out = {"pages": a.pages, "steps": a.steps, "repeats": a.repeats, "lines_per_batch": lines, "words_per_batch": words,
               "words_when_off": words_off, "texts_equal": texts_on == texts_off}
        for k, v in rates.items():
            out["images_per_s_" + k] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
        out["profile_on"] = on.profile(a.profile_steps)
        out["profile_off"] = off.profile(a.profile_steps)
        print(json.dumps(out))
    finally:
        on.close(); off.close()


if __name__ == "__main__":
    main()
