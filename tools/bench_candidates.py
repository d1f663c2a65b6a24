"""Cost of rec_return_candidates on C3: 32 synthetic 960 x 960 pages with 32 planted lines each (bench.py's C3 pages), pages and
planted maps resident in HBM, one session each for K = 0 (off), 1 and 5 in one process.

Reported per K: the C3 step time and images/s (batches submitted ahead, two in flight, the sessions alternating `--repeats`
times, median and spread), and from a serial profiled pass (one lane, per-launch events) the device time per batch of the
option's launch families (`ctc_kept_rows`, `ctc_gather_rows`, `gemm_cand_fc`, `ctc_topk`) next to `ctc_decode` and `net/rec`,
with the lines, time steps' kept tokens and candidate bytes of one batch.

    python tools/bench_candidates.py --steps 20 --warmup 3 --repeats 3
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

FAMILIES = ("ctc_kept_rows", "ctc_gather_rows", "gemm_cand_fc", "ctc_topk")


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


class C3:
    """one session with its own HBM copies of the pages and maps"""

    def __init__(self, k, n_pages, lines):
        cfg = retto_amd.synthetic_session_config(0)
        cfg.rec_processor_config.return_candidates = k
        self.k = k
        self.sess = retto_amd.RettoSession(cfg)
        lib, h = self.sess._hd.lib, self.sess._hd.h
        self.lib, self.h = lib, h
        self.d_pages, self.d_maps = [], []
        for i in range(n_pages):
            page, rects = workload.planted_page(960, 960, lines, seed=i)
            rh, rw, dh, dw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert lib.rt_resize_both_dims(h, 960, 960, C.byref(rh), C.byref(rw)) == 0
            assert lib.rt_det_input_dims(h, rh.value, rw.value, C.byref(dh), C.byref(dw)) == 0
            m = workload.planted_map(dh.value, dw.value, 960, 960, rects)
            self.d_pages.append(upload(lib, h, page)); self.d_maps.append(upload(lib, h, m))
        self.n = n_pages

    def run(self):
        return self.sess.run_batch_raw(self.d_pages, [960] * self.n, [960] * self.n, retto_amd.RT_MEM_DEVICE, self.d_maps)

    def steps(self, k, inflight=2):
        q = []
        for _ in range(k):
            q.append(self.sess.submit_batch_raw(self.d_pages, [960] * self.n, [960] * self.n, retto_amd.RT_MEM_DEVICE, self.d_maps))
            if len(q) >= inflight:
                self.lib.rt_results_free(self.sess.wait_batch_raw(q.pop(0)))
        while q:
            self.lib.rt_results_free(self.sess.wait_batch_raw(q.pop(0)))

    def step_ms(self, k):
        self.lib.rt_synchronize(self.h)
        t0 = time.perf_counter()
        self.steps(k)
        return (time.perf_counter() - t0) * 1e3 / k

    def counts(self):
        r = self.run()
        try:
            lines = tokens = 0
            texts = []
            for i in range(self.n):
                for k in range(self.lib.rt_results_count(r, i)):
                    tp = C.POINTER(C.c_int32)()
                    nt = self.lib.rt_results_rec_tokens(r, i, k, C.byref(tp))
                    assert self.lib.rt_results_rec_candidates(r, i, k, None, None) == self.k
                    lines += 1; tokens += nt
                    texts.append(self.lib.rt_results_rec_text(r, i, k))
        finally:
            self.lib.rt_results_free(r)
        return lines, tokens, texts

    def profile(self, k):
        """device ms per batch of the scopes of interest, from a serial pass with per-launch events"""
        self.lib.rt_set_lanes(self.h, 1)
        for _ in range(2):
            self.lib.rt_results_free(self.run())
        self.sess.profile_enable(True)
        for _ in range(k):
            self.lib.rt_results_free(self.run())
        prof = self.sess.profile_get()
        self.sess.profile_enable(False)
        self.lib.rt_set_lanes(self.h, 1 << 20)
        keep = FAMILIES + ("ctc_decode", "gemm_ctc_fc", "net/rec", "net/det", "net/cls")
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
    ap.add_argument("--k", type=int, nargs="+", default=[0, 1, 5],
                    help="the candidate counts to compare (0 = off); a count given twice gets two sessions: their difference is "
                         "what two sessions of one configuration differ by")
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1:
        ap.error("--steps, --repeats and --profile-steps must be at least 1")
    runs = [C3(k, a.pages, a.lines) for k in a.k]
    try:
        out = {"pages": a.pages, "steps": a.steps, "repeats": a.repeats}
        texts, tokens_of = [], []
        for s in runs:
            lines, tokens, t = s.counts()
            texts.append(t); tokens_of.append(tokens)
            out["lines_per_batch"], out["tokens_per_batch"] = lines, tokens_of[0]
            s.steps(a.warmup)
        out["texts_equal"] = all(t == texts[0] for t in texts)
        ms = [[] for _ in runs]
        for _ in range(a.repeats):
            for i, s in enumerate(runs):
                ms[i].append(s.step_ms(a.steps))
        for i, s in enumerate(runs):
            v = ms[i]
            med = float(np.median(v))
            name = "K=%d" % s.k
            while name in out:
                name += "'"
            out[name] = {"step_ms": {"median": med, "min": min(v), "max": max(v)}, "images_per_s": a.pages * 1e3 / med,
                                 "tokens_per_batch": tokens_of[i], "texts_equal_first": texts[i] == texts[0],
                                 "candidate_bytes_returned_per_batch": tokens_of[i] * s.k * 8,
                                 "profile": s.profile(a.profile_steps)}
        off = out.get("K=0")
        if off:
            out["new_families_when_off"] = [f for f in FAMILIES if f in off["profile"]]
        print(json.dumps(out))
    finally:
        for s in runs:
            s.close()


if __name__ == "__main__":
    main()
