"""Encoded-page throughput: rt_run_encoded_batch (host decode, then the batch) against rt_submit_encoded_batch with two batches
in flight (host entropy decoding of batch i + 1 under the GPU work of batch i, pixel reconstruction on the GPU).

32 JPEG pages of 960 x 960 (q90 4:2:0, planted text lines from a seed), synthetic C3 session.  The two forms alternate inside
one process, `--repeats` times each; reported: pages/s (median and spread) and host CPU seconds per page (process CPU time
over the timed window).  Kernel times of k_jpeg_idct / k_jpeg_color come from a separate rocprofv3 --kernel-trace --stats run
of this script.

    python tools/bench_encoded.py --steps 10 --warmup 2 --repeats 3
"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import retto_amd  # noqa: E402
from retto_amd import workload  # noqa: E402


def pages(n, seed):
    out = []
    for i in range(n):
        page, _ = workload.planted_page(960, 960, 32, seed=seed + i)
        b = io.BytesIO()
        Image.fromarray(page).save(b, "JPEG", quality=90, subsampling=2)
        out.append(b.getvalue())
    return out


def run_sync(sess, files, steps):
    for _ in range(steps):
        sess.run_encoded_batch(files)


def run_pipelined(sess, files, steps):
    inflight = [sess.submit_encoded_batch(files)]
    for _ in range(steps - 1):
        inflight.append(sess.submit_encoded_batch(files))
        sess.wait_batch(inflight.pop(0))
    sess.wait_batch(inflight.pop(0))


def timed(fn, sess, files, steps):
    c0, t0 = time.process_time(), time.perf_counter()
    fn(sess, files, steps)
    t1, c1 = time.perf_counter(), time.process_time()
    n = steps * len(files)
    return n / (t1 - t0), (c1 - c0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1:
        ap.error("--steps and --repeats must be at least 1")
    files = pages(a.pages, a.seed)
    sess = retto_amd.RettoSession(retto_amd.synthetic_session_config(0))
    try:
        ref = sess.run_encoded_batch(files)
        got = sess.wait_batch(sess.submit_encoded_batch(files))
        same = all(len(x.det_result) == len(y.det_result) and [r.text for r in x.rec_result] == [r.text for r in y.rec_result]
                   for x, y in zip(ref, got))
        for fn in (run_sync, run_pipelined):
            fn(sess, files, a.warmup)
        res = {"sync": [], "pipelined": []}
        for _ in range(a.repeats):
            res["sync"].append(timed(run_sync, sess, files, a.steps))
            res["pipelined"].append(timed(run_pipelined, sess, files, a.steps))
        out = {"pages": a.pages, "steps": a.steps, "repeats": a.repeats, "results_equal": same,
               "host_cpu_budget": sess._hd.lib.rt_host_cpu_budget()}
        for k, v in res.items():
            rate = [r for r, _ in v]; cpu = [c for _, c in v]
            out[k] = {"pages_per_s": float(np.median(rate)), "pages_per_s_min": min(rate), "pages_per_s_max": max(rate),
                      "cpu_s_per_page": float(np.median(cpu))}
        print(json.dumps(out))
    finally:
        sess.close()


if __name__ == "__main__":
    main()
