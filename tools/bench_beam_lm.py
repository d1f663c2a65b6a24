"""Cost of language-model fusion in the rec beams (rt_set_rec_beam_lm) at C3's shape: tools/bench_beam.py's pages -- 32 synthetic
960 x 960 pages with 32 planted lines each, resident in HBM, the regions being the boxes the session's own detector finds on them
-- one session, the same beam and nbest, with and without a seeded trigram model over the session's dictionary (built around the
strings the lines read, so that the higher orders are reached; about 10 % of the classes without a unigram).

Reported per leg ("unused": no beam at all, "beams", "beams_lm"): the time of one rt_run_regions call over the 32 pages (three
lanes; the legs alternate `--repeats` times: median and spread) and, from a serial profiled pass (one lane, per-launch events), the
device time per call of the search family -- `ctc_beam_search` without a model, `ctc_beam_search_lm` with one -- next to the rest
of the beams' families.  `lm_cost` is the fused leg over the beams-only leg of the same run; `new_families_when_unused` must be
empty.

    python tools/bench_beam_lm.py --beam 16 --nbest 4 --steps 10 --warmup 2 --repeats 3
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import retto_amd  # noqa: E402
from retto_amd import workload  # noqa: E402

import ctc_lm_ref as MR  # noqa: E402  (the seeded model generator and the ARPA writer)

FAMILIES = ("ctc_gather_rows", "gemm_cand_fc", "ctc_row_lse", "ctc_beam_topc", "ctc_beam_search", "ctc_beam_search_lm")


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--nbest", type=int, default=4)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--beta", type=float, default=0.6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=3)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1 or a.beam < 1:
        ap.error("--steps, --repeats, --profile-steps and --beam must be at least 1")
    sess = retto_amd.RettoSession(retto_amd.synthetic_session_config(0))
    lib, h = sess._hd.lib, sess._hd.h
    d_pages = []
    try:
        pages, maps = [], []
        for i in range(a.pages):
            page, rects = workload.planted_page(960, 960, a.lines, seed=i)
            rh, rw, dh, dw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert lib.rt_resize_both_dims(h, 960, 960, C.byref(rh), C.byref(rw)) == 0
            assert lib.rt_det_input_dims(h, rh.value, rw.value, C.byref(dh), C.byref(dw)) == 0
            pages.append(page); maps.append(workload.planted_map(dh.value, dw.value, 960, 960, rects))
            d_pages.append(upload(lib, h, page))
        first = sess.run_batch(pages, det_map_override=maps)
        quads = [np.stack([d.boxes.as_array() for d in r.det_result]) if r.det_result else np.zeros((0, 4, 2), np.float32) for r in first]
        dic = sess._dictionary()
        texts = [tuple(int(t) for t in g.tokens) for r in first for g in r.rec_result]
        model = MR.random_model(2024, len(dic), a.order, texts, per_level=4000)
        lm = sess.create_lm(MR.write_arpa(model, dic), oov_log10=model.oov / MR.LN10)
        legs = [("unused", (0, 1), -1), ("beams", (a.beam, a.nbest), -1), ("beams_lm", (a.beam, a.nbest), lm)]

        def run(leg):
            sess.set_rec_beam(*leg[1])
            sess.set_rec_beam_lm(leg[2], a.alpha, a.beta)
            return sess.run_regions_raw(d_pages, [960] * a.pages, [960] * a.pages, quads, retto_amd.RT_MEM_DEVICE)

        def step_ms(leg, steps):
            lib.rt_synchronize(h)
            t0 = time.perf_counter()
            for _ in range(steps):
                lib.rt_results_free(run(leg))
            return (time.perf_counter() - t0) * 1e3 / steps

        def profile(leg):
            lib.rt_set_lanes(h, 1)
            for _ in range(2):
                lib.rt_results_free(run(leg))
            sess.profile_enable(True)
            for _ in range(a.profile_steps):
                lib.rt_results_free(run(leg))
            prof = sess.profile_get()
            sess.profile_enable(False)
            lib.rt_set_lanes(h, 1 << 20)
            keep = FAMILIES + ("ctc_decode", "gemm_ctc_fc", "net/rec", "net/cls", "warp_crops")
            return {name: {"ms_per_call": v[0] / a.profile_steps, "launches_per_call": v[1] / a.profile_steps}
                    for name, v in prof.items() if name in keep and v[1] > 0}

        out = {"pages": a.pages, "lines_per_call": int(sum(len(q) for q in quads)), "steps": a.steps, "repeats": a.repeats,
               "beam": a.beam, "nbest": a.nbest, "alpha": a.alpha, "beta": a.beta,
               "model": dict(sess.lm_info(lm), classes=len(dic), classes_without_unigram=sum(1 for c in range(1, len(dic)) if (c,) not in model.ngrams))}
        for leg in legs:
            step_ms(leg, a.warmup)
        ms = {leg[0]: [] for leg in legs}
        for _ in range(a.repeats):
            for leg in legs:
                ms[leg[0]].append(step_ms(leg, a.steps))
        for leg in legs:
            v = ms[leg[0]]
            med = float(np.median(v))
            out[leg[0]] = {"step_ms": {"median": med, "min": min(v), "max": max(v)}, "images_per_s": a.pages * 1e3 / med,
                           "profile": profile(leg)}
        search = out["beams"]["profile"].get("ctc_beam_search", {}).get("ms_per_call")
        search_lm = out["beams_lm"]["profile"].get("ctc_beam_search_lm", {}).get("ms_per_call")
        out["lm_cost"] = {"added_ms_per_step": out["beams_lm"]["step_ms"]["median"] - out["beams"]["step_ms"]["median"],
                          "search_ms_per_call": search, "search_lm_ms_per_call": search_lm,
                          "search_ratio": None if not search or search_lm is None else search_lm / search}
        r = run(legs[-1])   # how many hypotheses the lines report, and on how many lines the model changes rank 0
        out["beams_lm"]["hypotheses"] = sum(lib.rt_results_rec_beam_lm(r, i, k, None) for i, q in enumerate(quads) for k in range(len(q)))
        lib.rt_results_free(r)
        out["new_families_when_unused"] = [f for f in FAMILIES if f in out["unused"]["profile"]]
        out["lm_families_without_a_model"] = [f for f in out["beams"]["profile"] if f.endswith("_lm")]
        print(json.dumps(out))
    finally:
        sess.set_rec_beam_lm(-1)
        sess.set_rec_beam(0)
        for p in d_pages:
            lib.rt_device_free(h, C.c_void_p(p))
        sess.close()


if __name__ == "__main__":
    main()
