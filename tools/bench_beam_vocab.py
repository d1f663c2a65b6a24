"""Cost of the word-list constraint in the rec beams (rt_set_rec_beam_vocab) at C3's shape: tools/bench_beam.py's pages -- 32
synthetic 960 x 960 pages with 32 planted lines each, resident in HBM, the regions being the boxes the session's own detector
finds on them -- one session, the same beam and nbest, with and without a vocabulary of about 100 000 words of 2 to 12 ids over
the session's dictionary, generated from a seed: a tenth of them pieces of the strings the lines read, so that the search walks
down the trie and not only off its root, the rest random; the classes divisible by 4 occur in no word and separate them.

Reported per leg ("unused": no beam at all, "beams", "beams_vocab"): the time of one rt_run_regions call over the 32 pages (three
lanes; the legs alternate `--repeats` times: median and spread) and, from a serial profiled pass (one lane, per-launch events), the
device time per call of the search family -- `ctc_beam_search` without a vocabulary, `ctc_beam_search_vocab` with one -- next to
the rest of the beams' families.  `vocab_cost` is the constrained leg over the beams-only leg of the same run, a ratio of this
very process and no target fixed in advance; `new_families_when_unused` and `vocab_families_without_a_vocabulary` must be empty.

    python tools/bench_beam_vocab.py --beam 16 --nbest 4 --steps 10 --warmup 2 --repeats 3
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

FAMILIES = ("ctc_gather_rows", "gemm_cand_fc", "ctc_row_lse", "ctc_beam_topc", "ctc_beam_search", "ctc_beam_search_vocab",
            "ctc_beam_search_lm", "ctc_beam_search_lm_vocab")


def upload(lib, h, arr):
    p = C.c_void_p()
    assert lib.rt_device_malloc(h, arr.nbytes, C.byref(p)) == 0
    assert lib.rt_memcpy_h2d(h, p, arr.ctypes.data, arr.nbytes) == 0
    return p.value


def seeded_words(seed, classes, n_words, texts):
    """n_words words of 2 to 12 ids of [1, classes) that are no multiple of 4: a tenth cut from `texts`, the rest random"""
    rng = np.random.default_rng(seed)
    real = np.array([c for c in range(1, classes) if c % 4], np.int32)
    words = []
    runs = [[c for c in t if c % 4] for t in texts]
    runs = [r for r in runs if len(r) >= 2]
    for _ in range(n_words // 10 if runs else 0):
        r = runs[int(rng.integers(len(runs)))]
        n = int(rng.integers(2, min(12, len(r)) + 1))
        o = int(rng.integers(0, len(r) - n + 1))
        words.append(r[o:o + n])
    while len(words) < n_words:
        words.append(real[rng.integers(0, len(real), int(rng.integers(2, 13)))].tolist())
    return words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--nbest", type=int, default=4)
    ap.add_argument("--words", type=int, default=100000)
    ap.add_argument("--gamma", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=3)
    a = ap.parse_args()
    if a.steps < 1 or a.repeats < 1 or a.profile_steps < 1 or a.beam < 1 or a.words < 1:
        ap.error("--steps, --repeats, --profile-steps, --beam and --words must be at least 1")
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
        texts = [[int(t) for t in g.tokens] for r in first for g in r.rec_result]
        t0 = time.perf_counter()
        vocab = sess.create_vocab(ids=seeded_words(a.seed, len(dic), a.words, texts))
        create_ms = (time.perf_counter() - t0) * 1e3
        legs = [("unused", (0, 1), -1), ("beams", (a.beam, a.nbest), -1), ("beams_vocab", (a.beam, a.nbest), vocab)]

        def run(leg):
            sess.set_rec_beam(*leg[1])
            sess.set_rec_beam_vocab(leg[2], a.gamma)
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
               "beam": a.beam, "nbest": a.nbest, "gamma": a.gamma, "seed": a.seed,
               "vocab": dict(sess.vocab_info(vocab), classes=len(dic), words_asked=a.words, create_ms=create_ms)}
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
        search_v = out["beams_vocab"]["profile"].get("ctc_beam_search_vocab", {}).get("ms_per_call")
        out["vocab_cost"] = {"added_ms_per_step": out["beams_vocab"]["step_ms"]["median"] - out["beams"]["step_ms"]["median"],
                             "step_ratio": out["beams_vocab"]["step_ms"]["median"] / out["beams"]["step_ms"]["median"],
                             "search_ms_per_call": search, "search_vocab_ms_per_call": search_v,
                             "search_ratio": None if not search or search_v is None else search_v / search}
        r = run(legs[-1])   # how many hypotheses the lines report, and how many of their words are no entries
        n_h = n_oov = 0
        for i, q in enumerate(quads):
            for k in range(len(q)):
                vp = C.POINTER(retto_amd._lib.BeamVocab)()
                n = lib.rt_results_rec_beam_vocab(r, i, k, C.byref(vp))
                n_h += n
                n_oov += sum(vp[j].oov_words for j in range(n))
        lib.rt_results_free(r)
        out["beams_vocab"]["hypotheses"] = n_h
        out["beams_vocab"]["oov_words"] = n_oov
        out["new_families_when_unused"] = [f for f in FAMILIES if f in out["unused"]["profile"]]
        out["vocab_families_without_a_vocabulary"] = [f for f in out["beams"]["profile"] if f.endswith("_vocab")]
        print(json.dumps(out))
    finally:
        sess.set_rec_beam_vocab(-1)
        sess.set_rec_beam(0)
        for p in d_pages:
            lib.rt_device_free(h, C.c_void_p(p))
        sess.close()


if __name__ == "__main__":
    main()
