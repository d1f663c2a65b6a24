"""Pages, maps and result digests shared by test_gpu_crop_source.py and test_gpu_regions.py (not a test module)."""
import numpy as np

from oracle import ref_lib as R
from retto_amd import workload

SMALL_LIMIT = 512   # max_side_len of the sessions that must shrink a page: keeps every page of these tests small


def planted_for(page_h, page_w, lines, seed, max_side=2000, ratio_range=(3.0, 20.0)):
    """page + planted map at the det-input size a session with that max_side_len derives for it."""
    page, rects = workload.planted_page(page_h, page_w, lines, seed, ratio_range)
    return page, map_for(page_h, page_w, rects, max_side)


def map_for(page_h, page_w, rects, max_side=2000):
    plan = R.resize_both_plan(page_h, page_w, max_side, 30)
    ah, aw = plan[-1] if plan else (page_h, page_w)
    dh, dw = R.resize_either_dims(ah, aw)
    return workload.planted_map(dh, dw, page_h, page_w, rects)


def page_with_tall_line(seed=7):
    """620 x 1000: five horizontal lines in the left 840 columns and one tall line (40 x 320: h / w = 8) to their right.  With
    max_side_len = 512 it resizes to 288 x 512, at unequal ratios (0.4645 down, 0.512 across)."""
    h, w = 620, 1000
    left, rects = workload.planted_page(h, 840, 5, seed, (3.0, 12.0))
    page = np.zeros((h, w, 3), np.uint8)
    page[:, :840] = left
    x0, y0, x1, y1 = 900, 100, 940, 420
    tex = np.random.default_rng(seed + 1).integers(120, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    tex[::7, :] //= 3
    page[y0:y1, x0:x1] = tex
    m = map_for(h, w, rects, SMALL_LIMIT)
    # (planted_map shrinks by a fraction of the HEIGHT, which would erase a tall line: its kernel is shrunk by its width here)
    sy, sx, d = m.shape[0] / h, m.shape[1] / w, 0.12 * (x1 - x0)
    m[int(round((y0 + d) * sy)):int(round((y1 - d) * sy)), int(round((x0 + d) * sx)):int(round((x1 - d) * sx))] = 0.92
    return page, m


def _bits(a, dtype=np.float32):
    return np.ascontiguousarray(a, dtype).view(np.uint32).tolist()


def digest(r, boxes=True):
    """Everything a RettoWorkerResult holds, one entry per line under every key, floats as their bit patterns (NaN equals NaN).
    boxes=False leaves out the boxes and their det scores (regions report 1.0 where the detector reports its own)."""
    d = {}
    if boxes:
        d["boxes"] = [_bits(x.boxes.as_array()) for x in r.det_result]
        d["det_scores"] = _bits([x.score for x in r.det_result])
    d["labels"] = [c.label.label for c in r.cls_result]
    d["tokens"] = [g.tokens.tolist() for g in r.rec_result]
    d["text"] = [g.text for g in r.rec_result]
    d["cls_scores"] = _bits([c.label.score for c in r.cls_result])
    d["rec_scores"] = _bits([g.score for g in r.rec_result])
    d["words"] = [None if g.words is None else
                  [(w.text, _bits(w.box.as_array()), w.kind, w.first_token, w.n_tokens, w.first_col, w.last_col) for w in g.words]
                  for g in r.rec_result]
    d["cands"] = [None if g.candidates is None else
                  ([[(i, _bits([p])[0]) for i, _t, p in tok] for tok in g.candidates], g.token_cols.tolist())
                  for g in r.rec_result]
    return d


def differing(a, b):
    """the keys under which two digests differ, with the indices of the differing lines (for a failing test's message)"""
    return {k: [i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y] or "length" for k in a if a[k] != b[k]}
