"""Independent restatement of DB post-processing with score_mode Slow (test helper, not a test module).

Slow is det_processor.rs:188-221 box_score_fast applied to a contour's full point chain (the doc comment of ScoreMode::Slow,
det_processor.rs:22-31: the mean over "all pixels within the original polygon").  Everything else is composed from the
oracle's primitives (oracle.ref_lib) in the order of orc_det_postprocess (oracle/retto_oracle.cpp), with the score step
swapped.  `draw_polygon` is imageproc 0.25 draw_polygon_mut for any number of points; it assumes nothing about the input
(no 8-adjacency), so it also scores 4-point boxes and can be checked against ref_lib.box_score_fast.
"""
from __future__ import annotations

import numpy as np

from oracle import ref_lib as R

f32 = np.float32


def _rs_round_i32(v: np.float32) -> int:
    """Rust f32::round (half away from zero) then `as i32` (saturating)."""
    r = float(np.floor(abs(float(v)) + 0.5)) * (1.0 if v >= 0 else -1.0)   # (exact: |v| + 0.5 is exact in f64 for an f32 v)
    return int(max(-2 ** 31, min(2 ** 31 - 1, r)))


def _bresenham(x0, y0, x1, y1):
    """imageproc BresenhamLineIter (f32 state) from (x0, y0) to (x1, y1)."""
    x0, y0, x1, y1 = f32(x0), f32(y0), f32(x1), f32(y1)
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, x1, y0, y1 = x1, x0, y1, y0
    dx, dy = f32(x1 - x0), f32(abs(y1 - y0))
    x, y, end_x = int(x0), int(y0), int(x1)
    error = f32(dx / f32(2))
    step = 1 if y0 < y1 else -1
    while x <= end_x:
        yield (y, x) if steep else (x, y)
        x += 1
        error = f32(error - dy)
        if error < 0:
            y += step
            error = f32(error + dx)


def draw_polygon(poly, width: int, height: int):
    """imageproc 0.25 draw_polygon_mut with colour 1 on a width x height u8 canvas; None where the crate panics (first point
    == last point)."""
    poly = [(int(p[0]), int(p[1])) for p in poly]
    canvas = np.zeros((height, width), np.uint8)
    if not poly:
        return canvas
    if poly[0] == poly[-1]:
        return None
    y_min = max(0, min(min(p[1] for p in poly), height - 1))
    y_max = max(0, min(max(p[1] for p in poly), height - 1))
    closed = poly + [poly[0]]
    edges = list(zip(closed[:-1], closed[1:]))
    rows = {}   # the per-row scan of every edge, visited edge by edge: the order inside a row does not matter (sorted below)
    for p0, p1 in edges:
        for y in range(max(y_min, min(p0[1], p1[1])), min(y_max, max(p0[1], p1[1])) + 1):
            inter = rows.setdefault(y, [])
            if p0[1] == p1[1]:
                inter += [p0[0], p1[0]]
            elif p0[1] == y or p1[1] == y:
                if p1[1] > y:
                    inter.append(p0[0])
                if p0[1] > y:
                    inter.append(p1[0])
            else:
                fraction = f32(f32(y - p0[1]) / f32(p1[1] - p0[1]))
                x = f32(f32(p0[0]) + f32(fraction * f32(p1[0] - p0[0])))
                inter.append(_rs_round_i32(x))
    for y, inter in rows.items():
        inter.sort()
        assert len(inter) % 2 == 0   # (chunks(2) of an odd list would panic: a closed polygon never gives one)
        for k in range(0, len(inter), 2):
            lo, hi = min(inter[k], width), min(inter[k + 1], width - 1)
            if lo < width and hi >= 0:
                lo, hi = max(0, lo), max(0, hi)
                canvas[y, lo:hi + 1] = 1
    for p0, p1 in edges:
        for x, y in _bresenham(p0[0], p0[1], p1[0], p1[1]):
            if 0 <= x < width and 0 <= y < height:
                canvas[y, x] = 1
    return canvas


def masked_mean(pred: np.ndarray, x0: int, y0: int, canvas: np.ndarray) -> np.float32:
    """box_score_fast's sum: f32, sequential, row-major over the canvas, each pixel adding v * mask; sum / count."""
    h, w = canvas.shape
    terms = (pred[y0:y0 + h, x0:x0 + w].astype(f32) * canvas.astype(f32)).reshape(-1)
    count = int(canvas.sum())
    if count == 0:
        return f32(0.0)
    s = np.add.accumulate(np.concatenate([np.zeros(1, f32), terms]), dtype=f32)[-1]   # np.add.accumulate is sequential
    return f32(f32(s) / f32(count))


def polygon_score(pred: np.ndarray, pts) -> np.float32:
    """det_processor.rs:188-221 box_score_fast over the polygon `pts` (n x 2 ints); 0 where draw_polygon_mut would panic."""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    H, W = pred.shape
    x_min, x_max = int(np.clip(pts[:, 0].min(), 0, W - 1)), int(np.clip(pts[:, 0].max(), 0, W - 1))
    y_min, y_max = int(np.clip(pts[:, 1].min(), 0, H - 1)), int(np.clip(pts[:, 1].max(), 0, H - 1))
    canvas = draw_polygon(pts - np.array([x_min, y_min]), x_max - x_min + 1, y_max - y_min + 1)
    if canvas is None:
        return f32(0.0)
    return masked_mean(pred, x_min, y_min, canvas)


def _euclid(ax, ay, bx, by):
    dx, dy = f32(f32(ax) - f32(bx)), f32(f32(ay) - f32(by))
    return f32(np.sqrt(f32(f32(dx * dx) + f32(dy * dy))))


def _side_len(a, b):
    dx, dy = float(f32(a[0] - b[0])), float(f32(a[1] - b[1]))
    return f32(np.sqrt(dx * dx + dy * dy))


def _merge_sort(items, less):
    """The stable bottom-up merge sort (run widths 1, 2, 4, ...) of orc_det_postprocess / k_sort_boxes."""
    src = list(items)
    n = len(src)
    width = 1
    while width < n:
        dst = []
        for lo in range(0, n, 2 * width):
            mid, hi = min(lo + width, n), min(lo + 2 * width, n)
            i, j = lo, mid
            while i < mid and j < hi:
                if less(src[j], src[i]):
                    dst.append(src[j]); j += 1
                else:
                    dst.append(src[i]); i += 1
            dst += src[i:mid] + src[j:hi]
        src = dst
        width *= 2
    return src


def det_postprocess(pred, ori_h, ori_w, thresh=0.3, box_thresh=0.5, unclip_ratio=1.6, min_size=3, dilate=True,
                    score_mode="Slow"):
    """a5 with the given score mode: (boxes [n,4,2] f32, scores [n] f32).  score_mode "Fast" must reproduce
    ref_lib.det_postprocess bit for bit (that validates the composition)."""
    pred = np.ascontiguousarray(pred, f32)
    h, w = pred.shape
    mask = R.threshold_dilate(pred, thresh, dilate)
    res = []
    for pts, _bt in find_contours(mask):
        box = R.min_area_rect(pts.astype(np.float64)).astype(np.int32).reshape(8)
        sside = min(_euclid(box[0], box[1], box[2], box[3]), _euclid(box[6], box[7], box[4], box[5]))
        if sside < f32(min_size):
            continue
        score = f32(R.box_score_fast(pred, box)) if score_mode == "Fast" else polygon_score(pred, pts)
        if score < f32(box_thresh):
            continue
        off = R.unclip(box, unclip_ratio)
        if len(off) == 0:
            continue
        b = R.min_area_rect(off.astype(np.float64)).astype(f32).reshape(8)
        if min(_euclid(b[0], b[1], b[2], b[3]), _euclid(b[6], b[7], b[4], b[5])) < f32(min_size + 2):
            continue
        b = R.scale_and_clip(b, w, h, ori_w, ori_h).reshape(8)
        if _side_len(b[0:2], b[6:8]) <= f32(3) or _side_len(b[0:2], b[2:4]) <= f32(3):
            continue
        res.append((b, score))

    def less(a, b):
        ya, yb = f32(f32(a[0][1] + a[0][5]) / f32(2)), f32(f32(b[0][1] + b[0][5]) / f32(2))
        if abs(f32(ya - yb)) < f32(10):
            return f32(f32(a[0][0] + a[0][4]) / f32(2)) < f32(f32(b[0][0] + b[0][4]) / f32(2))
        return ya < yb

    res = _merge_sort(res, less)
    boxes = np.array([r[0] for r in res], f32).reshape(-1, 4, 2)
    return boxes, np.array([r[1] for r in res], f32)


# ---- the chain facts the device kernels rely on (retto_amd/csrc/dbpost_kernels.hip, score_mode Slow) ----------------
DIRS = [(-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1)]   # W NW N NE E SE S SW


def trace_from(mask: np.ndarray, start, outer: bool):
    """find_contours' border following from `start`, entered from W (outer) or E (hole), asking of every pixel only whether
    it is nonzero -- the form the device traces every chain in, independently of the others."""
    H, W = mask.shape
    nz = lambda x, y: 0 <= x < W and 0 <= y < H and mask[y, x] != 0
    cx, cy = start
    d = 0 if outer else 4
    for k in range(8):
        dd = (d + k) % 8
        if nz(cx + DIRS[dd][0], cy + DIRS[dd][1]):
            break
    else:
        return [(cx, cy)]
    p1 = (cx + DIRS[dd][0], cy + DIRS[dd][1])
    chain, (x, y), dv = [], (cx, cy), dd
    while True:
        chain.append((x, y))
        for k in range(1, 9):
            d4 = (dv - k) % 8
            if nz(x + DIRS[d4][0], y + DIRS[d4][1]):
                break
        nx, ny = x + DIRS[d4][0], y + DIRS[d4][1]
        if (nx, ny) == (cx, cy) and (x, y) == p1:
            break
        dv = (d4 + 4) % 8
        x, y = nx, ny
    return chain


def components(mask: np.ndarray, fg: bool):
    """Connected components (8-connected foreground / 4-connected background) as {root raster index: pixel list}; the root
    is the component's first pixel in raster order."""
    H, W = mask.shape
    want = (mask != 0) if fg else (mask == 0)
    seen = np.zeros((H, W), bool)
    nb = [(dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx or dy) and (fg or dx == 0 or dy == 0)]
    out = {}
    for y0 in range(H):
        for x0 in range(W):
            if not want[y0, x0] or seen[y0, x0]:
                continue
            stack, pix = [(x0, y0)], []
            seen[y0, x0] = True
            while stack:
                x, y = stack.pop()
                pix.append((x, y))
                for dx, dy in nb:
                    u, v = x + dx, y + dy
                    if 0 <= u < W and 0 <= v < H and want[v, u] and not seen[v, u]:
                        seen[v, u] = True
                        stack.append((u, v))
            out[y0 * W + x0] = pix
    return out


def find_contours(mask: np.ndarray):
    """R.find_contours' list (chains and border types, discovery order) for maps of any size: ref_lib re-runs the whole
    Suzuki-Abe pass per contour, which takes minutes on a 960 x 960 noise page.  One contour per foreground component
    (8-connected; start = its root, entered from W) and per hole (4-connected background off the frame; start = the pixel
    left of its root, entered from E), in raster order of the start pixels.  test_score_mode_cpu checks it against
    R.find_contours."""
    from scipy import ndimage
    mask = np.asarray(mask)
    H, W = mask.shape
    fg = mask != 0
    starts = []
    lab, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    if n:
        _, first = np.unique(lab.ravel(), return_index=True)
        starts += [(int(i), True) for i in first[1:]] if lab.ravel()[first[0]] == 0 else [(int(i), True) for i in first]
    blab, bn = ndimage.label(~fg)
    if bn:
        frame = set(np.unique(np.concatenate([blab[0], blab[-1], blab[:, 0], blab[:, -1]])).tolist())
        labels, first = np.unique(blab.ravel(), return_index=True)
        starts += [(int(i) - 1, False) for l, i in zip(labels.tolist(), first.tolist()) if l != 0 and l not in frame]
    starts.sort()
    return [(np.array(trace_from(mask, (i % W, i // W), outer), np.int32).reshape(-1, 2), 0 if outer else 1) for i, outer in starts]
