"""score_mode Slow (DetProcessorConfig::score_mode, det_processor.rs:22-31): the restatement in tests/slow_score_ref.py, the
chain facts the device kernels rely on, hand-checked scores, and the config plumbing.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import retto_amd
from oracle import ref_lib as R
from retto_amd import _lib, cli, workload

import slow_score_ref as S

f32 = np.float32


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the restated fill on 4-point boxes
def test_polygon_fill_equals_box_score_fast_on_boxes():
    """draw_polygon (any n, interpolation branch included) scores 4-point boxes exactly as the oracle's box_score_fast."""
    rng = np.random.default_rng(5)
    H, W = 24, 28
    n = 0
    for i in range(2000):
        pred = rng.uniform(0, 1, (H, W)).astype(np.float32)
        kind = i % 5
        if kind == 0:   # random quads, partly off the map
            box = rng.integers(-6, 34, 8)
        elif kind == 1:   # rotated rectangles with floored corners (what min_area_rect gives)
            cx, cy, a, b, t = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0, 12), rng.uniform(0, 6), rng.uniform(0, np.pi)
            c, s = np.cos(t), np.sin(t)
            box = np.array([[np.floor(cx + sx * a * c - sy * b * s), np.floor(cy + sx * a * s + sy * b * c)]
                            for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]).reshape(8)
        elif kind == 2:   # degenerate: repeated corners, first == last (score 0), a single point
            p, q, r = (rng.integers(-2, 26, 2) for _ in range(3))
            box = np.array([[p, p, q, p], [p, q, q, r], [p, p, p, p], [p, q, p, q], [p, q, r, r]][i // 5 % 5]).reshape(8)
        elif kind == 3:   # collinear / flat
            y = int(rng.integers(0, H)); xs = np.sort(rng.integers(-3, W + 3, 4))
            box = np.array([[xs[0], y], [xs[1], y], [xs[2], y + int(rng.integers(0, 2))], [xs[3], y]]).reshape(8)
        else:   # thin slanted
            x0, y0 = rng.integers(0, W), rng.integers(0, H)
            dx, dy = rng.integers(-20, 21), rng.integers(-20, 21)
            box = np.array([[x0, y0], [x0 + dx, y0 + dy], [x0 + dx + 1, y0 + dy], [x0 + 1, y0]]).reshape(8)
        box = np.asarray(box, np.int32).reshape(8)
        got = S.polygon_score(pred, box.reshape(4, 2))
        ref = R.box_score_fast(pred, box)
        assert _bits(got) == _bits(ref), (i, box.tolist(), got, ref)
        n += 1
    assert n == 2000


# ---------------------------------------------------------------- the composition, run in Fast
def _maps():
    out = []
    page, rects = workload.planted_page(320, 480, lines=6, seed=3)
    out.append(("planted", workload.planted_map(320, 480, 320, 480, rects), 320, 480))
    out.append(("rotated", workload.planted_map_rotated(384, 512, [(256, 100, 150, 14, 12.0), (200, 250, 120, 10, -31.0),
                                                                   (400, 200, 100, 12, 83.0), (90, 330, 60, 9, 45.0)]), 384, 512))
    m = workload.planted_map(256, 320, 256, 320, [(20, 20, 300, 120)], shrink=0.0)
    m[50:90, 60:260] = 0.02
    m[60:80, 100:200] = 0.9
    out.append(("nested", m, 256, 320))
    rng = np.random.default_rng(7)
    out.append(("noise", rng.uniform(0, 1, (96, 128)).astype(np.float32), 96, 128))
    blobs = (rng.uniform(0, 1, (20, 24)) > 0.6).astype(np.float32)
    out.append(("blobs", np.kron(blobs, np.ones((6, 6), np.float32)) * 0.9 + 0.01, 120, 144))
    return out


@pytest.mark.parametrize("name,pred,oh,ow", _maps(), ids=lambda v: v if isinstance(v, str) else None)
def test_composition_in_fast_mode_equals_the_oracle(name, pred, oh, ow):
    gb, gs = S.det_postprocess(pred, oh, ow, score_mode="Fast")
    rb, rs = R.det_postprocess(pred, oh, ow)
    assert len(gb) == len(rb)
    assert np.array_equal(gb, rb) and np.array_equal(_bits(gs), _bits(rs))


# ---------------------------------------------------------------- the chain facts of the device kernels
def _fact_masks():
    rng = np.random.default_rng(11)
    out = [R.threshold_dilate(p, 0.3, True) for _, p, _, _ in _maps()[1:]]
    out.append(R.threshold_dilate((rng.uniform(0, 1, (64, 80)) > 0.8).astype(np.float32), 0.3, False))   # threads, diagonals
    out.append(R.threshold_dilate((rng.uniform(0, 1, (48, 64)) > 0.55).astype(np.float32), 0.3, False))  # dense, many holes
    return out


def _parity_fill(chain, w, h):
    """The device's fill: per pixel the parity of its intersection count (P) and whether it is a chain point (N)."""
    P = np.zeros((h, w), np.int64); N = np.zeros((h, w), bool)
    n = len(chain)
    for i in range(n if n > 1 else 0):
        (px, py), (qx, qy) = chain[i], chain[(i + 1) % n]
        if py == qy:
            P[py, px] ^= 1; P[qy, qx] ^= 1
        elif qy > py:
            P[py, px] ^= 1
        else:
            P[qy, qx] ^= 1
    for x, y in chain:
        N[y, x] = True
    before = (np.cumsum(P, axis=1) - P) & 1
    return (N | (before == 1)).astype(np.uint8)


@pytest.mark.parametrize("k", range(6))
def test_chain_facts_against_find_contours(k):
    """For every contour of find_contours: (1) consecutive points and last / first are 8-adjacent; (2) the chain starts at the
    root of its component (outer) or left of the root of its hole, and tracing from there with nothing but the mask gives
    the same chain -- chains are independent of each other; (3) the chain's bounding box is that of the contour's row
    extents (component pixels / foreground 4-neighbours of the hole); (4) the parity form of the fill equals draw_polygon_mut
    on the chain."""
    mask = _fact_masks()[k]
    H, W = mask.shape
    fg = S.components(mask, True)
    bg = {r: p for r, p in S.components(mask, False).items()
          if not any(x in (0, W - 1) or y in (0, H - 1) for x, y in p)}
    contours = R.find_contours(mask)
    assert len(contours) == len(fg) + len(bg)
    fast = S.find_contours(mask)   # (the restatement's own contour list, for large maps)
    assert [bt for _, bt in fast] == [bt for _, bt in contours]
    assert all(np.array_equal(a, b) for (a, _), (b, _) in zip(fast, contours))
    seen_self_touching = 0
    for pts, bt in contours:
        chain = [tuple(map(int, p)) for p in pts]
        n = len(chain)
        for i in range(n if n > 1 else 0):
            (ax, ay), (bx, by) = chain[i], chain[(i + 1) % n]
            assert max(abs(ax - bx), abs(ay - by)) == 1
        sx, sy = chain[0]
        if bt == 0:
            root = sy * W + sx
            assert root in fg
            region = fg[root]
        else:
            root = sy * W + sx + 1
            assert root in bg
            hole = set(bg[root])
            region = {(x + dx, y + dy) for x, y in hole for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))} - hole
        assert S.trace_from(mask, chain[0], bt == 0) == chain
        rx, ry = [p[0] for p in region], [p[1] for p in region]
        cx, cy = [p[0] for p in chain], [p[1] for p in chain]
        assert (min(cx), max(cx), min(cy), max(cy)) == (min(rx), max(rx), min(ry), max(ry))
        if n > 1:
            x0, y0 = min(cx), min(cy)
            rel = [(x - x0, y - y0) for x, y in chain]
            w, h = max(cx) - x0 + 1, max(cy) - y0 + 1
            want = S.draw_polygon(rel, w, h)
            assert np.array_equal(_parity_fill(rel, w, h), want)
            seen_self_touching += len(set(chain)) < n
    if k >= 4:
        assert seen_self_touching > 0   # revisited pixels (thin lines, bridges) are covered


# ---------------------------------------------------------------- hand-checked Slow scores
def _shape(name):
    """(mask, covered): `covered` is the pixel set Slow averages over, worked out by hand for the outer contour."""
    m = np.zeros((14, 16), np.uint8)
    if name == "L":
        m[2:10, 2:4] = 1; m[8:10, 2:9] = 1
        cov = m.copy()                      # the L itself: its polygon is the L
    elif name == "U":
        m[2:11, 2:4] = 1; m[2:11, 9:11] = 1; m[9:11, 2:11] = 1
        cov = m.copy()                      # the notch stays out
    elif name == "ring":
        m[2:9, 2:9] = 1; m[4:7, 4:7] = 0; m[7:9, 9:14] = 1
        cov = m.copy(); cov[4:7, 4:7] = 1   # the outer polygon covers the hole
    else:   # "bridge": two squares joined by a 1-pixel-high bridge
        m[3:7, 1:5] = 1; m[3:7, 10:14] = 1; m[4, 5:10] = 1
        cov = m.copy()                      # the bridge is walked twice; its pixels are chain points
    return m, cov


@pytest.mark.parametrize("name", ["L", "U", "ring", "bridge"])
def test_hand_checked_slow_scores(name):
    m, cov = _shape(name)
    pred = np.where(m > 0, f32(0.75), f32(0.25)).astype(np.float32)
    contours = R.find_contours(R.threshold_dilate(pred, 0.5, False))
    outer = [p for p, bt in contours if bt == 0]
    assert len(outer) == 1
    slow = S.polygon_score(pred, outer[0])
    # every covered value is a multiple of 1/4: the f32 sum is exact, the mean is one rounding of it
    want = f32(f32(0.75 * m[cov > 0].sum() + 0.25 * (cov > 0).sum() - 0.25 * m[cov > 0].sum()) / f32((cov > 0).sum()))
    assert _bits(slow) == _bits(want), (slow, want)
    box = R.min_area_rect(outer[0].astype(np.float64)).astype(np.int32).reshape(8)
    fast = R.box_score_fast(pred, box)
    assert fast < slow   # the rect takes in background the polygon leaves out
    if name == "ring":
        holes = [p for p, bt in contours if bt == 1]
        assert len(holes) == 1 and len(holes[0]) == 12   # the hole's chain: the 4-neighbours of the 3 x 3 hole (corners cut)
        assert _bits(S.polygon_score(pred, holes[0])) == _bits(f32(f32(12 * 0.75 + 9 * 0.25) / f32(21)))   # 5 x 5 less 4 corners


def test_one_point_chain_scores_zero():
    pred = np.full((8, 8), 0.1, np.float32); pred[3, 4] = 0.9
    (pts, bt), = R.find_contours(R.threshold_dilate(pred, 0.5, False))
    assert len(pts) == 1 and bt == 0
    assert S.polygon_score(pred, pts) == 0.0


def test_slow_keeps_a_curved_line_fast_drops():
    """The restatement shows the point of the mode: an arc whose rect mean is below box_thresh and polygon mean above."""
    pred = _arc_map()
    fb, _ = S.det_postprocess(pred, 256, 256, score_mode="Fast")
    sb, ss = S.det_postprocess(pred, 256, 256)
    assert len(fb) == 0 and len(sb) == 1 and ss[0] >= f32(0.5)


def _arc_map():
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float32)
    r = np.sqrt((xx - 128) ** 2 + (yy - 200) ** 2)
    arc = (np.abs(r - 100) < 6) & (yy < 170)
    return np.where(arc, f32(0.7), f32(0.05)).astype(np.float32)


# ---------------------------------------------------------------- config plumbing
def test_score_mode_defaults_to_fast():
    assert retto_amd.DetProcessorConfig().score_mode == "Fast"
    c = _lib.Config()
    _lib.load().rt_config_default(C.byref(c))
    assert c.det_score_mode == 0
    assert cli.build_parser().parse_args(["-i", "x"]).det_score_mode == "Fast"
    assert cli.build_parser().parse_args(["-i", "x", "--det-score-mode", "Slow"]).det_score_mode == "Slow"


def test_rt_create_rejects_an_unknown_score_mode():
    """Checked before any device is touched: RT_ERR_INVALID on any machine."""
    lib = _lib.load()
    lib.rt_create.argtypes = [C.POINTER(_lib.Config), C.POINTER(C.c_void_p)]
    lib.rt_last_error.restype = C.c_char_p
    for bad in (2, -1):
        c = _lib.Config(); lib.rt_config_default(C.byref(c)); c.det_score_mode = bad
        out = C.c_void_p()
        assert lib.rt_create(C.byref(c), C.byref(out)) == 8 and not out.value
        assert b"det_score_mode" in lib.rt_last_error(None)


@pytest.mark.parametrize("bad", ["slow", "SLOW", "", "Polygon", 1])
def test_bad_score_mode_string_raises_invalid_argument(bad):
    cfg = retto_amd.synthetic_session_config(0)
    cfg.det_processor_config.score_mode = bad
    with pytest.raises(retto_amd.InvalidArgument):
        retto_amd.RettoSession(cfg)
