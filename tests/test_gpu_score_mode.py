"""score_mode Slow on the MI355X: rt_det_postprocess and the L2 batch path against the restatement in
tests/slow_score_ref.py (boxes and score bit patterns equal), and the feature's point: a curved line Fast drops and Slow keeps."""
import numpy as np
import pytest

import retto_amd
from oracle import ref_lib as R
from retto_amd import workload

import slow_score_ref as S

pytestmark = pytest.mark.gpu
f32 = np.float32


def _session(**det):
    cfg = retto_amd.synthetic_session_config(0)
    cfg.det_processor_config.score_mode = "Slow"
    for k, v in det.items():
        setattr(cfg.det_processor_config, k, v)
    return retto_amd.RettoSession(cfg)


@pytest.fixture(scope="module")
def slow():
    s = _session()
    yield s
    s.close()


@pytest.fixture(scope="module")
def slow_nodilate():
    s = _session(dilation_kernel=None)
    yield s
    s.close()


def _check(sess, pred, oh, ow, min_boxes=0, **kw):
    gb, gs = sess.det_postprocess(pred, oh, ow)
    rb, rs = S.det_postprocess(pred, oh, ow, **kw)
    assert len(gb) == len(rb), (len(gb), len(rb))
    assert np.array_equal(gb, rb), "box coordinates differ"
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), "scores differ"
    assert len(gb) >= min_boxes
    return gb, gs


def _arcs(H, W, arcs, inside=0.8, outside=0.03):
    """Thick circular arcs (cx, cy, radius, half-width, angle from, angle to) on a soft background."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.full((H, W), outside, np.float32)
    for cx, cy, r, hw, a0, a1 in arcs:
        d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
        ang = np.degrees(np.arctan2(yy - cy, xx - cx))
        m[(np.abs(d - r) < hw) & (ang >= a0) & (ang <= a1)] = inside
    return m


def _sine(H, W, lines):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.full((H, W), 0.02, np.float32)
    for y0, amp, period, hw, x0, x1 in lines:
        yc = y0 + amp * np.sin(2 * np.pi * xx / period)
        m[(np.abs(yy - yc) < hw) & (xx >= x0) & (xx <= x1)] = 0.85
    return m


def test_curved_lines_and_arcs(slow):
    m = _arcs(384, 512, [(256, 330, 200, 9, -160, -20), (120, 120, 60, 5, 0, 200), (400, 100, 70, 12, -90, 90),
                         (300, 260, 40, 3, 30, 300)])
    _check(slow, m, 384, 512, min_boxes=2)
    m = _sine(320, 640, [(60, 12, 200, 7, 20, 600), (160, 25, 300, 9, 40, 620), (260, 6, 80, 4, 10, 500)])
    rng = np.random.default_rng(3)
    m = np.clip(m + rng.normal(0, 0.06, m.shape).astype(np.float32), 0, 1).astype(np.float32)
    _check(slow, m, 480, 960, min_boxes=3)


def test_rings_holes_and_an_island(slow):
    m = _arcs(320, 320, [(90, 90, 50, 8, -180, 180), (230, 100, 30, 4, -180, 180), (160, 230, 60, 14, -180, 180)])
    m[215:245, 145:175] = 0.9   # an island inside the last ring's hole
    _check(slow, m, 320, 320, min_boxes=2)
    m = workload.planted_map(256, 320, 256, 320, [(20, 20, 300, 120)], shrink=0.0)
    m[50:90, 60:260] = 0.02
    m[60:80, 100:200] = 0.9
    _check(slow, m, 256, 320)


def test_comb_and_u_shapes(slow):
    m = np.full((200, 320), 0.02, np.float32)
    m[20:40, 20:300] = 0.9
    for x in range(20, 300, 24):
        m[40:110, x:x + 8] = 0.9   # comb teeth
    m[130:190, 30:50] = 0.9; m[130:190, 120:140] = 0.9; m[170:190, 30:140] = 0.9   # U
    m[130:190, 180:200] = 0.9; m[130:190, 280:300] = 0.9; m[130:150, 180:300] = 0.9   # upside-down U
    _check(slow, m, 200, 320, min_boxes=3)


def test_threads_and_bridges_without_dilation(slow_nodilate):
    m = np.full((160, 224), 0.02, np.float32)
    for k in range(120):
        m[20 + k // 2, 10 + k] = 0.9   # 1-pixel diagonal thread (8-connected steps)
    m[30:60, 140:170] = 0.9; m[30:60, 190:215] = 0.9; m[44, 170:190] = 0.9   # two squares, a 1-pixel bridge
    for k in range(40):
        m[100 + k, 40 + k] = 0.9; m[100 + k, 120 - k] = 0.9   # an X of threads
    m[90:150, 150:200] = 0.9; m[110:130, 165:185] = 0.02; m[120, 165:185] = 0.9   # a block with a hole cut by a thread
    rng = np.random.default_rng(4)
    m[rng.uniform(0, 1, m.shape) > 0.985] = 0.9
    _check(slow_nodilate, m, 160, 224, dilate=False)


def test_noise_and_blob_pages(slow):
    rng = np.random.default_rng(7)
    _check(slow, rng.uniform(0, 1, (160, 192)).astype(np.float32), 160, 192)
    rng = np.random.default_rng(8)
    blobs = (rng.uniform(0, 1, (40, 48)) > 0.6).astype(np.float32)
    _check(slow, np.kron(blobs, np.ones((6, 6), np.float32)) * 0.9 + 0.01, 240, 288)
    pred = (rng.uniform(0, 1, (480, 640)) > 0.93).astype(np.float32) * 0.9 + 0.01
    _check(slow, pred, 480, 640)


@pytest.mark.parametrize("seed", range(8))
def test_rotated_fuzz(slow, seed):
    rng = np.random.default_rng(1000 + seed)
    H, W = int(rng.integers(6, 24)) * 32, int(rng.integers(6, 24)) * 32
    boxes = []
    for _ in range(int(rng.integers(1, 14))):
        bw = float(rng.uniform(20, 0.6 * W)); bh = float(rng.uniform(4, 40))
        boxes.append((float(rng.uniform(0, W)), float(rng.uniform(0, H)), bw, bh, float(rng.uniform(-90, 90))))
    m = workload.planted_map_rotated(H, W, boxes)
    m = np.clip(m + rng.normal(0, 0.08, m.shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    oh, ow = int(H * rng.uniform(0.5, 1.5)), int(W * rng.uniform(0.5, 1.5))
    _check(slow, m, oh, ow)


@pytest.mark.parametrize("w", [250, 251, 252, 253])
def test_widths_mod_4(slow, w):
    rng = np.random.default_rng(w)
    h = 190
    pred = (rng.uniform(0, 1, (h, w)) > 0.975).astype(np.float32) * 0.85 + 0.02
    pred[0:9, 0:60] = 0.9; pred[h - 8:h, w - 70:w] = 0.9
    pred += _arcs(h, w, [(w / 2, h / 2, 60, 6, -170, 10)], inside=0.8, outside=0.0)
    _check(slow, np.clip(pred, 0, 1).astype(np.float32), h, w)


def test_border_hugging_contours(slow):
    m = workload.planted_map(256, 256, 256, 256, [(0, 0, 120, 30), (200, 100, 256, 140), (10, 230, 200, 256)], shrink=0.0)
    m[0:256, 0:3] = 0.9   # a strip down the left edge
    m += _arcs(256, 256, [(256, 256, 90, 6, -180, -90)], inside=0.85, outside=0.0)   # an arc into the corner
    _check(slow, np.clip(m, 0, 1).astype(np.float32), 256, 256)


def test_full_noise_page(slow):
    pred = np.random.default_rng(1).uniform(0, 1, (960, 960)).astype(np.float32)
    _check(slow, pred, 960, 960)


def test_large_blob_takes_the_global_path(slow):
    """One blob of 1984 x 1408 with a ragged edge: a long chain whose frame does not fit in LDS (k_contour_boxes_slow_big)."""
    H, W = 1408, 1984
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    r = 600 + 40 * np.sin(np.arctan2(yy - 704, xx - 992) * 9)
    m = np.where(np.sqrt((xx - 992) ** 2 / 1.7 + (yy - 704) ** 2) < r, f32(0.9), f32(0.05)).astype(np.float32)
    m[600:700, 900:1100] = 0.05   # a hole, with an island
    m[630:670, 950:1050] = 0.9
    gb, _ = _check(slow, m, H, W, min_boxes=1)


def test_one_point_chains(slow):
    """min_mini_box_size = 0 lets single pixels through the sside filter: their one-point chains are traced and score 0."""
    s = _session(min_mini_box_size=0)
    try:
        rng = np.random.default_rng(9)
        pred = np.full((96, 128), 0.05, np.float32)
        pred[rng.uniform(0, 1, pred.shape) > 0.97] = 0.9
        pred[40:60, 30:90] = 0.9
        _check(s, pred, 96, 128, min_size=0, min_boxes=1)
        _check(s, pred, 96, 128, min_size=0, min_boxes=1)
    finally:
        s.close()


def test_slow_keeps_a_curved_line_fast_drops(slow, hip_session):
    m = _arcs(256, 256, [(128, 200, 100, 6, -180, 0)], inside=0.7, outside=0.05)
    fb, fs = hip_session.det_postprocess(m, 256, 256)
    sb, ss = slow.det_postprocess(m, 256, 256)
    assert len(fb) == 0, fs
    assert len(sb) == 1 and ss[0] >= f32(0.5)
    rb, rs = S.det_postprocess(m, 256, 256)
    assert np.array_equal(sb, rb) and np.array_equal(ss.view(np.uint32), rs.view(np.uint32))


def test_l2_batches_equal_the_stage_function(slow):
    """32 planted 960 x 960 pages (curved lines among them) through rt_run_batch on 3 lanes and through two submitted batches:
    every page's boxes and det scores equal rt_det_postprocess on its map, and repeated calls are bit-identical."""
    pages, maps = [], []
    for i in range(32):
        page, rects = workload.planted_page(960, 960, 24, seed=700 + i)
        m = workload.planted_map(960, 960, 960, 960, rects)
        if i % 2 == 0:
            m = np.maximum(m, _arcs(960, 960, [(480, 1100, 500 + 20 * (i % 5), 8, -150, -30)], inside=0.75, outside=0.0))
        pages.append(page); maps.append(m.astype(np.float32))
    want = [slow.det_postprocess(m, 960, 960) for m in maps]
    assert any(len(b) for b, _ in want)

    def det(results):
        return [(np.stack([d.boxes.as_array() for d in r.det_result]) if r.det_result else np.zeros((0, 4, 2), np.float32),
                 np.array([d.score for d in r.det_result], np.float32)) for r in results]

    lib = slow._hd.lib
    first = det(slow.run_batch(pages, det_map_override=maps))
    again = det(slow.run_batch(pages, det_map_override=maps))
    for (gb, gs), (ab, as_), (wb, ws) in zip(first, again, want):
        assert np.array_equal(gb.reshape(-1, 4, 2), wb) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
        assert np.array_equal(ab, gb) and np.array_equal(as_.view(np.uint32), gs.view(np.uint32))
    halves = [(pages[:16], maps[:16]), (pages[16:], maps[16:])]
    tickets = [slow.submit_batch_raw(p, [x.shape[0] for x in p], [x.shape[1] for x in p], retto_amd.RT_MEM_HOST, mm)
               for p, mm in halves]
    got = []
    for t, (p, _) in zip(tickets, halves):
        r = slow.wait_batch_raw(t)
        for i in range(len(p)):
            k = lib.rt_results_count(r, i)
            b = np.ctypeslib.as_array(lib.rt_results_boxes(r, i), (k, 8)).copy() if k else np.zeros((0, 8), np.float32)
            s = np.ctypeslib.as_array(lib.rt_results_det_scores(r, i), (k,)).copy() if k else np.zeros(0, np.float32)
            got.append((b.reshape(-1, 4, 2), s))
        lib.rt_results_free(r)
    for (gb, gs), (wb, ws) in zip(got, want):
        assert np.array_equal(gb, wb) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
