"""rt_config.crop_source = Original and the flat warp kernel on the GPU.  Every comparison is exact: the kernels are
deterministic, the two warp launches share their per-pixel code, and the oracle chain is teacher-forced with the HIP networks."""
import io
import math

import numpy as np
import pytest

import retto_amd
from oracle import ref_lib as R
from retto_amd import workload

import crop_source_cases as CS

pytestmark = pytest.mark.gpu


def _session(crop_source, max_side_len=2000, lanes=0, full=True):
    cfg = retto_amd.synthetic_session_config(0, crop_source=crop_source, max_side_len=max_side_len, lanes=lanes)
    if full:
        cfg.rec_processor_config.return_word_box = True
        cfg.rec_processor_config.return_candidates = 3
    return retto_amd.RettoSession(cfg)


@pytest.fixture(scope="module")
def original_small():
    """Original mode, pages above 512 are shrunk for the detector, three lanes, word boxes and candidates on."""
    s = _session("Original", CS.SMALL_LIMIT, lanes=3)
    yield s
    s.close()


# ---------------------------------------------------------------- k_warp_crops_flat against k_warp_crops and the oracle
def _rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float32)


def _rot(cx, cy, bw, bh, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    pts = [(-bw / 2, -bh / 2), (bw / 2, -bh / 2), (bw / 2, bh / 2), (-bw / 2, bh / 2)]
    return np.array([[cx + x * c - y * s, cy + x * s + y * c] for x, y in pts], np.float32)


_TINY = [_rect(10 + 9 * i, 150 + 3 * (i % 3), 16.5 + 9 * i, 154.5 + 3 * (i % 3)) for i in range(10)]   # ten crops of 6 x 4
_WARP_CASES = {
    # 3 x 24 = 72 output pixels: the whole call is one partly filled workgroup
    "fewer_than_256_pixels": _TINY[:3],
    # 70 x 9 = 630 then 6 x 4: the boundary between two crops falls inside the third workgroup
    "boundary_inside_a_block": [_rect(20, 20, 90.5, 29.5), _TINY[0], _rect(100, 40, 180.5, 52.5)],
    "tall_quad_is_rotated270": [_rect(50, 20, 60.5, 80.5), _TINY[1]],
    "rotated_17_degrees": [_rot(160, 100, 120, 18, 17.0), _rect(30, 60, 80.5, 70.5)],
    "touches_the_page_border": [_rect(0, 0, 100, 12), _rect(250, 180, 319, 199), _rot(300, 30, 60, 14, -25.0)],
    "one_crop": [_rot(150, 120, 90, 16, 17.0)],
    "one_long_crop_beside_ten_tiny_ones": _TINY[:5] + [_rect(10, 100, 310.5, 120.5)] + _TINY[5:],
}


@pytest.mark.parametrize("name", list(_WARP_CASES))
def test_flat_warp_equals_row_warp_and_the_oracle(hip_session, name):
    page = workload.noise_page(200, 320, 5)
    boxes = np.stack(_WARP_CASES[name])
    rows = hip_session.crop_images(page, boxes, form=0)
    flat = hip_session.crop_images(page, boxes, form=1)
    assert len(rows) == len(flat) == len(boxes)
    for b, a, f in zip(boxes, rows, flat):
        ref = R.get_crop_img(page, b)
        assert a.shape == f.shape == ref.shape and ref.size > 0
        assert np.array_equal(f, a)
        assert np.array_equal(f, ref)
    if name == "tall_quad_is_rotated270":
        assert flat[0].shape[1] > flat[0].shape[0]   # 10 x 60 came out as 60 wide
    if name == "fewer_than_256_pixels":
        assert sum(f.shape[0] * f.shape[1] for f in flat) < 256
    if name == "touches_the_page_border":
        assert (flat[0][0] == 255).all()   # the bicubic taps of the first row leave the page: white


def test_flat_warp_grid_stride_loop(hip_session):
    """One quad over nearly all of a 2100 x 2100 page: 2095 x 2095 = 4.39 M output pixels = 17145 workgroups of 256, more than the
    16384 the launch is capped at, so the grid-stride loop runs a second sweep."""
    page = workload.noise_page(2100, 2100, 6)
    box = _rect(2, 2, 2097.5, 2097.5)[None]
    assert (2095 * 2095 + 255) // 256 > 16384
    a = hip_session.crop_images(page, box, form=0)[0]
    f = hip_session.crop_images(page, box, form=1)[0]
    assert f.shape == (2095, 2095, 3)
    assert np.array_equal(f, a)


# ---------------------------------------------------------------- Original equals Resized where nothing is resized
def test_original_equals_resized_on_pages_within_the_limits():
    p1, m1 = CS.planted_for(320, 480, 3, 51)
    p2 = workload.noise_page(416, 608, 52)
    dh, dw = R.resize_either_dims(416, 608)
    sy, sx = dh / 416, dw / 608
    m2 = workload.planted_map_rotated(dh, dw, [(300 * sx, 80 * sy, 200 * sx, 16 * sy, 9.0), (200 * sx, 250 * sy, 150 * sx, 14 * sy, -21.0),
                                               (520 * sx, 300 * sy, 90 * sy, 12 * sx, 90.0)])
    got = []
    for mode in ("Resized", "Original"):
        s = _session(mode)
        try:
            got.append(s.run_batch([p1, p2], det_map_override=[m1, m2]))
        finally:
            s.close()
    assert len(got[0][0].rec_result) == 3 and len(got[0][1].rec_result) >= 2
    for a, b in zip(*got):
        assert all(g.words is not None and g.candidates is not None for g in a.rec_result)
        assert CS.digest(a) == CS.digest(b)


# ---------------------------------------------------------------- a resized page against the oracle chain on the original page
def test_original_mode_against_the_oracle_on_the_original_page(models, original_small):
    from oracle.pipeline import OracleSession
    page, m = CS.page_with_tall_line()
    assert R.resize_both_plan(620, 1000, CS.SMALL_LIMIT, 30)[-1] == (288, 512)
    oracle = OracleSession(*models, max_side_len=CS.SMALL_LIMIT)
    w = original_small.worker
    oracle.det_worker, oracle.cls_worker, oracle.rec_worker = w.det, w.cls, w.rec   # teacher-forced
    o = oracle.run(page, det_map_override=m)
    boxes_ori = o.det_boxes
    assert len(boxes_ori) == 6
    assert [R.crop_dims(b)[2] for b in boxes_ori].count(True) == 1   # the tall line: rotate270 decided on the original-coordinate quad
    crops = [R.get_crop_img(page, b) for b in boxes_ori]
    dims = [c.shape[:2] for c in crops]
    labels, _ = oracle.cls_process(crops, dims)
    toks, _, _ = oracle.rec_process(crops, dims)

    r = original_small.run_batch([page], det_map_override=[m])[0]
    assert np.array_equal(np.stack([d.boxes.as_array() for d in r.det_result]), boxes_ori)
    assert [c.label.label for c in r.cls_result] == list(labels)
    for k, (g, t) in enumerate(zip(r.rec_result, toks)):
        assert np.array_equal(g.tokens, t), f"line {k}"

    # the default mode reads the shrunk page: same boxes, other crops, other tokens
    s = _session("Resized", CS.SMALL_LIMIT, full=False)
    try:
        d = s.run_batch([page], det_map_override=[m])[0]
    finally:
        s.close()
    assert np.array_equal(np.stack([x.boxes.as_array() for x in d.det_result]), boxes_ori)
    assert [g.tokens.tolist() for g in d.rec_result] == [t.tolist() for t in o.rec_tokens]
    assert any(not np.array_equal(a.tokens, b.tokens) for a, b in zip(d.rec_result, r.rec_result))


# ---------------------------------------------------------------- batches, lanes, entry points
def _batch():
    p0, m0 = CS.page_with_tall_line()
    p1, m1 = CS.planted_for(700, 540, 4, 61, CS.SMALL_LIMIT, (3.0, 10.0))
    p2, m2 = CS.planted_for(320, 480, 3, 62, CS.SMALL_LIMIT)
    p3 = np.zeros((200, 300, 3), np.uint8)
    m3 = np.zeros(R.resize_either_dims(200, 300), np.float32)
    return [p0, p1, p2, p3], [m0, m1, m2, m3]


def test_original_mode_batch_over_three_lanes(original_small):
    pages, maps = _batch()
    res = original_small.run_batch(pages, det_map_override=maps)
    assert [len(r.rec_result) for r in res] == [6, 4, 3, 0]
    # a page alone equals the page inside the batch, bit for bit: every GEMM route gives a row the same bits whatever the row count
    for i, (p, m) in enumerate(zip(pages, maps)):
        alone = original_small.run_batch([p], det_map_override=[m])[0]
        a, b = CS.digest(alone), CS.digest(res[i])
        assert a == b, f"page {i}: {CS.differing(a, b)}"
    # submit / wait: the pages are staged in HBM by the submitting thread, the lanes cut from the staged originals
    t = original_small.submit_batch_raw(pages, [p.shape[0] for p in pages], [p.shape[1] for p in pages], det_map_override=maps)
    waited = original_small.wait_batch(t)
    assert [CS.digest(a) for a in waited] == [CS.digest(b) for b in res]


def test_original_mode_encoded_pages(original_small):
    """Encoded entry points take no map override, so the boxes are the synthetic-weight detector's own: it reports one
    whole-page box on a page that is black but for thin stripes (and on a black page), nothing on the planted pages.  Three of
    the four pages are above the size limit: their line is cut from the decoded original, stripes and all."""
    from PIL import Image
    h16 = np.zeros((620, 1000, 3), np.uint8); h16[::16] = 255
    v16 = np.zeros((620, 1000, 3), np.uint8); v16[:, ::16] = 255
    pages = [h16, v16, np.zeros((700, 900, 3), np.uint8), np.zeros((200, 300, 3), np.uint8)]
    files = []
    for p in pages:
        b = io.BytesIO(); Image.fromarray(p).save(b, format="PNG"); files.append(b.getvalue())
    ref = original_small.run_batch(pages)
    assert [len(r.rec_result) for r in ref] == [1, 1, 1, 1]
    # the crops' pixels reach the recogniser: horizontal and vertical stripes read differently (a score is continuous in them)
    assert ref[0].rec_result[0].score != ref[1].rec_result[0].score
    enc = original_small.run_encoded_batch(files)
    assert [CS.digest(a) for a in enc] == [CS.digest(b) for b in ref]
    sub = original_small.wait_batch(original_small.submit_encoded_batch(files))
    assert [CS.digest(a) for a in sub] == [CS.digest(b) for b in ref]
