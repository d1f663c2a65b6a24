"""Det tiles (retto_amd/csrc/det_tiles.h) on the GPU: the stitch against the numpy selection of det_tiles_ref bit for bit, every
tile's map against the fp32 oracle on the numpy-cut tile, untiled pages and tiles-off runs untouched, the pipeline teacher-forced
against the oracle, mixed calls of tiled and untiled pages against each page alone, the setter's guard, and a large planted map
through DB post-processing.

One deviation from the issue's list.  Its mixed call names a 320 x 416 page as "untiled after the upscale"; under the default det
limit (Min 736) that page becomes 736 x 960 and IS tiled by (384, 64), and at its own size it is 416 wide, still more than 384.
The mixed sessions here lower the det limit to 320 so that pages keep their sizes: the 320 x 416 page is then tiled in one
direction only (one tile row shorter than the tile), and a fifth page of 320 x 384 is the untiled one."""
import numpy as np
import pytest
import torch

from oracle import nets_torch as N
from oracle import ref_lib as R
import retto_amd
from retto_amd import workload

import det_tiles_ref as TR

pytestmark = pytest.mark.gpu

DET_ATOL = 1e-4   # the project's bound for the fp32 DB probability map (tests/test_gpu_parity.py test_det_net)
CASES = [(160, 224, 96, 32), (160, 224, 64, 0), (160, 224, 128, 64), (64, 224, 96, 32), (224, 96, 96, 32)]
CASE_TILES = [(2, 3), (3, 4), (2, 3), (1, 3), (3, 1)]


def _rand_page(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _session(**kw):
    limit = kw.pop("det_limit", None)
    cfg = retto_amd.synthetic_session_config(0, **kw)
    if limit is not None:
        cfg.det_processor_config.limit_side_len = limit
    return retto_amd.RettoSession(cfg)


@pytest.fixture(scope="module")
def s32():
    """fp32, one lane, default det limits"""
    s = _session(lanes=1)
    yield s
    s.close()


@pytest.fixture(scope="module")
def s16():
    s = _session(lanes=1, dtype="f16")
    yield s
    s.close()


@pytest.fixture(scope="module")
def tile_runs(s32):
    """debug_det_tiles of every case on the fp32 session, computed once"""
    out = []
    for k, (h, w, T, O) in enumerate(CASES):
        img = _rand_page(h, w, 500 + k)
        s32.set_det_tiles(T, O)
        assert s32.det_tiles == (T, O)
        out.append((img,) + s32.debug_det_tiles(img))
    s32.set_det_tiles(0)
    return out


def _calls(prof, name):
    return prof.get(name, (0.0, 0))[1]


def _same(a, b, same_call=True):
    """two RettoWorkerResults equal bit for bit: boxes, det scores, labels, tokens.  same_call: the two come from calls with the
    same pages, so the cls and rec launch groups are the same too and the two networks' scores are compared bit for bit as well;
    across calls of different composition (a page inside a batch and alone) the cls / rec GEMMs run at other shapes and their
    scores may differ in the last bits, with or without tiles (test_pipeline_mixed_sizes_c4 compares the discrete results too)."""
    assert len(a.det_result) == len(b.det_result)
    for x, y in zip(a.det_result, b.det_result):
        assert np.array_equal(x.boxes.as_array(), y.boxes.as_array())
        assert np.float32(x.score).tobytes() == np.float32(y.score).tobytes()
    assert [c.label.label for c in a.cls_result] == [c.label.label for c in b.cls_result]
    for x, y in zip(a.rec_result, b.rec_result):
        assert np.array_equal(x.tokens, y.tokens)
    if same_call:
        assert [np.float32(c.label.score).tobytes() for c in a.cls_result] == [np.float32(c.label.score).tobytes() for c in b.cls_result]
        assert [np.float32(x.score).tobytes() for x in a.rec_result] == [np.float32(y.score).tobytes() for y in b.rec_result]


# ---- 1. the stitch is a selection ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=["%dx%d-%d-%d" % c for c in CASES])
def test_stitch_is_a_selection(tile_runs, k):
    h, w, T, O = CASES[k]
    img, tiles, page, plan = tile_runs[k]
    assert plan == TR.page_plan(h, w, T, O)
    assert (len(plan["row_origins"]), len(plan["col_origins"])) == CASE_TILES[k] and len(tiles) == CASE_TILES[k][0] * CASE_TILES[k][1]
    assert np.isfinite(tiles).all()
    want = TR.stitch(tiles, plan, h, w)
    assert not np.isnan(want).any()                     # the ownership rectangles cover the page
    assert page.tobytes() == want.tobytes()


@pytest.mark.parametrize("k", range(len(CASES)), ids=["%dx%d-%d-%d" % c for c in CASES])
def test_stitch_is_a_selection_f16(s16, k):
    h, w, T, O = CASES[k]
    img = _rand_page(h, w, 600 + k)
    s16.set_det_tiles(T, O)
    tiles, page, plan = s16.debug_det_tiles(img)
    s16.set_det_tiles(0)
    assert len(tiles) == CASE_TILES[k][0] * CASE_TILES[k][1] and np.isfinite(tiles).all()
    assert page.tobytes() == TR.stitch(tiles, plan, h, w).tobytes()


# ---- 2. every tile against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=["%dx%d-%d-%d" % c for c in CASES])
def test_tiles_equal_the_oracle_on_the_cut_tile(tile_runs, oracle_session, k):
    img, tiles, page, plan = tile_runs[k]
    cuts = TR.cut(img, plan)
    assert len(cuts) == len(tiles)
    for i, (c, got) in enumerate(zip(cuts, tiles)):
        x = R.det_preprocess(np.ascontiguousarray(c), limit_len=32)   # (limit 32: the tile keeps its size)
        assert x.shape[2:] == got.shape
        ref = N.det_forward(oracle_session.wd, torch.from_numpy(x)).numpy()[0, 0]
        err = float(np.abs(got - ref).max())
        print("case %d tile %d max abs err %.3e" % (k, i, err))
        assert err <= DET_ATOL, (k, i, err)


# ---- 3. untiled pages are untouched ----------------------------------------------------------------------------------------
def test_untiled_pages_and_tiles_off_launch_nothing_new():
    s = _session(lanes=1, det_limit=320)
    try:
        page = _rand_page(320, 384, 71)                  # det size 320 x 384: fits into one 384 tile
        big = _rand_page(736, 800, 72)
        s.profile_enable()
        off = s.run_batch([page])[0]; cs_off = s.last_det_checksum
        s.run_batch([big])
        prof = s.profile_get()
        assert _calls(prof, "det_tile_cut") == 0 and _calls(prof, "det_tile_stitch") == 0 and _calls(prof, "net/det") == 2
        s.set_det_tiles(384, 64)
        s.profile_enable()
        on = s.run_batch([page])[0]; cs_on = s.last_det_checksum
        prof = s.profile_get()
        assert _calls(prof, "det_tile_cut") == 0 and _calls(prof, "det_tile_stitch") == 0 and _calls(prof, "net/det") == 1
        _same(on, off)
        assert np.float64(cs_on).tobytes() == np.float64(cs_off).tobytes()
        s.profile_enable()
        s.run_batch([big])
        prof = s.profile_get()                           # (and the labels do appear when a page is tiled)
        assert _calls(prof, "det_tile_cut") == 1 and _calls(prof, "det_tile_stitch") == 1 and _calls(prof, "net/det") == 1
        tiles, stitched, plan = s.debug_det_tiles(page)  # an untiled page: one tile, its whole map
        assert tiles.shape == (1, 320, 384) and tiles[0].tobytes() == stitched.tobytes()
    finally:
        s.close()


# ---- 4. the pipeline, teacher-forced ---------------------------------------------------------------------------------------
def _assert_page_equal(r, o):
    assert len(r.det_result) == len(o.det_boxes)
    if len(o.det_boxes):
        assert np.array_equal(np.stack([d.boxes.as_array() for d in r.det_result]), o.det_boxes)
    assert [c.label.label for c in r.cls_result] == list(o.cls_labels)
    for g, ot in zip(r.rec_result, o.rec_tokens):
        assert np.array_equal(g.tokens, ot)


def test_pipeline_teacher_forced(s32, oracle_session):
    h, w = 736, 800
    page = _rand_page(h, w, 81)
    assert R.resize_both_plan(h, w) == [] or R.resize_both_plan(h, w)[-1] == (h, w)
    assert tuple(R.resize_either_dims(h, w)) == (h, w)
    s32.set_det_tiles(384, 64)
    keep = (oracle_session.det_worker, oracle_session.cls_worker, oracle_session.rec_worker)
    try:
        plan = retto_amd.det_tile_plan(h, w, 384, 64)
        assert (len(plan["row_origins"]), len(plan["col_origins"])) == (3, 3)
        assert plan["col_origins"][1] + 384 - plan["col_origins"][2] > 64        # the last pair overlaps by more than O
        det_img = R.thumbnail(R.resize_both(page), h, w)                         # the det image the oracle derives
        stitched = s32.debug_det_tiles(det_img)[1]
        oracle_session.det_worker = lambda x: stitched[None, None]
        oracle_session.cls_worker, oracle_session.rec_worker = s32.worker.cls, s32.worker.rec
        got = s32.run_batch([page])[0]
        _assert_page_equal(got, oracle_session.run(page))
        page2, rects = workload.planted_page(h, w, 6, seed=82)
        pmap = workload.planted_map(h, w, h, w, rects)
        got2 = s32.run_batch([page2], det_map_override=[pmap])[0]
        o2 = oracle_session.run(page2, det_map_override=pmap)
        assert len(o2.det_boxes) == 6
        _assert_page_equal(got2, o2)
    finally:
        oracle_session.det_worker, oracle_session.cls_worker, oracle_session.rec_worker = keep
        s32.set_det_tiles(0)


# ---- 5. a mixed call ---------------------------------------------------------------------------------------------------------
MIXED = [(736, 800, 5, 91), (320, 416, 3, 92), (320, 384, 3, 95), (1184, 736, 6, 93), (736, 800, 4, 94)]


def test_mixed_call_equals_every_page_alone():
    planted = [workload.planted_page(h, w, L, seed=sd) for h, w, L, sd in MIXED]
    pages = [p for p, _ in planted]
    maps = [workload.planted_map(h, w, h, w, rects) for (h, w, _, _), (_, rects) in zip(MIXED, planted)]
    raw = [_rand_page(h, w, sd + 100) for h, w, _, sd in MIXED]
    s = _session(lanes=1, det_sub_batch=4, det_limit=320)
    try:
        s.set_det_tiles(384, 64)
        units = 0
        for h, w, _, _ in MIXED:
            p = retto_amd.det_tile_plan(h, w, 384, 64)
            units += len(p["row_origins"]) * len(p["col_origins"])
        assert units == 9 + 2 + 1 + 12 + 9   # groups of 4: the untiled page shares its group with tiles of two pages
        s.profile_enable()
        together = s.run_batch(pages, det_map_override=maps)
        prof = s.profile_get()
        groups = -(-units // 4)                          # det_sub_batch = 4: a page's tiles span several groups
        assert _calls(prof, "net/det") == groups and _calls(prof, "det_tile_cut") == groups and _calls(prof, "det_tile_stitch") == groups
        for i, (p, m) in enumerate(zip(pages, maps)):
            alone = s.run_batch([p], det_map_override=[m])[0]
            assert len(alone.det_result) == MIXED[i][2]
            _same(together[i], alone, same_call=False)
        s.run_batch(raw)
        cs = s.last_det_checksum
        cs_alone = 0.0
        for p in raw:
            s.run_batch([p]); cs_alone += s.last_det_checksum
        print("checksum together %.9g alone %.9g" % (cs, cs_alone))
        assert abs(cs - cs_alone) <= 1e-6 * abs(cs_alone)
    finally:
        s.close()
    s3 = _session(lanes=3, det_limit=320)   # (the default grouping: every lane's units in one mixed group, the last one)
    try:
        s3.set_det_tiles(384, 64)
        hs, ws = [p.shape[0] for p in pages], [p.shape[1] for p in pages]
        lanes3 = s3.wait_batch(s3.submit_batch_raw(pages, hs, ws, det_map_override=maps))
        assert len(lanes3) == len(together)
        for a, b in zip(lanes3, together):
            _same(a, b, same_call=False)
    finally:
        s3.close()


# ---- 6. the setter -----------------------------------------------------------------------------------------------------------
def test_setter_is_guarded_and_a_batch_keeps_its_value():
    s = _session(lanes=2, det_limit=320)
    try:
        pages = [_rand_page(736, 800, 111), _rand_page(736, 800, 112)]
        for bad in ((48, 0), (96, 48), (96, 64), (-32, 0)):
            with pytest.raises(retto_amd.InvalidArgument):
                s.set_det_tiles(*bad)
        assert s.det_tiles == (0, 0)
        ref_off = s.run_batch(pages)
        s.set_det_tiles(384, 64)
        ref_on = s.run_batch(pages)
        s.profile_enable()
        ticket = s.submit_batch_raw(pages, [736, 736], [800, 800])
        with pytest.raises(retto_amd.InvalidArgument) as e:   # refused while the ticket is in flight
            s.set_det_tiles(0)
        assert "in flight" in str(e.value)
        got = s.wait_batch(ticket)
        assert s.det_tiles == (384, 64)
        prof = s.profile_get()
        assert _calls(prof, "det_tile_cut") == 2 and _calls(prof, "det_tile_stitch") == 2   # one group on each lane
        for a, b in zip(got, ref_on):
            _same(a, b)
        # the batch carries the value of its submit: changed right after the wait, the next batch runs without tiles
        s.set_det_tiles(0)
        s.profile_enable()
        got_off = s.wait_batch(s.submit_batch_raw(pages, [736, 736], [800, 800]))
        prof = s.profile_get()
        assert _calls(prof, "det_tile_cut") == 0 and _calls(prof, "det_tile_stitch") == 0
        for a, b in zip(got_off, ref_off):
            _same(a, b)
    finally:
        s.close()


# ---- 7. a large map through DB post-processing -------------------------------------------------------------------------------
def test_large_planted_map_through_db_post(s32):
    H, W = 2048, 4096
    rng = np.random.default_rng(7)
    rects = []
    for gy in range(24):
        for gx in range(10):
            x0 = 40 + gx * 400 + int(rng.integers(0, 60)); y0 = 30 + gy * 84 + int(rng.integers(0, 20))
            rects.append((x0, y0, x0 + int(rng.integers(120, 320)), y0 + int(rng.integers(18, 44))))
    pmap = workload.planted_map(H, W, H, W, rects)
    gb, gs = s32.det_postprocess(pmap, H, W)
    rb, rs = R.det_postprocess(pmap, H, W)
    assert len(rb) > 0.9 * len(rects) and len(gb) == len(rb)
    assert np.array_equal(gb, rb) and np.array_equal(gs.view(np.uint32), rs.view(np.uint32))
