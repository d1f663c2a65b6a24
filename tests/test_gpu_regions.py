"""rt_run_regions on the GPU: the pipeline from the crop plan on, over quads the caller supplies.  Comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import retto_amd
from retto_amd import RT_MEM_DEVICE

import crop_source_cases as CS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session():
    """Original mode with max_side_len = 512 (the 620 x 1000 page is shrunk for the detector), word boxes and candidates on."""
    cfg = retto_amd.synthetic_session_config(0, crop_source="Original", max_side_len=CS.SMALL_LIMIT, lanes=3)
    cfg.rec_processor_config.return_word_box = True
    cfg.rec_processor_config.return_candidates = 3
    s = retto_amd.RettoSession(cfg)
    yield s
    s.close()


@pytest.fixture(scope="module")
def page_and_boxes(session):
    page, m = CS.page_with_tall_line()
    r = session.run_batch([page], det_map_override=[m])[0]
    B = np.stack([d.boxes.as_array() for d in r.det_result])
    assert len(B) == 6
    return page, B, r


def _boxes(r):
    return np.stack([d.boxes.as_array() for d in r.det_result]) if r.det_result else np.zeros((0, 4, 2), np.float32)


def test_regions_equal_the_pipeline_on_its_own_boxes(session, page_and_boxes):
    page, B, ref = page_and_boxes
    r = session.run_regions([page], [B])[0]
    assert np.array_equal(_boxes(r).view(np.uint32), B.view(np.uint32))
    assert [d.score for d in r.det_result] == [1.0] * len(B)
    assert session.last_det_checksum == 0.0
    assert all(g.words is not None and g.candidates is not None for g in r.rec_result)
    assert CS.digest(r, boxes=False) == CS.digest(ref, boxes=False)


def test_permuting_the_quads_permutes_the_results(session, page_and_boxes):
    page, B, _ = page_and_boxes
    perm = [3, 0, 5, 1, 4, 2]
    a = session.run_regions([page], [B])[0]
    b = session.run_regions([page], [B[perm]])[0]
    assert np.array_equal(_boxes(b), B[perm])
    da, db = CS.digest(a), CS.digest(b)
    for key in da:
        assert db[key] == [da[key][k] for k in perm], key


def test_pages_without_quads(session, page_and_boxes):
    page, B, _ = page_and_boxes
    empty = np.zeros((0, 4, 2), np.float32)
    r = session.run_regions([page], [empty])
    assert len(r) == 1 and r[0].det_result == [] and r[0].cls_result == [] and r[0].rec_result == []
    full = session.run_regions([page], [B])[0]
    r = session.run_regions([page, page, page, page], [B, empty, B[:2], []])
    assert [len(x.rec_result) for x in r] == [6, 0, 2, 0]
    a, b = CS.digest(r[0]), CS.digest(full)
    assert a == b, CS.differing(a, b)
    # two of the six quads: each line's results are those it has among all six
    a = CS.digest(r[2])
    assert a == {k: v[:2] for k, v in b.items()}, CS.differing(a, {k: v[:2] for k, v in b.items()})
    assert session.run_regions([], []) == []


def test_quads_are_clamped_to_the_page(session, page_and_boxes):
    page, B, _ = page_and_boxes
    h, w = page.shape[:2]
    poking = np.array([[[-30.5, -4.25], [400.5, -8.0], [400.5, 38.5], [-30.5, 41.0]],
                       [[700.25, 580.5], [1200.0, 580.5], [1200.0, 700.0], [700.25, 700.0]]], np.float32)
    clamped = poking.copy()
    clamped[..., 0] = np.clip(clamped[..., 0], np.float32(0), np.float32(w - 1))
    clamped[..., 1] = np.clip(clamped[..., 1], np.float32(0), np.float32(h - 1))
    assert clamped[0, 3, 1] == 41.0 and clamped[1, 0, 0] == 700.25   # no rounding
    a = session.run_regions([page], [poking])[0]
    b = session.run_regions([page], [clamped])[0]
    assert np.array_equal(_boxes(a).view(np.uint32), clamped.view(np.uint32))
    assert CS.digest(a) == CS.digest(b)


@pytest.mark.parametrize("kind", ["nan", "inf", "point"])
def test_bad_quads_are_rejected_and_the_session_lives_on(session, page_and_boxes, kind):
    page, B, ref = page_and_boxes
    bad = B.copy()
    if kind == "nan":
        bad[4, 2, 1] = np.nan
    elif kind == "inf":
        bad[4, 0, 0] = np.inf
    else:
        bad[4] = np.float32(123.5)   # all four corners equal
    with pytest.raises(retto_amd.InvalidArgument, match=r"page 1 region 4"):
        session.run_regions([page, page], [B, bad])
    r = session.run_regions([page], [B])[0]
    assert CS.digest(r, boxes=False) == CS.digest(ref, boxes=False)


def test_bad_counts_and_null_quads_are_rejected(session, page_and_boxes):
    page, B, _ = page_and_boxes
    lib, h = session._hd.lib, session._hd.h
    p = np.ascontiguousarray(page)
    pages = (C.c_void_p * 1)(p.ctypes.data); hs = (C.c_int * 1)(p.shape[0]); ws = (C.c_int * 1)(p.shape[1])
    q = np.ascontiguousarray(B.reshape(-1, 8))
    out = C.c_void_p()
    for quads, n, what in (((C.c_void_p * 1)(q.ctypes.data), -1, b"negative"), ((C.c_void_p * 1)(None), 2, b"NULL")):
        assert lib.rt_run_regions(h, pages, hs, ws, 1, 0, quads, (C.c_int * 1)(n), C.byref(out)) == 8 and not out.value
        msg = lib.rt_last_error(h)
        assert b"page 0" in msg and what in msg
    assert lib.rt_run_regions(h, pages, hs, ws, 1, 2, (C.c_void_p * 1)(q.ctypes.data), (C.c_int * 1)(6), C.byref(out)) == 8   # RT_MEM_HOST_MAPS_DEVICE
    assert len(session.run_regions([page], [B])[0].rec_result) == 6


def test_null_output_with_a_live_session(session, page_and_boxes):
    page, B, _ = page_and_boxes
    lib, h = session._hd.lib, session._hd.h
    p = np.ascontiguousarray(page)
    pages = (C.c_void_p * 1)(p.ctypes.data); hs = (C.c_int * 1)(p.shape[0]); ws = (C.c_int * 1)(p.shape[1])
    q = np.ascontiguousarray(B.reshape(-1, 8))
    assert lib.rt_run_regions(h, pages, hs, ws, 1, 0, (C.c_void_p * 1)(q.ctypes.data), (C.c_int * 1)(6), None) == 8
    assert lib.rt_debug_warp_crops(h, p.ctypes.data, p.shape[0], p.shape[1], q.ctypes.data, 6, 1, None, 0) == 8
    assert b"rt_debug_warp_crops" in lib.rt_last_error(h)
    assert len(session.run_regions([page], [B])[0].rec_result) == 6


def test_no_detector_runs(session, page_and_boxes):
    page, B, _ = page_and_boxes
    session.profile_enable(True)
    try:
        session.run_batch([page])
        assert session.profile_get()["net/det"][1] > 0
        session.profile_enable(True)   # (zeroes the totals; the names stay)
        session.run_regions([page], [B])
        prof = {k for k, (_ms, calls) in session.profile_get().items() if calls > 0}   # the scopes this call recorded
    finally:
        session.profile_enable(False)
    assert "net/det" not in prof and "db_postprocess" not in prof and "thumbnail" not in prof
    assert "warp_crops" in prof and "net/cls" in prof and "net/rec" in prof
    assert session.last_det_checksum == 0.0


def test_device_pages_equal_host_pages(session, page_and_boxes):
    page, B, _ = page_and_boxes
    lib, h = session._hd.lib, session._hd.h
    host = session.run_regions([page, page], [B, B[::-1].copy()])
    d = C.c_void_p()
    assert lib.rt_device_malloc(h, page.nbytes, C.byref(d)) == 0
    try:
        assert lib.rt_memcpy_h2d(h, d, np.ascontiguousarray(page).ctypes.data, page.nbytes) == 0
        r = session.run_regions_raw([d.value, d.value], [page.shape[0]] * 2, [page.shape[1]] * 2, [B, B[::-1].copy()], RT_MEM_DEVICE)
        try:
            dev = [session._collect(r, i) for i in range(2)]
        finally:
            lib.rt_results_free(r)
    finally:
        lib.rt_device_free(h, d)
    assert [CS.digest(a) for a in dev] == [CS.digest(b) for b in host]
