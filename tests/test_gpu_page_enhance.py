"""Page enhance on the GPU (rt_set_page_enhance, retto_amd/csrc/page_enhance.hip): rt_enhance_page against the numpy reference
byte for byte (the rule is integer: no tolerance), and the pipeline with enhance on against the pipeline with enhance off on the
enhanced pages, bit for bit."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import retto_amd
from oracle import ref_lib as R
from page_enhance_ref import CLIPS, KINDS, SHAPES
from retto_amd import workload
from test_page_enhance_cpu import case

pytestmark = pytest.mark.gpu
TILE, CLIP = 32, 2.5


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "t%d_%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_enhance_page_equals_numpy_reference(hip_session, kind, shape, clip):
    img, ref, _ = case(kind, shape, clip)
    assert np.array_equal(hip_session.enhance_page(img, shape[0], clip), ref)


def same_results(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert len(g.det_result) == len(r.det_result)
        for a, b in zip(g.det_result, r.det_result):
            assert np.array_equal(a.boxes.as_array(), b.boxes.as_array()) and a.score == b.score
        assert [(c.label.label, c.label.score) for c in g.cls_result] == [(c.label.label, c.label.score) for c in r.cls_result]
        for a, b in zip(g.rec_result, r.rec_result):
            assert np.array_equal(a.tokens, b.tokens) and a.score == b.score


@pytest.fixture(scope="module")
def planted():
    """three planted pages of different sizes (odd widths: rows off the dword grid), their det maps and line quads"""
    pages, maps, quads = [], [], []
    for i, (h, w) in enumerate(((224, 320), (203, 291), (97, 333))):
        page, rects = workload.planted_page(h, w, 3, seed=70 + i)
        page = (page // 3 + 60).astype(np.uint8)   # a faded page: the enhancement changes it
        dh, dw = R.resize_either_dims(h, w)
        pages.append(page); maps.append(workload.planted_map(dh, dw, h, w, rects))
        quads.append(np.array([[x0, y0, x1, y0, x1, y1, x0, y1] for x0, y0, x1, y1 in rects], np.float32))
    return pages, maps, quads


@pytest.fixture
def enhancing(hip_session):
    hip_session.set_page_enhance(TILE, CLIP)
    assert hip_session.page_enhance() == (TILE, CLIP)
    yield hip_session
    hip_session.set_page_enhance(0, 0.0)


def test_pipeline_reads_the_enhanced_pages(enhancing, planted):
    """several pages of different sizes in one call (one flat list of tiles, one of cells): each is read as its single-page
    enhancement is; then the same through rt_run_regions and the encoded entry point; reset to 0 equals a fresh session"""
    s, (pages, maps, quads) = enhancing, planted
    on = s.run_batch(pages, det_map_override=maps)
    assert all(len(r.det_result) == 3 for r in on)
    on_regions = s.run_regions(pages, quads)
    pngs = []
    for p in pages:
        b = io.BytesIO(); Image.fromarray(p).save(b, "PNG"); pngs.append(b.getvalue())
    on_encoded = s.run_encoded_batch(pngs)
    single = [s.enhance_page(p, TILE, CLIP) for p in pages]
    assert all(not np.array_equal(a, b) for a, b in zip(single, pages))
    s.set_page_enhance(0, 0.0)
    assert s.page_enhance() == (0, 0.0)
    same_results(on, s.run_batch(single, det_map_override=maps))
    same_results(on_regions, s.run_regions(single, quads))
    enc_single = []
    for p in single:
        b = io.BytesIO(); Image.fromarray(p).save(b, "PNG"); enc_single.append(b.getvalue())
    same_results(on_encoded, s.run_encoded_batch(enc_single))
    fresh = retto_amd.RettoSession(retto_amd.synthetic_session_config(0))
    try:
        same_results(s.run_batch(pages, det_map_override=maps), fresh.run_batch(pages, det_map_override=maps))
    finally:
        fresh.close()


def test_device_page_is_not_written(enhancing, planted):
    s, (pages, maps, _) = enhancing, planted
    lib, h = s._hd.lib, s._hd.h
    page = pages[1]; d = C.c_void_p()
    assert lib.rt_device_malloc(h, page.nbytes, C.byref(d)) == 0
    try:
        assert lib.rt_memcpy_h2d(h, d, page.ctypes.data, page.nbytes) == 0
        r = s.run_batch_raw([d.value], [page.shape[0]], [page.shape[1]], retto_amd.RT_MEM_DEVICE)
        got = s._collect(r, 0); lib.rt_results_free(r)
        back = np.empty_like(page)
        assert lib.rt_memcpy_d2h(h, back.ctypes.data, d, page.nbytes) == 0
        assert np.array_equal(back, page)
        same_results([got], s.run_batch([page]))   # and the device page was read as the host page is
    finally:
        lib.rt_device_free(h, d)


def test_setter_refuses_bad_parameters(hip_session):
    for tile, clip in ((16, 2.5), (48, 2.5), (544, 2.5), (64, 0.5), (64, 65.0), (64, float("nan")), (64, float("inf"))):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_set_page_enhance: "):
            hip_session.set_page_enhance(tile, clip)
    assert hip_session.page_enhance() == (0, 0.0)
