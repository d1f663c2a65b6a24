"""Page flatten on the GPU (rt_set_page_flatten, retto_amd/csrc/page_flatten.hip): rt_flatten_page against the numpy reference
byte for byte (the rule is integer: no tolerance), and the pipeline with flatten on against the pipeline with flatten off on the
flattened pages, bit for bit -- alone, and in front of page enhance."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import retto_amd
from oracle import ref_lib as R
from page_flatten_ref import FLOORS, KINDS, SHAPES
from retto_amd import workload
from test_gpu_page_enhance import same_results
from test_page_flatten_cpu import case

pytestmark = pytest.mark.gpu
RADIUS, FLOOR, TILE, CLIP = 3, 64, 32, 2.5


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_flatten_page_equals_numpy_reference(hip_session, kind, shape, floor):
    img, ref, _ = case(kind, shape, floor)
    assert np.array_equal(hip_session.flatten_page(img, shape[0], floor), ref)


@pytest.fixture(scope="module")
def planted():
    """three planted pages of different sizes and odd widths under an illumination ramp, their det maps and line quads"""
    pages, maps, quads = [], [], []
    for i, (h, w) in enumerate(((224, 320), (203, 291), (97, 333))):
        page, rects = workload.planted_page(h, w, 3, seed=80 + i)
        ramp = (255 - (150 * np.arange(w)) // (w - 1))[None, :, None]
        page = (page.astype(np.int64) * ramp // 255).astype(np.uint8)   # a shadowed page: flattening changes it
        dh, dw = R.resize_either_dims(h, w)
        pages.append(page); maps.append(workload.planted_map(dh, dw, h, w, rects))
        quads.append(np.array([[x0, y0, x1, y0, x1, y1, x0, y1] for x0, y0, x1, y1 in rects], np.float32))
    return pages, maps, quads


@pytest.fixture
def flattening(hip_session):
    hip_session.set_page_flatten(RADIUS, FLOOR)
    assert hip_session.page_flatten() == (RADIUS, FLOOR)
    yield hip_session
    hip_session.set_page_flatten(0, 0); hip_session.set_page_enhance(0, 0.0)


def png(p):
    b = io.BytesIO(); Image.fromarray(p).save(b, "PNG"); return b.getvalue()


def test_pipeline_reads_the_flattened_pages(flattening, planted):
    """pages of different sizes in one call, then regions and encoded pages: read as their single flattenings; reset = fresh"""
    s, (pages, maps, quads) = flattening, planted
    on = s.run_batch(pages, det_map_override=maps)
    assert all(len(r.det_result) == 3 for r in on)
    on_regions = s.run_regions(pages, quads)
    on_encoded = s.run_encoded_batch([png(p) for p in pages])
    single = [s.flatten_page(p, RADIUS, FLOOR) for p in pages]
    assert all(not np.array_equal(a, b) for a, b in zip(single, pages))
    s.set_page_flatten(0, 0)
    assert s.page_flatten() == (0, 0)
    same_results(on, s.run_batch(single, det_map_override=maps))
    same_results(on_regions, s.run_regions(single, quads))
    same_results(on_encoded, s.run_encoded_batch([png(p) for p in single]))
    fresh = retto_amd.RettoSession(retto_amd.synthetic_session_config(0))
    try:
        same_results(s.run_batch(pages, det_map_override=maps), fresh.run_batch(pages, det_map_override=maps))
    finally:
        fresh.close()


def test_flatten_comes_before_enhance(flattening, planted):
    s, (pages, maps, _) = flattening, planted
    s.set_page_enhance(TILE, CLIP)
    both = s.run_batch(pages, det_map_override=maps)
    single = [s.enhance_page(s.flatten_page(p, RADIUS, FLOOR), TILE, CLIP) for p in pages]
    s.set_page_flatten(0, 0); s.set_page_enhance(0, 0.0)
    same_results(both, s.run_batch(single, det_map_override=maps))


def test_device_page_is_not_written(flattening, planted):
    s, (pages, maps, _) = flattening, planted
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
    for radius, floor in ((17, 64), (-1, 64), (4, 0), (4, 256)):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_set_page_flatten: "):
            hip_session.set_page_flatten(radius, floor)
    assert hip_session.page_flatten() == (0, 0)
