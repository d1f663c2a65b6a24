"""Page deskew on the GPU (rt_set_page_deskew, retto_amd/csrc/page_deskew.hip): rt_deskew_page against the numpy reference byte for
byte in image and slope (the rule is integer: no tolerance), and the pipeline with deskew on against the pipeline with deskew off
on the deskewed pages, bit for bit -- alone, behind flatten and enhance, and never in a regions call."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import page_deskew_ref as ref
import retto_amd
from oracle import ref_lib as R
from page_deskew_ref import GAINS, KINDS, RANGES, SHAPES
from retto_amd import workload
from test_gpu_page_enhance import same_results
from test_page_deskew_cpu import case, shape_id

pytestmark = pytest.mark.gpu
RANGE, GAIN, RADIUS, FLOOR, TILE, CLIP = 64, 25, 3, 64, 32, 2.5


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("K", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
def test_deskew_page_equals_numpy_reference(hip_session, kind, shape, K, gain):
    img, want, want_slope, _ = case(kind, shape, K, gain)
    got, slope = hip_session.deskew_page(img, K, gain)
    assert slope == want_slope and np.array_equal(got, want)


@pytest.fixture(scope="module")
def planted():
    """three slanted text pages of different sizes and odd widths, det maps and line quads of planted rectangles on them"""
    pages, maps, quads = [], [], []
    for i, (h, w, slope) in enumerate(((224, 320, 60), (203, 291, -60), (97, 333, 45))):
        _, rects = workload.planted_page(h, w, 3, seed=90 + i)
        dh, dw = R.resize_either_dims(h, w)
        pages.append(ref.page(slope, h, w, seed=i)); maps.append(workload.planted_map(dh, dw, h, w, rects))
        quads.append(np.array([[x0, y0, x1, y0, x1, y1, x0, y1] for x0, y0, x1, y1 in rects], np.float32))
    return pages, maps, quads


@pytest.fixture
def deskewing(hip_session):
    hip_session.set_page_deskew(RANGE, GAIN)
    assert hip_session.page_deskew() == (RANGE, GAIN)
    yield hip_session
    hip_session.set_page_deskew(0, 0); hip_session.set_page_flatten(0, 0); hip_session.set_page_enhance(0, 0.0)


def png(p):
    b = io.BytesIO(); Image.fromarray(p).save(b, "PNG"); return b.getvalue()


def test_pipeline_reads_the_deskewed_pages(deskewing, planted):
    """pages of different sizes in one call, then encoded pages: read as their single deskewings, with the reference's slope and
    matrix per page; regions are read as with deskew off; reset = fresh"""
    s, (pages, maps, quads) = deskewing, planted
    on = s.run_batch(pages, det_map_override=maps)
    assert all(len(r.det_result) == 3 for r in on)
    on_encoded = s.run_encoded_batch([png(p) for p in pages])
    on_regions = s.run_regions(pages, quads)
    single = [s.deskew_page(p, RANGE, GAIN)[0] for p in pages]
    for p, got in zip(pages + pages, on + on_encoded):
        k = ref.deskew(p, RANGE, GAIN)[1]
        assert k != 0 and got.deskew.slope == k
        assert np.array_equal(got.deskew.matrix.ravel(), ref.matrix(k, p.shape[0], p.shape[1]))
    s.set_page_deskew(0, 0)
    assert s.page_deskew() == (0, 0)
    same_results(on, s.run_batch(single, det_map_override=maps))
    same_results(on_encoded, s.run_encoded_batch([png(p) for p in single]))
    off_regions = s.run_regions(pages, quads)
    same_results(on_regions, off_regions)
    for got in on_regions + off_regions:
        assert got.deskew.slope == 0 and np.array_equal(got.deskew.matrix, np.eye(2, 3, dtype=np.float32))
    fresh = retto_amd.RettoSession(retto_amd.synthetic_session_config(0))
    try:
        same_results(s.run_batch(pages, det_map_override=maps), fresh.run_batch(pages, det_map_override=maps))
    finally:
        fresh.close()


def test_deskew_comes_after_flatten_and_enhance(deskewing, planted):
    s, (pages, maps, _) = deskewing, planted
    s.set_page_flatten(RADIUS, FLOOR); s.set_page_enhance(TILE, CLIP)
    all_on = s.run_batch(pages, det_map_override=maps)
    single = [s.deskew_page(s.enhance_page(s.flatten_page(p, RADIUS, FLOOR), TILE, CLIP), RANGE, GAIN)[0] for p in pages]
    s.set_page_deskew(0, 0); s.set_page_flatten(0, 0); s.set_page_enhance(0, 0.0)
    same_results(all_on, s.run_batch(single, det_map_override=maps))


def test_device_page_is_not_written(deskewing, planted):
    s, (pages, maps, _) = deskewing, planted
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
    for K, gain in ((129, 25), (-1, 25), (16, -1), (16, 10001)):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_set_page_deskew: "):
            hip_session.set_page_deskew(K, gain)
    assert hip_session.page_deskew() == (0, 0)
