"""Page derule on the GPU (rt_set_page_derule, retto_amd/csrc/page_derule.hip): rt_derule_page against the numpy reference byte for
byte (the rule is integer: no tolerance), and the pipeline with derule on against the pipeline with derule off on the deruled
pages, bit for bit."""
import numpy as np
import pytest

import retto_amd
from oracle import ref_lib as R
from page_derule_ref import derule
from retto_amd import workload
from test_gpu_page_enhance import same_results
from test_page_derule_cpu import CASES, case, case_id

pytestmark = pytest.mark.gpu
SETTING = (32, 4, 96)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_derule_page_equals_numpy_reference(hip_session, c):
    img, ref = case(*c)
    assert np.array_equal(hip_session.derule_page(img, *c[0]), ref)


@pytest.fixture(scope="module")
def ruled():
    """two planted pages of different sizes (one of odd width) with a grid of 2-pixel rules over them, and their det maps"""
    pages, maps = [], []
    for i, (h, w) in enumerate(((224, 320), (203, 291))):
        page, rects = workload.planted_page(h, w, 3, seed=110 + i)
        page = page.copy()
        page[20::45][:, 6:w - 6] = 10; page[21::45][:, 6:w - 6] = 10
        page[8:h - 8, 30::70] = 10; page[8:h - 8, 31::70] = 10
        dh, dw = R.resize_either_dims(h, w)
        pages.append(page); maps.append(workload.planted_map(dh, dw, h, w, rects))
    return pages, maps


def test_pipeline_reads_the_deruled_pages(hip_session, ruled):
    s, (pages, maps) = hip_session, ruled
    off = s.run_batch(pages, det_map_override=maps)
    s.set_page_derule(*SETTING)
    try:
        assert s.page_derule() == SETTING
        on = s.run_batch(pages, det_map_override=maps)
    finally:
        s.set_page_derule(0, 0, 0)
    assert s.page_derule() == (0, 0, 0)
    single = [s.derule_page(p, *SETTING) for p in pages]
    for p, d in zip(pages, single):
        assert np.array_equal(d, derule(p, *SETTING)) and not np.array_equal(d, p)
    same_results(on, s.run_batch(single, det_map_override=maps))
    same_results(off, s.run_batch(pages, det_map_override=maps))   # off again: the build's ordinary result


def test_setter_refuses_bad_parameters(hip_session):
    for L, T, I in ((15, 4, 96), (513, 4, 96), (32, 9, 96), (32, 4, 0)):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_set_page_derule: "):
            hip_session.set_page_derule(L, T, I)
    assert hip_session.page_derule() == (0, 0, 0)
