"""Page enhance (retto_amd/csrc/page_enhance.h) without a GPU: rt_debug_enhance_page_host, the rule in plain C++ loops over the
header the kernels share, against the numpy reference byte for byte, and the parameter checks every entry point shares."""
import functools

import numpy as np
import pytest

import retto_amd
from page_enhance_ref import CLIPS, KINDS, SHAPES, enhance, page


@functools.lru_cache(maxsize=None)
def case(kind, shape, clip):
    """(page, reference page, reference LUTs) of one case; computed once, shared with tests/test_gpu_page_enhance.py"""
    tile, h, w = shape
    img = page(kind, h, w, seed=h * 1000 + w)
    ref, luts = enhance(img, tile, clip)
    for a in (img, ref, luts):
        a.setflags(write=False)
    return img, ref, luts


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "t%d_%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_host_rule_equals_numpy_reference(kind, shape, clip):
    img, ref, ref_luts = case(kind, shape, clip)
    got, luts = retto_amd.debug_enhance_page_host(img, shape[0], clip, with_luts=True)
    assert np.array_equal(luts, ref_luts)
    assert np.array_equal(got, ref)
    assert np.array_equal(retto_amd.debug_enhance_page_host(img, shape[0], clip), ref)   # without the LUTs
    if kind in ("gradient", "white", "text"):   # a grey page stays grey
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])


@pytest.mark.parametrize("tile,clip,what", [(16, 2.5, "tile"), (48, 2.5, "tile"), (544, 2.5, "tile"), (64, 0.5, "clip"), (64, 65.0, "clip"),
                                            (64, float("nan"), "clip"), (64, float("inf"), "clip")])
def test_bad_parameters_are_refused_by_name(tile, clip, what):
    img = page("noise", 40, 40)
    with pytest.raises(retto_amd.InvalidArgument, match="rt_debug_enhance_page_host: " + what):
        retto_amd.debug_enhance_page_host(img, tile, clip)


def test_tile_zero_is_off():
    """the check all entry points share takes tile 0 as "off" whatever clip is: the page comes back as it is"""
    img = page("noise", 40, 40)
    for clip in (2.5, 0.0, float("nan")):
        assert np.array_equal(retto_amd.debug_enhance_page_host(img, 0, clip), img)
