"""Page deskew (retto_amd/csrc/page_deskew.h) without a GPU: the numpy reference finds the planted slopes; rt_debug_deskew_page_host,
the rule in plain C++ loops over the header the kernels share, equals it byte for byte; the angle table; the names; and the
argument checks that need no device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import retto_amd
from page_deskew_ref import GAINS, KINDS, RANGES, SHAPES, angle, deskew, ink_grid, page
from retto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 8
NAMES = ("rt_set_page_deskew", "rt_page_deskew", "rt_deskew_page", "rt_debug_deskew_page_host", "rt_results_page_deskew")
shape_id = lambda s: "%dx%d" % s


@functools.lru_cache(maxsize=None)
def case(kind, shape, K, gain):
    """(page, reference page, reference slope, reference scores) of one case; computed once, shared with
    tests/test_gpu_page_deskew.py"""
    if gain != GAINS[0]:   # the scores do not depend on the gate
        img, _, _, S = case(kind, shape, K, GAINS[0])
    else:
        img = page(kind, shape[0], shape[1], seed=shape[0] * 1000 + shape[1]); S = None
    ref, slope, S = deskew(img, K, gain, S)
    for a in (img, ref):
        a.setflags(write=False)
    return img, ref, slope, S


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("K", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
def test_reference_finds_the_planted_slope(kind, shape, K, gain):
    """within one step wherever the slope moves the outermost grid column by at least two cells (and lies inside the range); 0 on
    the uniform and the noise page"""
    img, _, slope, _ = case(kind, shape, K, gain)
    if isinstance(kind, str):
        assert slope == 0
    elif abs(kind) <= K and abs(kind) * (ink_grid(img).shape[1] // 2) / 512 >= 2:
        assert abs(slope - kind) <= 1, slope


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("K", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
def test_host_rule_equals_numpy_reference(kind, shape, K, gain):
    img, ref, ref_slope, S = case(kind, shape, K, gain)
    got, slope, scores = retto_amd.debug_deskew_page_host(img, K, gain, with_scores=True)
    assert slope == ref_slope and [int(s) for s in scores] == S and np.array_equal(got, ref)
    got, slope = retto_amd.debug_deskew_page_host(img, K, gain)   # without the scores
    assert slope == ref_slope and np.array_equal(got, ref)


def test_angle_table_is_a_rotation():
    for a in range(129):
        cosq, sinq = angle(a)
        assert abs(cosq * cosq + sinq * sinq - (1 << 32)) <= 1 << 18, a
        assert angle(-a) == (cosq, -sinq)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert "RT_API int %s(" % name in header, name
    assert "deskew" not in header[header.index("typedef struct rt_config"):header.index("} rt_config;")]   # no rt_config field
    for name in ("set_page_deskew", "page_deskew", "deskew_page"):
        assert hasattr(retto_amd.RettoSession, name)


def test_null_and_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.rt_set_page_deskew(None, 16, 25) == INVALID and b"rt_set_page_deskew" in lib.rt_last_error(None)
    assert lib.rt_page_deskew(None, None, None) == INVALID
    slope = C.c_int(7); m = (C.c_float * 6)()
    assert lib.rt_results_page_deskew(None, 0, C.byref(slope), m) == INVALID and slope.value == 0 and list(m) == [1, 0, 0, 0, 1, 0]
    img = page("noise", 8, 8); out = np.empty_like(img)
    assert lib.rt_debug_deskew_page_host(None, 8, 8, 16, 25, out.ctypes.data, None, None) == INVALID
    assert lib.rt_debug_deskew_page_host(img.ctypes.data, 8, 8, 16, 25, None, None, None) == INVALID
    for K, gain, what in ((129, 25, "range"), (-1, 25, "range"), (16, -1, "min_gain"), (16, 10001, "min_gain")):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_debug_deskew_page_host: " + what):
            retto_amd.debug_deskew_page_host(img, K, gain)
    got, slope = retto_amd.debug_deskew_page_host(img, 0, -5)   # range 0 is off whatever min_gain is
    assert slope == 0 and np.array_equal(got, img)
