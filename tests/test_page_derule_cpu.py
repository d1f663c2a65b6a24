"""Page derule (retto_amd/csrc/page_derule.h) without a GPU: what the numpy reference does to the planted pages;
rt_debug_derule_page_host, the rule in plain C++ loops over the header the kernels share, equals it byte for byte; the names; and
the argument checks that need no device."""
import functools
import os

import numpy as np
import pytest

import retto_amd
from page_derule_ref import SETTINGS, derule, luma, page, shapes
from retto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 8
NAMES = ("rt_set_page_derule", "rt_page_derule", "rt_derule_page", "rt_debug_derule_page_host")
CASES = [(s, k) for s in SETTINGS for k in range(len(shapes(s[0], s[1])))]
case_id = lambda c: "L%d-T%d-I%d-%dx%d" % (c[0] + shapes(c[0][0], c[0][1])[c[1]])


@functools.lru_cache(maxsize=None)
def case(setting, k):
    """(page, reference page) of one case; computed once, shared with tests/test_gpu_page_derule.py"""
    L, T, I = setting
    h, w = shapes(L, T)[k]
    img, _ = page(h, w, L, T, seed=1000 * h + w)
    ref = derule(img, L, T, I)
    for a in (img, ref):
        a.setflags(write=False)
    return img, ref


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_host_rule_equals_numpy_reference(c):
    img, ref = case(*c)
    L = c[0][0]
    assert np.array_equal(retto_amd.debug_derule_page_host(img, *c[0]), ref)
    if max(img.shape[:2]) < L:
        assert np.array_equal(ref, img)        # no run can be long: nothing may change
    else:
        assert not np.array_equal(ref, img)    # the case is about something


@pytest.mark.parametrize("setting", SETTINGS[:3])
def test_reference_erases_a_grid_and_keeps_crossing_strokes(setting):
    L, T, I = setting
    img, grid = page(120, 150, L, 2, "grid")
    out = derule(img, L, 2, I)
    assert not (255 - luma(out) >= I)[grid].any()
    img, strokes = page(60, 150, L, T, "cross")
    out = derule(img, L, T, I)
    assert np.array_equal(out[strokes], img[strokes]) and not np.array_equal(out, img)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert "RT_API int %s(" % name in header, name
    assert "derule" not in header[header.index("typedef struct rt_config"):header.index("} rt_config;")]   # no rt_config field
    for name in ("set_page_derule", "page_derule", "derule_page"):
        assert hasattr(retto_amd.RettoSession, name)


def test_null_and_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.rt_set_page_derule(None, 16, 1, 96) == INVALID and b"rt_set_page_derule" in lib.rt_last_error(None)
    assert lib.rt_page_derule(None, None, None, None) == INVALID
    img, _ = page(8, 8, 16, 1); out = np.empty_like(img)
    assert lib.rt_debug_derule_page_host(None, 8, 8, 16, 1, 96, out.ctypes.data) == INVALID
    assert lib.rt_debug_derule_page_host(img.ctypes.data, 8, 8, 16, 1, 96, None) == INVALID
    for L, T, I, what in ((15, 1, 96, "min_len"), (513, 1, 96, "min_len"), (-1, 1, 96, "min_len"), (16, 0, 96, "max_thick"),
                          (16, 9, 96, "max_thick"), (16, 1, 0, "ink"), (16, 1, 256, "ink")):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_debug_derule_page_host: " + what):
            retto_amd.debug_derule_page_host(img, L, T, I)
    assert np.array_equal(retto_amd.debug_derule_page_host(img, 0, -5, 999), img)   # min_len 0 is off whatever the others are
