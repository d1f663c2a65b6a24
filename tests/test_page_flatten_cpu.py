"""Page flatten (retto_amd/csrc/page_flatten.h) without a GPU: rt_debug_flatten_page_host, the rule in plain C++ loops over the
header the kernels share, against the numpy reference byte for byte; the division of step 5 over its whole domain; the four
names; and the argument checks that need no device."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import retto_amd
from page_flatten_ref import FLOORS, KINDS, SHAPES, flatten, page
from retto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 8
NAMES = ("rt_set_page_flatten", "rt_page_flatten", "rt_flatten_page", "rt_debug_flatten_page_host")


@functools.lru_cache(maxsize=None)
def case(kind, shape, floor):
    """(page, reference page, reference level) of one case; computed once, shared with tests/test_gpu_page_flatten.py"""
    if floor != FLOORS[0]:   # the level does not depend on the floor
        img, _, level = case(kind, shape, FLOORS[0])
    else:
        img = page(kind, shape[1], shape[2], seed=shape[1] * 1000 + shape[2]); level = None
    ref, level = flatten(img, shape[0], floor, level)
    for a in (img, ref, level):
        a.setflags(write=False)
    return img, ref, level


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_host_rule_equals_numpy_reference(kind, shape, floor):
    img, ref, ref_level = case(kind, shape, floor)
    got, level = retto_amd.debug_flatten_page_host(img, shape[0], floor, with_level=True)
    assert np.array_equal(level, ref_level) and np.array_equal(got, ref)
    assert np.array_equal(retto_amd.debug_flatten_page_host(img, shape[0], floor), ref)   # without the level


def test_division_over_its_whole_domain(tmp_path):
    """every p and L in [64, 16320] through the header: the integer form equals numpy's, the kernel's reciprocal form equals it"""
    exe, table = str(tmp_path / "div_driver"), str(tmp_path / "table.bin")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "retto_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "page_flatten_div_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "the driver does not build:\n" + r.stderr[-3000:]
    r = subprocess.run([exe, table], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr
    p = np.arange(256, dtype=np.int64)[:, None]; L = np.arange(64, 16321, dtype=np.int64)[None, :]
    assert np.array_equal(np.fromfile(table, np.uint8).reshape(256, -1), np.minimum(255, (p * 16320 + L // 2) // L))


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert "RT_API int %s(" % name in header, name
    assert "NOT\n * been measured" in header[header.index("Page flatten"):header.index("rt_set_page_flatten(")]
    assert "flatten" not in header[header.index("typedef struct rt_config"):header.index("} rt_config;")]   # no rt_config field
    for name in ("set_page_flatten", "page_flatten", "flatten_page"):
        assert hasattr(retto_amd.RettoSession, name)


def test_null_and_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.rt_set_page_flatten(None, 4, 64) == INVALID and b"rt_set_page_flatten" in lib.rt_last_error(None)
    assert lib.rt_page_flatten(None, None, None) == INVALID
    img = page("noise", 8, 8); out = np.empty_like(img)
    assert lib.rt_debug_flatten_page_host(None, 8, 8, 4, 64, out.ctypes.data, None) == INVALID
    assert lib.rt_debug_flatten_page_host(img.ctypes.data, 8, 8, 4, 64, None, None) == INVALID
    for radius, floor, what in ((17, 64, "radius"), (-1, 64, "radius"), (4, 0, "floor"), (4, 256, "floor")):
        with pytest.raises(retto_amd.InvalidArgument, match="rt_debug_flatten_page_host: " + what):
            retto_amd.debug_flatten_page_host(img, radius, floor)
    assert np.array_equal(retto_amd.debug_flatten_page_host(img, 0, 999), img)   # radius 0 is off whatever floor is
