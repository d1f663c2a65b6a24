"""rt_config.crop_source, rt_run_regions and rt_debug_warp_crops: the parts that need no GPU -- the config field and its place in
the struct, the argument checks that run before any device is touched, the exported symbols, the Python mirror and the CLI
switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 8


def _default_config():
    c = _lib.Config()
    _lib.load().rt_config_default(C.byref(c))
    return c


# ---------------------------------------------------------------- config
def test_crop_source_defaults_to_resized():
    assert _default_config().crop_source == 0
    assert retto_amd.RettoSessionConfig().crop_source == "Resized"
    assert cli.build_parser().parse_args(["-i", "x"]).crop_source == "Resized"
    assert cli.build_parser().parse_args(["-i", "x", "--crop-source", "Original"]).crop_source == "Original"


def test_crop_source_sits_directly_before_rec_return_word_box():
    names = [f[0] for f in _lib.Config._fields_]
    assert names[-3:] == ["rec_return_candidates", "crop_source", "rec_return_word_box"]
    assert _lib.Config.crop_source.offset + 4 == _lib.Config.rec_return_word_box.offset
    assert _lib.Config.crop_source.size == 4


def test_struct_size_matches_the_mirror():
    assert _default_config().struct_size == C.sizeof(_lib.Config)


def test_header_declares_the_field_in_the_same_place():
    src = open(os.path.join(ROOT, "include", "retto_hip.h"), encoding="utf-8").read()
    body = src[src.index("typedef struct rt_config {"):src.index("} rt_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[\d+\])?\s*;", body)
    assert fields[-3:] == ["rec_return_candidates", "crop_source", "rec_return_word_box"]


@pytest.mark.parametrize("bad", [2, -1, 255])
def test_rt_create_rejects_an_unknown_crop_source(bad):
    """Checked before the device probe: RT_ERR_INVALID on any machine."""
    lib = _lib.load()
    c = _default_config(); c.crop_source = bad
    out = C.c_void_p()
    assert lib.rt_create(C.byref(c), C.byref(out)) == INVALID and not out.value
    assert b"crop_source" in lib.rt_last_error(None)


# ---------------------------------------------------------------- symbols and arguments
def test_new_entry_points_are_exported_and_declared():
    lib = _lib.load()
    for name in ("rt_run_regions", "rt_debug_warp_crops"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "retto_hip.h"), encoding="utf-8").read()
    assert "RT_API int rt_run_regions(" in hdr and "RT_API int rt_debug_warp_crops(" in hdr


def test_run_regions_rejects_a_null_session():
    """(a NULL output with a live session needs a device: tests/test_gpu_regions.py)"""
    lib = _lib.load()
    out = C.c_void_p()
    assert lib.rt_run_regions(None, None, None, None, 0, 0, None, None, C.byref(out)) == INVALID
    assert lib.rt_run_regions(None, None, None, None, 0, 0, None, None, None) == INVALID


def test_debug_warp_crops_rejects_a_null_session():
    lib = _lib.load()
    page = np.zeros((8, 8, 3), np.uint8); box = np.zeros(8, np.float32); out = np.zeros(16, np.uint8)
    assert lib.rt_debug_warp_crops(None, page.ctypes.data, 8, 8, box.ctypes.data, 1, 1, out.ctypes.data, 16) == INVALID
    assert lib.rt_debug_warp_crops(None, page.ctypes.data, 8, 8, box.ctypes.data, 1, 1, None, 0) == INVALID


# ---------------------------------------------------------------- Python mirror
@pytest.mark.parametrize("bad", ["original ", "original", "ORIGINAL", "", 1, None])
def test_bad_crop_source_string_raises_invalid_argument(bad):
    """Validated in Python before rt_create (so no device is needed to see it)."""
    cfg = retto_amd.synthetic_session_config(0)
    cfg.crop_source = bad
    with pytest.raises(retto_amd.InvalidArgument, match="crop_source"):
        retto_amd.RettoSession(cfg)


def test_session_has_run_regions():
    assert callable(retto_amd.RettoSession.run_regions) and callable(retto_amd.RettoSession.run_regions_raw)
