"""Device JPEG entropy decoding without a GPU: the host preparation (unstuffed stream, segments, tables, geometry) and the decode
step the kernels share with the CPU (retto_amd/csrc/jpeg_huff.h), run serially by rt_debug_jpeg_entropy how = 2, against the host
decoder's coefficients (how = 0), which are exact integers.  CASES is the matrix tests/test_gpu_jpeg_entropy.py runs on the GPU."""
import io

import numpy as np
import pytest
from PIL import Image

import retto_amd


def jpeg(h, w, seed=0, mode="RGB", flat=False, **kw):
    rng = np.random.default_rng(seed)
    shape = (h, w) if mode == "L" else (h, w, 3)
    a = np.full(shape, 200, np.uint8) if flat else rng.integers(0, 256, shape, dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(a, mode).save(b, "JPEG", **kw)
    return b.getvalue()


# name -> (height, width, keywords of jpeg()).  Noise at quality 95 codes about 3.5 bits per pixel and component: 17 x 9 and
# 8 x 130 are a few 512-bit subsequences, 80 x 80 most of one 256-lane workgroup, 256 x 256 several workgroups.
CASES = {
    "1x1": (1, 1, dict(quality=90, subsampling=0)),
    "17x9": (17, 9, dict(quality=95, subsampling=0)),
    "8x130": (8, 130, dict(quality=95, subsampling=0)),
    "one_workgroup": (80, 80, dict(quality=95, subsampling=0)),
    "several_workgroups": (256, 256, dict(quality=95, subsampling=0)),
    "grey": (67, 93, dict(quality=90, mode="L")),
    "422": (67, 93, dict(quality=90, subsampling=1)),
    "420": (67, 93, dict(quality=90, subsampling=2)),
    "q35": (67, 93, dict(quality=35, subsampling=2)),
    "q100": (67, 93, dict(quality=100, subsampling=0)),
    "optimize": (67, 93, dict(quality=97, subsampling=2, optimize=True)),
    "restart_blocks3": (67, 93, dict(quality=90, subsampling=2, restart_marker_blocks=3)),
    "restart_rows1": (67, 93, dict(quality=90, subsampling=0, restart_marker_rows=1)),
    "flat": (120, 200, dict(quality=90, subsampling=2, flat=True)),
}


def case_file(name):
    h, w, kw = CASES[name]
    return jpeg(h, w, seed=sorted(CASES).index(name), **kw)


def assert_same_planes(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)


@pytest.mark.parametrize("name", sorted(CASES))
def test_serial_step_functions_equal_host_decoder(name):
    data = case_file(name)
    ref, _ = retto_amd.debug_jpeg_entropy(data, 0)
    got, info = retto_amd.debug_jpeg_entropy(data, 2)
    assert info["taken"] == 1 and info["flag"] == 0
    assert_same_planes(got, ref)


def test_preparation_refuses_other_markers_and_scans():
    data = case_file("420")
    sos = data.index(b"\xff\xda")
    at = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big") + 40   # inside the entropy data
    while data[at - 1] == 0xFF:
        at += 1
    with_marker = data[:at] + b"\xff\xfe\x00\x04ab" + data[at:]   # a COM segment: no RSTn
    assert retto_amd.debug_jpeg_entropy(with_marker, 2)[1]["taken"] == 0
    progressive = jpeg(67, 93, quality=90, progressive=True)
    assert retto_amd.debug_jpeg_entropy(progressive, 2)[1]["taken"] == 0
    assert retto_amd.debug_jpeg_entropy(data, 2)[1]["taken"] == 1
