"""JPEG reconstruction of the device decode path, checked without a GPU.

rt_debug_jpeg_reconstruct runs the host stage of rt_submit_encoded_batch / rt_decode_batch (parse and entropy decoding into
quantised int16 coefficients) and then the arithmetic of k_jpeg_idct / k_jpeg_color -- the __host__ __device__ functions of
retto_amd/csrc/jpeg_recon.h -- on the CPU.  Its pixels must equal rt_decode_image's byte for byte, and every file below must
be one the device path takes (on_device), so a silent host fallback cannot pass.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

PIL = pytest.importorskip("PIL.Image")
from PIL import Image  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 2), (17, 9), (8, 130), (37, 53), (200, 120), (960, 960)]


def _img(h, w, seed, grey=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(xx / 7.0 + seed) + np.cos(yy / 5.0)) * 60 + 128
    a = np.clip(base[..., None] + rng.normal(0, 25, (h, w, 1 if grey else 3)), 0, 255).astype(np.uint8)
    return Image.fromarray(a[..., 0] if grey else a)


def _jpeg(img, **kw):
    b = io.BytesIO()
    img.save(b, "JPEG", **kw)
    return b.getvalue()


def _check(data):
    ref = retto_amd.decode_image(data)
    got, on_device = retto_amd.debug_jpeg_reconstruct(data)
    assert on_device, "the device path would decode this file on the host"
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), "differs in %d bytes" % int((got != ref).sum())


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("q", [35, 90, 100])
def test_sequential_matrix(h, w, sub, q):
    _check(_jpeg(_img(h, w, h * 7 + w), quality=q, subsampling=sub))


@pytest.mark.parametrize("h,w", [(1, 1), (3, 2), (17, 9), (37, 53), (200, 120)])
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_progressive(h, w, sub):
    _check(_jpeg(_img(h, w, 3 + h), quality=90, subsampling=sub, progressive=True))


@pytest.mark.parametrize("h,w", [(1, 1), (17, 9), (200, 120)])
@pytest.mark.parametrize("prog", [False, True])
def test_grey(h, w, prog):
    _check(_jpeg(_img(h, w, 5, grey=True), quality=90, progressive=prog))


@pytest.mark.parametrize("sub", [0, 2])
def test_optimised_tables_and_restart_intervals(sub):
    img = _img(120, 200, 9)
    _check(_jpeg(img, quality=85, subsampling=sub, optimize=True))
    _check(_jpeg(img, quality=85, subsampling=sub, restart_marker_blocks=3))
    _check(_jpeg(img, quality=85, subsampling=sub, restart_marker_rows=1, progressive=True))


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_quantisation_table_extremes(sub):
    """All-255 8-bit tables, and 16-bit tables (Pillow writes Pq = 1 above 255) up to 32767: products past 2^24 drive the
    dequantisation clamp, large coefficients the 0..255 clamp of the transform."""
    img = _img(64, 72, 11)
    for qt in ([[255] * 64] * 2, [[1000] * 64] * 2, [[32767] * 64, [1] * 64], [[1] * 64, [32767] * 64]):
        data = _jpeg(img, qtables=qt, subsampling=sub)
        _check(data)
        if qt[0][0] == 1000:   # the file really carries 16-bit tables
            assert data[data.find(b"\xff\xdb") + 4] >> 4 == 1


def _rgb_coded(data):
    """A 4:4:4 file with its component ids patched to 'R', 'G', 'B' in the frame and scan headers (no Adobe segment: Pillow
    writes JFIF), so the decoder must pass the samples through instead of converting from YCbCr."""
    d = bytearray(data)
    sof = d.find(b"\xff\xc0")
    assert sof > 0 and d[sof + 9] == 3
    for k, cid in enumerate(b"RGB"):
        d[sof + 10 + 3 * k] = cid
    pos = 0
    while True:
        sos = d.find(b"\xff\xda", pos)
        if sos < 0:
            break
        ns = d[sos + 4]
        for k in range(ns):
            d[sos + 5 + 2 * k] = b"RGB"[d[sos + 5 + 2 * k] - 1]
        pos = sos + 2
    return bytes(d)


def test_rgb_coded_file():
    data = _rgb_coded(_jpeg(_img(37, 53, 13), quality=90, subsampling=0))
    ref = retto_amd.decode_image(data)
    ycc = retto_amd.decode_image(_jpeg(_img(37, 53, 13), quality=90, subsampling=0))
    assert not np.array_equal(ref, ycc)   # the patch changed how the samples are read
    _check(data)


def test_non_jpeg_pages_are_host_decoded():
    img = _img(9, 11, 2)
    for fmt in ("PNG", "BMP", "PPM"):
        b = io.BytesIO(); img.save(b, fmt); data = b.getvalue()
        got, on_device = retto_amd.debug_jpeg_reconstruct(data)
        assert not on_device
        assert np.array_equal(got, retto_amd.decode_image(data))


def test_decode_errors_match_the_host_decoder():
    good = _jpeg(_img(40, 48, 1), quality=90)
    for bad in (good[:len(good) // 3], b"GIF89a" + b"\0" * 20, b"not an image"):
        with pytest.raises(retto_amd.ImageError) as a:
            retto_amd.decode_image(bad)
        with pytest.raises(retto_amd.ImageError) as b:
            retto_amd.debug_jpeg_reconstruct(bad)
        assert str(a.value) == str(b.value)


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    lib = _lib.load()
    for name in ("rt_submit_encoded_batch", "rt_decode_batch", "rt_debug_jpeg_reconstruct"):
        assert "RT_API int %s(" % name in header
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)


def test_null_arguments_are_rejected_without_a_device():
    lib = _lib.load()
    RT_ERR_INVALID = 8
    t = C.c_void_p(123)
    assert lib.rt_submit_encoded_batch(None, None, None, 1, C.byref(t)) == RT_ERR_INVALID
    assert t.value is None                           # *out is cleared
    assert lib.rt_submit_encoded_batch(None, None, None, 0, None) == RT_ERR_INVALID
    h = (C.c_int * 1)(); w = (C.c_int * 1)()
    assert lib.rt_decode_batch(None, None, None, 1, h, w, None, 0, None) == RT_ERR_INVALID
    assert lib.rt_decode_batch(None, None, None, 0, None, None, None, 0, None) == RT_ERR_INVALID
    out = C.c_void_p(); hh = C.c_int(); ww = C.c_int(); dev = C.c_int()
    assert lib.rt_debug_jpeg_reconstruct(None, 0, C.byref(out), C.byref(hh), C.byref(ww), C.byref(dev), None, 0) == RT_ERR_INVALID
