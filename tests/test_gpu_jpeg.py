"""Encoded pages with JPEG reconstruction on the GPU (rt_decode_batch, rt_submit_encoded_batch).

The kernels' pixels must equal rt_decode_image's byte for byte, on_device must be 1 for every JPEG the device path claims,
and a ticket of encoded pages must give what rt_run_encoded_batch gives for the same files.
"""
import ctypes as C
import gc
import io

import numpy as np
import pytest

import retto_amd
from retto_amd import workload

pytestmark = pytest.mark.gpu

PIL = pytest.importorskip("PIL.Image")
from PIL import Image  # noqa: E402


def _img(h, w, seed, grey=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(xx / 7.0 + seed) + np.cos(yy / 5.0)) * 60 + 128
    a = np.clip(base[..., None] + rng.normal(0, 25, (h, w, 1 if grey else 3)), 0, 255).astype(np.uint8)
    return Image.fromarray(a[..., 0] if grey else a)


def _enc(img, fmt="JPEG", **kw):
    b = io.BytesIO()
    img.save(b, fmt, **kw)
    return b.getvalue()


def _matrix():
    files = []
    for (h, w) in [(1, 1), (3, 2), (17, 9), (8, 130), (37, 53), (200, 120), (960, 960)]:
        for sub in (0, 1, 2):
            for q in (35, 90, 100):
                files.append(_enc(_img(h, w, h + w + q), quality=q, subsampling=sub))
            if h * w < 960 * 960:   # (Pillow's encoder fails on a noisy 960 x 960 progressive 4:4:4 page)
                files.append(_enc(_img(h, w, h + 2 * w), quality=90, subsampling=sub, progressive=True))
        files.append(_enc(_img(h, w, 5, grey=True), quality=90))
    img = _img(120, 200, 9)
    files.append(_enc(img, quality=85, optimize=True))
    files.append(_enc(img, quality=85, restart_marker_blocks=3))
    files.append(_enc(img, quality=85, subsampling=2, restart_marker_rows=1, progressive=True))
    for qt in ([[255] * 64] * 2, [[1000] * 64] * 2, [[32767] * 64, [1] * 64]):
        files.append(_enc(_img(64, 72, 11), qtables=qt, subsampling=2))
    return files


def _text_page_jpeg(h, w, seed, lines=24):
    page, _ = workload.planted_page(h, w, lines, seed=seed)
    return _enc(Image.fromarray(page), quality=90, subsampling=2)


def test_decode_batch_equals_host_decoder(hip_session):
    files = _matrix()
    files.append(_enc(_img(3508, 2480, 1), quality=90, subsampling=2))
    files.append(_text_page_jpeg(4320, 7680, 2, lines=8))
    pages, dev = hip_session.decode_batch(files)
    assert all(dev), [i for i, d in enumerate(dev) if not d]
    for i, (f, p) in enumerate(zip(files, pages)):
        ref = retto_amd.decode_image(f)
        assert p.shape == ref.shape and np.array_equal(p, ref), (i, int((p != ref).sum()) if p.shape == ref.shape else p.shape)


def test_decode_batch_header_only_and_device_memory(hip_session):
    files = [_enc(_img(37, 53, 1), quality=90, subsampling=2), _enc(_img(20, 30, 2), "PNG"), _enc(_img(9, 11, 3), "BMP")]
    lib, h = hip_session._hd.lib, hip_session._hd.h
    n = len(files)
    ptrs = (C.c_char_p * n)(*files); lens = (C.c_size_t * n)(*[len(f) for f in files])
    hs = (C.c_int * n)(); ws = (C.c_int * n)(); dev = (C.c_int * n)()
    assert lib.rt_decode_batch(h, ptrs, lens, n, hs, ws, None, 0, None) == 0
    assert [(hs[i], ws[i]) for i in range(n)] == [(37, 53), (20, 30), (9, 11)]
    bufs = []
    for i in range(n):
        p = C.c_void_p()
        assert lib.rt_device_malloc(h, hs[i] * ws[i] * 3, C.byref(p)) == 0
        bufs.append(p.value)
    try:
        outs = (C.c_void_p * n)(*bufs)
        assert lib.rt_decode_batch(h, ptrs, lens, n, hs, ws, outs, retto_amd.RT_MEM_DEVICE, dev) == 0
        assert list(dev) == [1, 0, 0]
        for i in range(n):
            got = np.empty((hs[i], ws[i], 3), np.uint8)
            assert lib.rt_memcpy_d2h(h, got.ctypes.data, bufs[i], got.nbytes) == 0
            assert np.array_equal(got, retto_amd.decode_image(files[i]))
    finally:
        for b in bufs:
            lib.rt_device_free(h, b)


def test_mixed_formats(hip_session):
    img = _img(33, 47, 4)
    files = [_enc(img, "PNG"), _enc(img, quality=90, subsampling=2), _enc(img, "BMP"), _enc(img, "PPM"),
             _enc(img, quality=75, subsampling=0, progressive=True), _enc(img.convert("L"), "PNG")]
    pages, dev = hip_session.decode_batch(files)
    assert dev == [False, True, False, False, True, False]
    for f, p in zip(files, pages):
        assert np.array_equal(p, retto_amd.decode_image(f))


def _bad_files():
    good = _enc(_img(40, 48, 1), quality=90)
    cmyk = _enc(Image.fromarray(np.random.default_rng(2).integers(0, 256, (16, 16, 4), dtype=np.uint8), "CMYK"), quality=90)
    gif = _enc(_img(16, 16, 3), "GIF")
    return [good[:len(good) // 3], cmyk, gif]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_decode_errors_match_rt_decode_image(hip_session, which):
    bad = _bad_files()[which]
    with pytest.raises(retto_amd.ImageError) as ref:
        retto_amd.decode_image(bad)
    good = [_enc(_img(30, 40, k), quality=90, subsampling=2) for k in range(4)]
    files = good[:2] + [bad] + good[2:]
    with pytest.raises(retto_amd.ImageError) as got:
        hip_session.decode_batch(files)
    assert str(got.value) == str(ref.value)
    pages, dev = hip_session.decode_batch(good)   # the session's next call succeeds
    assert all(dev) and all(np.array_equal(p, retto_amd.decode_image(f)) for p, f in zip(pages, good))


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x.det_result) == len(y.det_result)
        for d, e in zip(x.det_result, y.det_result):
            assert np.array_equal(d.boxes.as_array(), e.boxes.as_array()) and d.score == e.score
        assert [c.label.label for c in x.cls_result] == [c.label.label for c in y.cls_result]
        assert [c.label.score for c in x.cls_result] == [c.label.score for c in y.cls_result]
        for r, s in zip(x.rec_result, y.rec_result):
            assert r.text == s.text and r.score == s.score and np.array_equal(r.tokens, s.tokens)


@pytest.fixture(scope="module")
def c3_files():
    return [_text_page_jpeg(960, 960, 100 + i, lines=32) for i in range(32)]


def _run_encoded_checksum(sess, files):
    lib, h = sess._hd.lib, sess._hd.h
    n = len(files)
    ptrs = (C.c_char_p * n)(*files); lens = (C.c_size_t * n)(*[len(f) for f in files])
    out = C.c_void_p()
    assert lib.rt_run_encoded_batch(h, ptrs, lens, n, None, None, C.byref(out)) == 0
    try:
        return lib.rt_results_det_checksum(out)
    finally:
        lib.rt_results_free(out)


@pytest.mark.parametrize("lanes", [1, 3])
def test_submit_encoded_equals_run_encoded(hip_session, c3_files, lanes):
    """32 JPEG pages of 960 x 960, submitted twice: two tickets in flight."""
    lib, h = hip_session._hd.lib, hip_session._hd.h
    lib.rt_set_lanes(h, lanes)
    try:
        for part in (c3_files,):
            ref = hip_session.run_encoded_batch(part)
            want_cs = _run_encoded_checksum(hip_session, part)
            t1 = hip_session.submit_encoded_batch(part)
            t2 = hip_session.submit_encoded_batch(part)
            got1 = hip_session.wait_batch(t1); cs1 = hip_session.last_det_checksum
            got2 = hip_session.wait_batch(t2); cs2 = hip_session.last_det_checksum
            _same(got1, ref); _same(got2, ref)
            assert cs1 == want_cs and cs2 == want_cs
    finally:
        lib.rt_set_lanes(h, 1 << 20)


def test_submit_encoded_mixed_batch(hip_session):
    img = _img(200, 300, 6)
    files = [_text_page_jpeg(4320, 7680, 7, lines=12), _enc(_img(8, 10, 1), quality=90), _enc(img, "PNG"),
             _text_page_jpeg(640, 480, 8), _enc(img, "BMP"), _enc(img, "PPM")]
    ref = hip_session.run_encoded_batch(files)
    got = hip_session.wait_batch(hip_session.submit_encoded_batch(files))
    _same(got, ref)


def test_submit_encoded_error_leaves_other_tickets(hip_session, c3_files):
    files = c3_files[:6]
    ref = hip_session.run_encoded_batch(files)
    t = hip_session.submit_encoded_batch(files)
    for bad in _bad_files():
        with pytest.raises(retto_amd.ImageError) as want:
            retto_amd.decode_image(bad)
        with pytest.raises(retto_amd.ImageError) as got:
            hip_session.submit_encoded_batch(files[:2] + [bad])
        assert str(got.value) == str(want.value)
    _same(hip_session.wait_batch(t), ref)
    _same(hip_session.wait_batch(hip_session.submit_encoded_batch(files)), ref)


def test_encoded_and_plain_tickets_out_of_order(hip_session, c3_files):
    enc_a, enc_b = c3_files[:8], c3_files[8:12]
    plain = [retto_amd.decode_image(f) for f in c3_files[12:18]]
    ref_a = hip_session.run_encoded_batch(enc_a)
    ref_b = hip_session.run_encoded_batch(enc_b)
    ref_p = hip_session.run_batch(plain)
    ta = hip_session.submit_encoded_batch(enc_a)
    tp = hip_session.submit_batch_raw(plain, [p.shape[0] for p in plain], [p.shape[1] for p in plain])
    tb = hip_session.submit_encoded_batch(enc_b)
    _same(hip_session.wait_batch(tb), ref_b)
    _same(hip_session.wait_batch(tp), ref_p)
    _same(hip_session.wait_batch(ta), ref_a)
    # slot reuse: page sizes grow, then shrink
    seq = [[_text_page_jpeg(320, 480, 50)], [_text_page_jpeg(1600, 1200, 51, lines=16)] * 3, [_text_page_jpeg(240, 200, 52, lines=4)] * 2]
    refs = [hip_session.run_encoded_batch(f) for f in seq]
    for f, r in zip(seq, refs):
        _same(hip_session.wait_batch(hip_session.submit_encoded_batch(f)), r)


def test_file_buffers_freed_after_submit(hip_session, c3_files):
    files = c3_files[20:26]
    ref = hip_session.run_encoded_batch(files)
    lib, h = hip_session._hd.lib, hip_session._hd.h
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ptrs = (C.c_char_p * n)(*[C.cast(b, C.c_char_p) for b in bufs]); lens = (C.c_size_t * n)(*[len(f) for f in files])
    t = C.c_void_p()
    assert lib.rt_submit_encoded_batch(h, ptrs, lens, n, C.byref(t)) == 0
    for b in bufs:                 # overwrite, then drop, the caller's file bytes while the ticket is in flight
        C.memset(b, 0xEE, len(b))
    del bufs, ptrs
    gc.collect()
    _same(hip_session.wait_batch((t, [])), ref)
