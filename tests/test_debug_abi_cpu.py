"""The kernel-level debug entry points rt_debug_gemm / rt_debug_attention (tests/test_gpu_ops.py drives them on the GPU) and
rt_debug_lc_block / rt_debug_conv13 / rt_debug_layernorm (tests/test_gpu_rec_kernels.py): declared, exported, and null or bad
arguments rejected with RT_ERR_INVALID before any device work."""
import ctypes as C
import os

import numpy as np

from retto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = 8


def test_debug_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    lib = _lib.load()
    for name in ("rt_debug_gemm", "rt_debug_attention", "rt_debug_lc_block", "rt_debug_conv13", "rt_debug_layernorm"):
        assert "RT_API int %s(" % name in header
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)


def _gemm(lib, s=None, A=True, M=4, K=8, lda=8, W=True, N=4, ldc=4, coff=0, act=2, res=None, ld_res=0, se=None, ld_scale=0,
          rows=None, n_img=0, se_rows=0, variant=0, ctc=-1, out=True, idx=None, prob=None, plan=True):
    a = np.zeros((M, max(lda, 1)), np.float32)
    w = np.zeros((K, N), np.float32)
    o = np.zeros(((M + 64) * max(ldc, 1),), np.float32)
    pl = (C.c_int * 5)()
    return lib.rt_debug_gemm(s, a.ctypes.data if A else None, M, K, lda, w.ctypes.data if W else None, N, None, act, 0, 1.0, 0.0,
                             res, ld_res, se, ld_scale, rows, n_img, se_rows, ldc, coff, variant, ctc, o.ctypes.data if out else None,
                             idx, prob, pl if plan else None)


def test_debug_null_and_bad_arguments_are_rejected_without_a_device():
    lib = _lib.load()
    # (no session can be created without a device: the null session is rejected whatever the other arguments)
    for kw in ({}, {"A": False}, {"W": False}, {"out": False}, {"plan": False}, {"M": 0}, {"ldc": 2}, {"ctc": 0}):
        assert _gemm(lib, **kw) == RT_ERR_INVALID, kw
    q = np.zeros((4, 3 * 8 * 15), np.float32)
    o = np.zeros((4, 8 * 15), np.float32)
    t = np.array([2, 2], np.int32)
    assert lib.rt_debug_attention(None, q.ctypes.data, 4, t.ctypes.data, 2, 8, o.ctypes.data) == RT_ERR_INVALID
    assert lib.rt_debug_attention(None, None, 4, t.ctypes.data, 2, 8, o.ctypes.data) == RT_ERR_INVALID
    assert lib.rt_debug_attention(None, q.ctypes.data, 4, None, 2, 8, o.ctypes.data) == RT_ERR_INVALID
    assert lib.rt_debug_attention(None, q.ctypes.data, 4, t.ctypes.data, 0, 8, None) == RT_ERR_INVALID


def _lc(lib, s=None, x=True, hs=(3, 2), ws=(5, 1), n_img=2, cin=16, cout=32, sh=1, sw=1, dww=True, dwb=True, pww=True, pwb=True,
        dw_act=2, form=3, out=True, info=True):
    a = lambda shape, dt=np.float32: np.zeros(shape, dt)   # noqa: E731
    p = lambda arr, on: arr.ctypes.data if on else None    # noqa: E731
    xs, h, w = a((17, max(cin, 1))), np.array(hs, np.int32), np.array(ws, np.int32)
    dw_w, dw_b, pw_w, pw_b = a((max(cin, 1), 3, 3)), a(max(cin, 1)), a((max(cout, 1), max(cin, 1))), a(max(cout, 1))
    o = a((17 + 64, max(cout, 1)))
    return lib.rt_debug_lc_block(s, p(xs, x), h.ctypes.data, w.ctypes.data, n_img, cin, cout, sh, sw, p(dw_w, dww), p(dw_b, dwb),
                                 p(pw_w, pww), p(pw_b, pwb), dw_act, 1, 1.3, 0.07, 1, 0.8, -0.05, form, p(o, out),
                                 (C.c_int * 1)() if info else None)


def _conv13(lib, s=None, x=True, rows=5, ldx=8, toks=(2, 3), n_lines=2, cin=8, w=True, cout=4, act=3, form=1, out=True, info=True):
    xs, t = np.zeros((max(rows, 1), max(ldx, 1)), np.float32), np.array(toks, np.int32)
    wt, b, o = np.zeros((max(cout, 1), max(cin, 1), 1, 3), np.float32), np.zeros(max(cout, 1), np.float32), np.zeros((max(rows, 1) + 64, 64), np.float32)
    return lib.rt_debug_conv13(s, xs.ctypes.data if x else None, rows, ldx, t.ctypes.data, n_lines, cin, wt.ctypes.data if w else None,
                               cout, b.ctypes.data, act, form, o.ctypes.data if out else None, (C.c_int * 2)() if info else None)


def _ln(lib, s=None, x=True, rows=3, c=120, g=True, beta=True, eps=1e-5, out=True):
    xs, gg, bb, o = np.zeros((max(rows, 1), max(c, 1)), np.float32), np.ones(max(c, 1), np.float32), np.zeros(max(c, 1), np.float32), np.zeros((max(rows, 1) + 64, max(c, 1)), np.float32)
    return lib.rt_debug_layernorm(s, xs.ctypes.data if x else None, None, rows, c, gg.ctypes.data if g else None,
                                  bb.ctypes.data if beta else None, eps, o.ctypes.data if out else None)


def test_rec_kernel_entries_reject_null_and_bad_arguments_without_a_device():
    lib = _lib.load()
    for kw in ({}, {"x": False}, {"dww": False}, {"dwb": False}, {"pww": False}, {"pwb": False}, {"out": False}, {"info": False},
               {"n_img": 0}, {"cin": 0}, {"cout": 0}, {"sh": 3}, {"sw": 0}, {"form": 2}, {"dw_act": 9}, {"hs": (3, 0)}):
        assert _lc(lib, **kw) == RT_ERR_INVALID, kw
    for kw in ({}, {"x": False}, {"w": False}, {"out": False}, {"info": False}, {"rows": 0}, {"n_lines": 0}, {"cin": 6}, {"ldx": 4},
               {"cout": 65}, {"form": 2}, {"act": -1}, {"toks": (2, 0)}, {"toks": (2, 2)}):
        assert _conv13(lib, **kw) == RT_ERR_INVALID, kw
    for kw in ({}, {"x": False}, {"g": False}, {"beta": False}, {"out": False}, {"rows": 0}, {"c": 0}, {"c": 257}, {"eps": 0.0}):
        assert _ln(lib, **kw) == RT_ERR_INVALID, kw
