"""The kernel-level debug entry points rt_debug_gemm / rt_debug_attention (tests/test_gpu_ops.py drives them on the GPU):
declared, exported, and null or bad arguments rejected with RT_ERR_INVALID before any device work."""
import ctypes as C
import os

import numpy as np

from retto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = 8


def test_debug_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    lib = _lib.load()
    for name in ("rt_debug_gemm", "rt_debug_attention"):
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
