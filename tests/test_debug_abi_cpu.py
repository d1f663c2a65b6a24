"""The kernel-level debug entry points rt_debug_gemm / rt_debug_attention (tests/test_gpu_ops.py drives them on the GPU) and
rt_debug_lc_block / rt_debug_conv13 / rt_debug_layernorm (tests/test_gpu_rec_kernels.py) and rt_debug_glue16 / rt_debug_conv16x
(tests/test_gpu_f16_kernels.py) and rt_debug_fpn (tests/test_gpu_fpn_kernels.py) and rt_debug_cls_block / rt_debug_stem /
rt_debug_glue32 (tests/test_gpu_cls_kernels.py) and rt_debug_dw_plan / rt_debug_lc_wide (tests/test_gpu_dw_kernels.py): declared, exported, and null or bad arguments rejected with RT_ERR_INVALID before
any device work."""
import ctypes as C
import os

import numpy as np

from retto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = 8


def test_debug_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    lib = _lib.load()
    for name in ("rt_debug_gemm", "rt_debug_attention", "rt_debug_lc_block", "rt_debug_conv13", "rt_debug_layernorm",
                 "rt_debug_glue16", "rt_debug_conv16x", "rt_debug_fpn", "rt_debug_cls_block", "rt_debug_stem", "rt_debug_glue32",
                 "rt_debug_dw_plan", "rt_debug_lc_wide"):
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


def _glue(lib, s=None, op=3, ip=(24, 24, 0, 48, 24, 24, 0, 0), fp=True, ipp=True, sh=True, sw=True, dh=True, dw=True, n_img=2, x=True, x_len=None,
          x2=True, x2_len=None, tab=True, tab_len=None, out=True, out_len=None, hs=(3, 1), ws=(2, 1)):
    """scale_channels16 with a residual on two images of 6 and 1 pixels, unless the arguments say otherwise"""
    i = np.zeros(12, np.int32); i[:len(ip)] = ip   # noqa: E702
    f = np.zeros(8, np.float32)
    h, w = np.array(hs, np.int32), np.array(ws, np.int32)
    pix = 7
    xs, x2s, t, o = np.zeros(pix * 64, np.float32), np.zeros(pix * 64, np.float32), np.zeros(256, np.float32), np.zeros((pix + 64) * 64, np.float32)
    p = lambda arr, on: arr.ctypes.data if on else None   # noqa: E731
    d = lambda v, dflt: dflt if v is None else v          # noqa: E731
    return lib.rt_debug_glue16(s, op, p(i, ipp), p(f, fp), p(h, sh), p(w, sw), p(h, dh), p(w, dw), n_img, p(xs, x), d(x_len, pix * max(int(i[1]), 1)),
                               p(x2s, x2), d(x2_len, pix * max(int(i[5]), 0)), p(t, tab), d(tab_len, 2 * max(int(i[0]), 0)), p(o, out),
                               d(out_len, (pix + 64) * max(int(i[3]), 1)))


def test_glue16_rejects_null_and_bad_arguments_without_a_device():
    """rt_debug_glue16 looks at its session last, so without a device every argument check still answers with its own message
    (rt_last_error(NULL) holds it): a check that was skipped would show as "null session"."""
    lib = _lib.load()
    null, op, chan, pitch8, window, params, lens, aux, img = (
        "null argument", "bad op or image count", "bad channel counts", "multiples of 8", "leaves the row", "bad parameters for the op",
        "x is too short or out has the wrong length", "x2 or tab is missing or too short", "empty or oversized image")
    sc = lambda *tail: (24, 24, 0, 48, 24) + tail   # noqa: E731  scale_channels16: x pitch 24 -> y pitch 48 at 24; tail = ldr, roff, in place
    cases = [({}, "null session"),
             ({"ipp": False}, null), ({"fp": False}, null), ({"sh": False}, null), ({"sw": False}, null), ({"dh": False}, null),
             ({"dw": False}, null), ({"x": False}, null), ({"out": False}, null), ({"x2": False}, aux), ({"tab": False}, aux),
             ({"n_img": 0}, op), ({"op": -1}, op), ({"op": 15}, op), ({"hs": (3, 0)}, img), ({"ws": (0, 1)}, img),
             ({"ip": (0, 24, 0, 48, 24, 24, 0, 0)}, chan),           # no channels
             ({"ip": (24, 0, 0, 48, 24, 24, 0, 0)}, chan),           # no source pitch
             ({"ip": (24, 16, 0, 48, 24, 24, 0, 0)}, window),        # source pitch below C
             ({"ip": (24, 28, 0, 48, 24, 24, 0, 0)}, pitch8),        # source pitch no multiple of 8
             ({"ip": (24, 24, 0, 52, 24, 24, 0, 0)}, pitch8),        # destination pitch no multiple of 8
             ({"ip": (24, 24, 0, 48, 20, 24, 0, 0)}, pitch8),        # destination offset no multiple of 8
             ({"ip": (24, 24, 0, 48, 32, 24, 0, 0)}, window),        # the window leaves the row
             ({"ip": sc(20, 0, 0)}, params),                         # residual pitch misaligned
             ({"ip": sc(24, 8, 0)}, params),                         # the residual's window leaves its row
             ({"ip": sc(24, 0, 1)}, params),                         # in place with different pitches
             ({"x_len": 7 * 24 - 1}, lens), ({"x2_len": 7 * 24 - 1}, aux), ({"tab_len": 47}, aux), ({"out_len": (7 + 64) * 48 - 1}, lens),
             ({"out_len": 0}, lens),
             # per-op parameter blocks: a geometry the kernel would read or write out of bounds with, a parameter it has no instance for
             ({"op": 0, "ip": (24, 24, 0, 24, 0, 4, 1, 1, 0, 0)}, params),      # dwconv16: K = 4
             ({"op": 0, "ip": (24, 24, 0, 24, 0, 3, 2, 2, 0, 0)}, params),      # dwconv16: destination is not ceil(source / stride)
             ({"op": 7, "ip": (24, 24, 0, 24, 0, 3, 2)}, params),               # avgpool16: the windows leave the source
             ({"op": 8, "ip": (24, 48, 0, 24, 0)}, window),                     # pixel_shuffle16: 4 C channels do not fit the source pitch
             ({"op": 9, "ip": (24, 24, 0, 1, 0)}, params),                      # deconv_to_map16: the map is not 2 x the features
             ({"op": 5, "ip": (24, 24, 0, 48, 24, 4, 0)}, params),              # upsample_into16: shift 4
             ({"op": 5, "ip": (24, 24, 0, 48, 24, 1, 16)}, params),             # upsample_into16: scale pitch below C
             ({"op": 6, "ip": (24, 24, 0, 24, 0, 2, 2, 2, 2, 2, 0)}, params),   # maxpool16: pad >= window
             ({"op": 10, "ip": (16, 1, 0, 24, 16)}, window),                    # map_window16: 16 channels from 16 leave a pitch of 24
             ({"op": 2, "ip": (24, 24, 0, 16, 0, 0)}, params),                  # gate16: Cp < C
             ({"op": 13, "ip": (24, 16, 0, 24, 0)}, window)]                    # h_to_f32: C above the source pitch
    lib.rt_last_error.restype = C.c_char_p
    for kw, why in cases:
        assert _glue(lib, **kw) == RT_ERR_INVALID, kw
        assert why in lib.rt_last_error(None).decode(), (kw, lib.rt_last_error(None))



def _conv16x(lib, s=None, ip=None, ipp=True, fp=True, hh=True, ww=True, n_img=2, x=True, x_len=None, wt=True, wt_len=None, res=False,
             res_len=None, dot=False, out=True, out_len=None, route=True, hs=(3, 1), ws=(2, 1), **named):
    """3x3 32 -> 24 relu on two images of 6 and 1 pixels, channels 8 .. 39 of pitch 48 into channels 8 .. 31 of pitch 40, unless
    the arguments say otherwise; named = single ip entries by name"""
    names = ("cin", "ldx", "xoff", "cout", "ldy", "coff", "kh", "kw", "sh", "sw", "pt", "pl", "flat", "act", "has_lab", "ld_res", "res_off",
             "in_place", "dot_py", "dot_px")
    i = np.array(ip if ip is not None else (32, 48, 8, 24, 40, 8, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 0), np.int32)
    for k, v in named.items():
        i[names.index(k)] = v
    f = np.zeros(3, np.float32)
    h, w = np.array(hs, np.int32), np.array(ws, np.int32)
    pix = 7
    xs, wts, rs, dws, o = (np.zeros(n, np.float32) for n in (pix * 128, 64 * 128 * 9, pix * 128, 64, (4 * pix + 64) * 128))
    r = (C.c_int * 1)()
    p = lambda arr, on: arr.ctypes.data if on else None   # noqa: E731
    d = lambda v, dflt: dflt if v is None else v          # noqa: E731
    return lib.rt_debug_conv16x(s, p(i, ipp), p(f, fp), p(h, hh), p(w, ww), n_img, p(xs, x), d(x_len, pix * max(int(i[1]), 1)),
                                p(wts, wt), d(wt_len, int(i[3]) * int(i[0]) * int(i[6]) * int(i[7])), None, p(rs, res),
                                d(res_len, pix * max(int(i[15]), 0)), p(dws, dot), p(o, out),
                                d(out_len, 4 * pix + 64 if dot else (pix + 64) * max(int(i[4]), 1)), r if route else None)


def test_conv16x_rejects_null_and_bad_arguments_without_a_device():
    """as rt_debug_glue16: the session is looked at last, so every argument check answers with its own message"""
    lib = _lib.load()
    null, count, chan, in8, outw, launch, img, place, lens, resid = (
        "null argument", "bad image count", "bad channel counts", "input channels, pitch and offset", "output window", "no such launch",
        "empty or oversized image", "in place needs", "x is too short, or wt or out", "the residual is")
    phase = (80, 80, 0, 64, 8, 0, 2, 2, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1)   # a PFHeadLocal phase conv (dot=True goes with it)
    cases = [({}, "null session"), ({"dot": True, "ip": phase}, "null session"), ({"res": True, "ld_res": 32, "res_off": 8}, "null session"),
             ({"ipp": False}, null), ({"fp": False}, null), ({"hh": False}, null), ({"ww": False}, null), ({"x": False}, null),
             ({"wt": False}, null), ({"out": False}, null), ({"route": False}, null),
             ({"n_img": 0}, count), ({"hs": (3, 0)}, img), ({"ws": (0, 1)}, img),
             ({"cin": 0}, chan), ({"cout": 0}, chan), ({"ldx": 0}, chan), ({"ldx": 32}, chan),     # (the window 8 .. 39 leaves a pitch of 32)
             ({"cin": 36}, in8), ({"ldx": 52}, in8), ({"xoff": 4}, in8),
             ({"ldy": 0}, outw), ({"ldy": 44}, outw), ({"coff": 4}, outw), ({"coff": 24}, outw),    # (24 + pitch8(24) > 40)
             ({"cout": 34}, outw),                                                                   # (pad channels 34 .. 39 leave the row)
             ({"kh": 2}, launch), ({"kh": 2, "kw": 2}, launch),                                      # (2x2 without the dot epilogue)
             ({"dot": True}, launch),                                                                # (the dot epilogue on a 3x3)
             ({"dot": True, "ip": phase, "cout": 96}, launch), ({"dot": True, "ip": phase, "pt": 2}, launch),
             ({"dot": True, "ip": phase, "dot_py": 2}, launch), ({"dot": True, "ip": phase, "cin": 24, "ldx": 24}, launch),
             ({"sh": 3}, launch), ({"sw": 0}, launch), ({"pt": 0}, launch), ({"act": 5}, launch), ({"flat": 1}, launch), ({"kw": 11}, launch),
             ({"in_place": 1}, place), ({"in_place": 1, "ldy": 48, "sh": 2}, place),
             ({"x_len": 7 * 48 - 1}, lens), ({"wt_len": 24 * 32 * 9 - 1}, lens), ({"out_len": (7 + 64) * 40 - 1}, lens), ({"out_len": 0}, lens),
             ({"dot": True, "ip": phase, "out_len": 4 * 7 + 63}, lens),
             ({"res": True, "ld_res": 0}, resid), ({"res": True, "ld_res": 28}, resid), ({"res": True, "ld_res": 32, "res_off": 4}, resid),
             ({"res": True, "ld_res": 32, "res_off": 16}, resid), ({"res": True, "ld_res": 32, "res_len": 7 * 32 - 1}, resid)]
    lib.rt_last_error.restype = C.c_char_p
    for kw, why in cases:
        assert _conv16x(lib, **kw) == RT_ERR_INVALID, kw
        assert why in lib.rt_last_error(None).decode(), (kw, lib.rt_last_error(None))


def _fpn(lib, s=None, op=0, ip=(12, 96, 1 | 2), fpv=(0.2,), fine=((8, 8), (4, 4)), coarse=((4, 4), (2, 2)), n_img=2, ipp=True, fpp=True,
         fh=True, cw=True, inp=True, outp=True, info=True, lens=None, short=None, missing=None, out_short=None):
    """the phase conv <3, 4, 0> with bias and pool on two images, unless the arguments say otherwise; lens = the operands' lengths by
    slot (pf = 80, pc = 20 pixels), short / missing = a slot one float short / a NULL slot, out_short = an output slot one float short"""
    i = np.zeros(8, np.int32); i[:len(ip)] = ip   # noqa: E702
    f = np.zeros(4, np.float32); f[:len(fpv)] = fpv   # noqa: E702
    g = [np.array(v, np.int32) for v in ([a for a, _ in fine], [b for _, b in fine], [a for a, _ in coarse], [b for _, b in coarse])]
    if lens is None:
        lens = {0: 80 * 12, 1: 20 * 96, 2: 24 * 96 * 9, 3: 24, 4: 2 * 216 * 12}
    olens = {0: (80 + 64) * 24, 1: (2 * 1 + 64) * 24} if isinstance(outp, bool) else dict(outp)
    arrs = [np.zeros(max(lens.get(k, 0) - (1 if k == short else 0), 1), np.float32) for k in range(10)]
    ptrs = (C.c_void_p * 10)(*[a.ctypes.data if k in lens and k != missing else None for k, a in enumerate(arrs)])
    ilen = (C.c_longlong * 10)(*[lens.get(k, 0) - (1 if k == short else 0) for k in range(10)])
    outs = [np.zeros(max(olens.get(k, 0), 1), np.float32) for k in range(3)]
    optrs = (C.c_void_p * 3)(*[a.ctypes.data if k in olens else None for k, a in enumerate(outs)])
    olen = (C.c_longlong * 3)(*[olens.get(k, 0) - (1 if k == out_short else 0) for k in range(3)])
    p = lambda arr, on: arr.ctypes.data if on else None   # noqa: E731
    return lib.rt_debug_fpn(s, op, p(i, ipp), p(f, fpp), p(g[0], fh), g[1].ctypes.data, g[2].ctypes.data, p(g[3], cw), n_img,
                            ptrs if inp else None, ilen, optrs if outp is not False else None, olen, (C.c_int * 1)() if info else None)


def test_fpn_rejects_null_and_bad_arguments_without_a_device():
    """as rt_debug_glue16: the session is looked at last, so every argument check answers with its own message"""
    lib = _lib.load()
    null, opn, img, twice, params, inst, operand, output = (
        "null argument", "bad op or image count", "empty or oversized image", "not exactly twice", "bad parameters for the op",
        "no kernel instance", "an operand is missing or too short", "an output is missing or has the wrong length")
    W = 24 * 96 * 9
    head = {0: 80 * 24, 1: 20 * 24, 2: W, 7: 48, 8: 48, 9: 9 * 5 * 24}        # the head conv with G and both scales
    head_out = {0: (80 + 64) * 24}
    cls = {0: 80 * 24, 1: W, 2: 24, 3: 48, 4: 9 * 20 * 24}
    cases = [({}, "null session"),
             ({"ip": (24, 24, 8 | 4 | 16 | 32), "lens": head, "outp": head_out}, "null session"),
             ({"op": 1, "ip": (24, 7), "lens": cls, "outp": {0: (9 * 80 + 64) * 24}}, "null session"),
             ({"op": 2, "ip": (18,), "lens": {0: 96 * 18, 1: 2 * 96, 2: W}, "outp": {0: (2 * 216 + 64) * 20}}, "null session"),
             ({"op": 3, "lens": {0: 80 * 24, 1: 2304, 2: 24, 3: 96, 4: 1}, "outp": {0: 16 * 80 + 1024}}, "null session"),
             ({"ipp": False}, null), ({"fpp": False}, null), ({"fh": False}, null), ({"cw": False}, null), ({"inp": False}, null),
             ({"outp": False}, null), ({"info": False}, null),
             ({"op": -1}, opn), ({"op": 10}, opn), ({"n_img": 0}, opn),
             ({"fine": ((8, 8), (0, 4))}, img), ({"coarse": ((4, 4), (2, 0))}, img), ({"fine": ((8, 5000), (4, 4))}, img),
             ({"coarse": ((4, 4), (2, 3))}, twice), ({"fine": ((8, 8), (5, 4))}, twice), ({"fine": ((9, 8), (4, 4)), "coarse": ((5, 4), (2, 2))}, twice),
             # the head's class tensor lives at a quarter of the fine level: 4 x 4 -> 2 x 2 -> 1 x 1, but 6 x 4 -> 3 x 2 has no half
             ({"ip": (24, 24, 8), "lens": head, "outp": head_out, "fine": ((8, 8), (6, 4)), "coarse": ((4, 4), (3, 2))}, twice),
             ({"op": 1, "ip": (24, 7), "lens": cls, "outp": {0: (9 * 80 + 64) * 24}, "coarse": ((4, 4), (2, 1))}, twice),
             ({"ip": (0, 96, 3)}, params), ({"ip": (12, 0, 3)}, params), ({"ip": (12, 96, 128)}, params), ({"ip": (24, 24, 8 | 1)}, params),
             ({"op": 1, "ip": (12, 0), "lens": cls}, params), ({"op": 1, "ip": (96, 0), "lens": cls}, params), ({"op": 1, "ip": (0, 8), "lens": cls}, params),
             ({"op": 2, "ip": (0,)}, params), ({"op": 4, "ip": (65, 0)}, params), ({"op": 5, "ip": (2, 0)}, params),
             ({"op": 6, "ip": (12, 0, 1)}, params), ({"op": 6, "ip": (12, 24, 1), "fpv": (0.0,)}, params), ({"op": 7, "ip": (25, 1)}, params),
             ({"op": 8, "ip": (64,), "fine": ((8, 8), (16, 8)), "coarse": ((4, 4), (8, 4))}, params),
             ({"op": 8, "ip": (0,)}, twice),         # (the fused head reads four levels: 4 x 4 has no eighth)
             ({"op": 9, "ip": (4,)}, params),
             ({"ip": (12, 24, 3)}, inst), ({"ip": (16, 96, 3)}, inst), ({"ip": (24, 96, 3)}, inst), ({"ip": (8, 96, 3)}, inst),
             ({"ip": (22, 24, 3)}, inst), ({"ip": (10, 96, 3)}, inst), ({"ip": (17, 96, 3)}, inst), ({"ip": (20, 96, 3)}, inst),   # an instance exists, the net has no such layer
             ({"ip": (12, 96, 8)}, inst),            # G with an inp conv
             ({"ip": (12, 96, 16)}, inst),           # a fine scale with an inp conv
             ({"ip": (24, 24, 64)}, inst),           # compose with the head conv
             ({"op": 2, "ip": (24,)}, inst), ({"op": 2, "ip": (16,)}, inst), ({"op": 2, "ip": (11,)}, inst), ({"op": 2, "ip": (20,)}, inst),
             ({"short": 0}, operand), ({"short": 1}, operand), ({"short": 2}, operand), ({"short": 3}, operand), ({"short": 4}, operand),
             ({"missing": 0}, operand), ({"missing": 3}, operand), ({"missing": 4}, operand),
             ({"ip": (24, 24, 8 | 16 | 32), "lens": head, "outp": head_out, "short": 9}, operand),
             ({"ip": (24, 24, 8 | 16 | 32), "lens": head, "outp": head_out, "short": 7}, operand),
             ({"ip": (24, 24, 8 | 16 | 32), "lens": head, "outp": head_out, "missing": 8}, operand),
             ({"ip": (12, 96, 3 | 64)}, operand),    # compose first without the lateral matrix and its scales
             ({"op": 1, "ip": (24, 7), "lens": cls, "outp": {0: (9 * 80 + 64) * 24}, "short": 4}, operand),
             ({"out_short": 0}, output), ({"out_short": 1}, output), ({"outp": {0: (80 + 64) * 24}}, output),
             ({"op": 3, "lens": {0: 80 * 24, 1: 2304, 2: 24, 3: 96, 4: 1}, "outp": {0: 16 * 80 + 64}}, output)]
    lib.rt_last_error.restype = C.c_char_p
    for kw, why in cases:
        assert _fpn(lib, **kw) == RT_ERR_INVALID, kw
        assert why in lib.rt_last_error(None).decode(), (kw, lib.rt_last_error(None))


def _cls(lib, s=None, n=2, H=3, W=16, cin=8, mid=16, cout=8, k=3, sh=1, act=1, se=1, form=1, null=None, info=True):
    """a 3 x 16 block with squeeze-excite on two crops, unless the arguments say otherwise; null = the name of a NULL operand"""
    a = lambda *shape: np.zeros([max(v, 1) for v in shape], np.float32)   # noqa: E731
    arr = {"x": a(n * H * W, cin), "exp_w": a(mid, cin), "exp_b": a(mid), "dw_w": a(mid, 5, 5), "dw_b": a(mid), "fc1_w": a(mid, mid),
           "fc1_b": a(mid), "fc2_w": a(mid, mid), "fc2_b": a(mid), "lin_w": a(cout, mid), "lin_b": a(cout), "out": a(n * H * W + 64, cout)}
    p = {k_: (None if k_ == null else v.ctypes.data) for k_, v in arr.items()}
    return lib.rt_debug_cls_block(s, p["x"], n, H, W, cin, mid, cout, k, sh, act, se, p["exp_w"], p["exp_b"], p["dw_w"], p["dw_b"], p["fc1_w"],
                                  p["fc1_b"], p["fc2_w"], p["fc2_b"], p["lin_w"], p["lin_b"], form, p["out"], (C.c_int * 4)() if info else None)


def _stem(lib, s=None, x4=True, rgb=False, hs=(3, 1), ws=(2, 1), hh=True, ww=True, n_img=2, cout=16, w=True, b=True, act=0, mean=True,
          std=(0.5, 0.5, 0.5), out=True, out_len=None):
    """the rec stem on two images of 6 and 1 pixels (outputs 2 x 1 and 1 x 1), unless the arguments say otherwise"""
    h, wd = np.array(hs, np.int32), np.array(ws, np.int32)
    xs, px, wt, bs, o = np.zeros((7, 4), np.float32), np.zeros((7, 3), np.uint8), np.zeros((16, 27), np.float32), np.zeros(16, np.float32), np.zeros((3 + 64) * 16, np.float32)
    m, sd = np.full(3, 0.5, np.float32), np.array(std, np.float32)
    p = lambda arr, on: arr.ctypes.data if on else None   # noqa: E731
    return lib.rt_debug_stem(s, p(xs, x4), p(px, rgb), p(h, hh), p(wd, ww), n_img, cout, p(wt, w), p(bs, b), act, 1 / 255.0, p(m, mean),
                             p(sd, True), p(o, out), (3 + 64) * max(cout, 1) if out_len is None else out_len)


def _glue32(lib, s=None, op=0, ip=(8, 2, 0, 1), fpv=(0.2,), hs=(3, 1), ws=(2, 1), hh=True, ww=True, n_img=2, ipp=True, fpp=True, x=True,
            x_len=None, w=True, w_null=None, out=True, out_len=None, out2=True, out2_len=None, idx=True):
    """se_scale at C = 8 applied in place on two images of 6 and 1 pixels, unless the arguments say otherwise"""
    i = np.zeros(8, np.int32); i[:len(ip)] = ip   # noqa: E702
    f = np.zeros(4, np.float32); f[:len(fpv)] = fpv   # noqa: E702
    h, wd = np.array(hs, np.int32), np.array(ws, np.int32)
    xs, o, o2, ix = np.zeros(1 << 16, np.float32), np.zeros(1 << 16, np.float32), np.zeros(1 << 16, np.float32), np.zeros(1 << 12, np.int32)
    wts = [np.zeros(64, np.float32) for _ in range(4)]
    wp = (C.c_void_p * 4)(*[None if k == w_null else a.ctypes.data for k, a in enumerate(wts)])
    p = lambda arr, on: arr.ctypes.data if on else None   # noqa: E731
    d = lambda v, dflt: dflt if v is None else v          # noqa: E731
    return lib.rt_debug_glue32(s, op, p(i, ipp), p(f, fpp), p(h, hh), p(wd, ww), n_img, p(xs, x), d(x_len, 7 * 8), wp if w else None,
                               p(o, out), d(out_len, (2 + 64) * 8), p(o2, out2), d(out2_len, (7 + 64) * 8), p(ix, idx))


def test_cls_kernel_entries_reject_null_and_bad_arguments_without_a_device():
    """rt_debug_cls_block, rt_debug_stem and rt_debug_glue32 look at their session last, so every argument check answers with its
    own message (rt_last_error(NULL) holds it): a check that was skipped would show as a null session"""
    lib = _lib.load()
    lib.rt_last_error.restype = C.c_char_p

    def run(fn, cases):
        for kw, why in cases:
            assert fn(lib, **kw) == RT_ERR_INVALID, kw
            assert why in lib.rt_last_error(None).decode(), (kw, lib.rt_last_error(None))

    null, se, crops, chan, block = "null argument", "needs both FCs", "bad crop count or extents", "multiples of 4", "no such block"
    run(_cls, [({}, "null session"), ({"se": 0, "null": "fc1_w"}, "null session"), ({"form": 0, "W": 24}, "null session")] +
        [({"null": k}, null) for k in ("x", "exp_w", "exp_b", "dw_w", "dw_b", "lin_w", "lin_b", "out")] + [({"info": False}, null)] +
        [({"null": k}, se) for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b")] + [({"se": 2}, se)] +
        [({"n": 0}, crops), ({"H": 0}, crops), ({"W": 0}, crops), ({"W": 5000}, crops),
         ({"cin": 0}, chan), ({"cin": 6}, chan), ({"cin": 68}, chan), ({"cout": 0}, chan), ({"cout": 10}, chan), ({"mid": 0}, chan), ({"mid": 18}, chan),
         ({"mid": 1028}, chan), ({"k": 4}, block), ({"k": 7}, block), ({"sh": 0}, block), ({"sh": 3}, block), ({"act": 0}, block), ({"act": 3}, block),
         ({"form": 2}, block), ({"form": -1}, block), ({"n": 4096, "H": 4096, "W": 16}, "too large")])
    null, count, pages, img, length = "null argument", "bad image count, activation or cout", "pages need", "empty or oversized image", "out has the wrong length"
    run(_stem, [({}, "null session"), ({"cout": 8, "act": 2, "out_len": (3 + 64) * 8}, "null session"), ({"x4": False, "rgb": True}, "null session"),
                ({"x4": False}, null), ({"rgb": True}, null), ({"hh": False}, null), ({"ww": False}, null), ({"w": False}, null), ({"b": False}, null),
                ({"out": False}, null), ({"n_img": 0}, count), ({"cout": 4}, count), ({"cout": 32}, count), ({"act": 5}, count), ({"act": -1}, count),
                ({"x4": False, "rgb": True, "cout": 8}, count), ({"x4": False, "rgb": True, "mean": False}, pages),
                ({"x4": False, "rgb": True, "std": (0.5, 0.0, 0.5)}, pages), ({"hs": (3, 0)}, img), ({"ws": (5000, 1)}, img),
                ({"out_len": (3 + 64) * 16 - 1}, length), ({"out_len": 0}, length)])
    null, opn, geom, img, chan, params, lens, second = (
        "null argument", "bad op or image / row count", "null geometry", "empty or oversized image", "bad channel count", "bad parameters for the op",
        "x is too short or out has the wrong length", "out2 is missing or has the wrong length")
    soft = {"op": 4, "ip": (2, 4), "x_len": 2 * 4, "out_len": (2 + 64) * 2, "hh": False, "ww": False}
    amax = {"op": 6, "ip": (5, 8), "x_len": 2 * 8, "out_len": 2 + 64}
    run(_glue32, [({}, "null session"), (soft, "null session"), (amax, "null session"), ({"ip": (8, 2, 1, 0), "out2": False}, "null session"),
                  ({"op": 3, "ip": (8, 16), "hs": (3, 6), "ws": (2, 5), "x_len": 36 * 8, "out_len": (5 + 64) * 16}, "null session"),
                  ({"ipp": False}, null), ({"fpp": False}, null), ({"x": False}, null), ({"out": False}, null),
                  ({"op": -1}, opn), ({"op": 7}, opn), ({"n_img": 0}, opn), ({"hh": False}, geom), ({"ww": False}, geom),
                  ({"hs": (3, 0)}, img), ({"ws": (0, 1)}, img), ({"ip": (0, 2, 0, 1)}, chan),
                  ({"ip": (6, 2, 0, 1)}, params), ({"ip": (8, 0, 0, 1)}, params), ({"ip": (8, 2, 2, 1)}, params), ({"ip": (8, 2, 0, 2)}, params),
                  ({"fpv": (0.0,)}, params), ({"w": False}, params), ({"w_null": 2}, params),
                  ({"op": 1, "ip": (6,)}, params),
                  ({"op": 2, "ip": (8,)}, params),                                   # maxpool_2x2: an image below the window
                  ({"op": 3, "ip": (8, 16), "hs": (2, 3), "ws": (2, 2)}, params),   # avgpool_3x2: an image below the window
                  ({"op": 3, "ip": (8, 4), "hs": (3, 3), "ws": (2, 2)}, params),    # avgpool_3x2: ldy below Cp
                  ({"op": 3, "ip": (8, 18), "hs": (3, 3), "ws": (2, 2)}, params),   # avgpool_3x2: ldy no multiple of 4
                  (dict(soft, ip=(5, 4)), params),                                   # softmax_rows: ld below C
                  (dict(amax, idx=False), params),                                   # argmax_rows without idx_out
                  ({"x_len": 7 * 8 - 1}, lens), ({"out_len": (2 + 64) * 8 - 1}, lens), ({"out_len": 0}, lens),
                  (dict(soft, x_len=7), lens), (dict(amax, out_len=2 + 63), lens),
                  ({"out2": False}, second), ({"out2_len": (7 + 64) * 8 - 1}, second)])


def _wide(lib, s=None, hs=(3, 2), ws=(5, 1), n_img=2, K=5, cin=192, cout=384, sh=1, sw=1, dw_act=2, se=1, form=1, null=None, info=True,
          out_len=None, y1_len=None, scale_len=None):
    """a 5x5 192 -> 384 block with squeeze-excite on two images of 15 and 2 pixels, unless the arguments say otherwise; null = the
    name of a NULL operand"""
    a = lambda *shape: np.zeros([max(v, 1) for v in shape], np.float32)   # noqa: E731
    arr = {"x": a(17, 512), "hs": np.array(hs, np.int32), "ws": np.array(ws, np.int32), "dw_w": a(cin, 5, 5), "dw_b": a(cin), "pw_w": a(cout, cin),
           "pw_b": a(cout), "fc1_w": a(cin, cin), "fc1_b": a(cin), "fc2_w": a(cin, cin), "fc2_b": a(cin), "out": a(17 + 64, 1024),
           "y1": a(17 + 64, 512), "scale": a(2 + 64, 512)}
    p = {k_: (None if k_ == null or (not se and k_.startswith(("fc", "scale"))) else v.ctypes.data) for k_, v in arr.items()}
    pitch = lambda c: (c + 31) // 32 * 32 if c >= 128 else (c + 3) // 4 * 4   # noqa: E731
    d = lambda v, dflt: dflt if v is None else v                             # noqa: E731
    return lib.rt_debug_lc_wide(s, p["x"], p["hs"], p["ws"], n_img, K, cin, cout, sh, sw, p["dw_w"], p["dw_b"], p["pw_w"], p["pw_b"], dw_act, 1,
                                1.3, 0.07, 1, 0.8, -0.05, p["fc1_w"], p["fc1_b"], p["fc2_w"], p["fc2_b"], form, p["out"],
                                d(out_len, (17 + 64) * pitch(max(cout, 1))), p["y1"], d(y1_len, (17 + 64) * pitch(max(cin, 1))), p["scale"],
                                d(scale_len, (2 + 64) * pitch(max(cin, 1)) if se else 0), (C.c_int * 16)() if info else None)


def test_dw_kernel_entries_reject_null_and_bad_arguments_without_a_device():
    """rt_debug_lc_wide looks at its session last, so every argument check answers with its own message (rt_last_error(NULL) holds
    it); rt_debug_dw_plan takes no session at all and answers on the host"""
    lib = _lib.load()
    lib.rt_last_error.restype = C.c_char_p
    null, se, count, chan, block, img, lens, slen = (
        "null argument", "needs both FCs and scale_out", "bad image count", "bad channel counts", "no such block", "empty or oversized image",
        "out or y1_out has the wrong length", "scale_out has the wrong length")
    cases = ([({}, "null session"), ({"se": 0}, "null session"), ({"K": 3, "cin": 96, "cout": 96, "form": 0}, "null session"),
              ({"sh": 2, "sw": 2, "hs": (6, 4), "ws": (5, 2), "out_len": (11 + 64) * 384, "y1_len": (11 + 64) * 192}, "null session")] +
             [({"null": k}, null) for k in ("x", "hs", "ws", "dw_w", "dw_b", "pw_w", "pw_b", "out", "y1")] + [({"info": False}, null)] +
             [({"null": k}, se) for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "scale")] +
             [({"n_img": 0}, count), ({"n_img": 5000}, count), ({"cin": 0}, chan), ({"cin": 190}, chan), ({"cin": 516}, chan), ({"cout": 0}, chan),
              ({"cout": 964}, chan), ({"K": 4}, block), ({"K": 7}, block), ({"sh": 0}, block), ({"sw": 3}, block), ({"dw_act": 9}, block),
              ({"form": 2}, block), ({"form": -1}, block), ({"hs": (3, 0)}, img), ({"ws": (0, 1)}, img), ({"hs": (5000, 2)}, img),
              ({"out_len": (17 + 64) * 384 - 1}, lens), ({"y1_len": 0}, lens), ({"scale_len": 0}, slen), ({"se": 0, "scale_len": 4}, slen)])
    for kw, why in cases:
        assert _wide(lib, **kw) == RT_ERR_INVALID, kw
        assert why in lib.rt_last_error(None).decode(), (kw, lib.rt_last_error(None))
    plan = (C.c_int * 8)()
    for args, why in (((5, 1, 1, 256, 12, 100, 0, 1, None), "null argument"), ((5, 1, 1, 250, 12, 100, 0, 1, plan), "bad shape"),
                      ((5, 1, 1, 256, 0, 100, 0, 1, plan), "bad shape"), ((5, 1, 1, 256, 12, 100, 0, 2, plan), "bad shape")):
        assert lib.rt_debug_dw_plan(*args) == RT_ERR_INVALID, args
        assert why in lib.rt_last_error(None).decode(), args
    # the plan itself, on the host: the rec net's 12-row 5x5 layer as the sweep and as row strips, and a kernel size without an instance
    assert lib.rt_debug_dw_plan(5, 1, 1, 256, 12, 800, 0, 1, plan) == 0 and tuple(plan) == (3, 1, 4, 16, 16, 38, 13, 4)
    assert lib.rt_debug_dw_plan(5, 1, 1, 256, 12, 800, 0, 0, plan) == 0 and tuple(plan) == (2, 17093, 4, 16, 16, 38, 38, 4)
    assert lib.rt_debug_dw_plan(7, 1, 1, 256, 12, 800, 0, 1, plan) == 0 and tuple(plan)[:2] == (0, 0)
