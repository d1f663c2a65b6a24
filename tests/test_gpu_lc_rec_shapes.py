"""Regression guard for the existing fused thin-block kernel (k_lc_lds, the production form 3 of rt_bench_lc) at the three
blocks the recognition net runs on its 24- and 12-row maps: 64 -> 64 and 32 -> 64 at stride 1, 64 -> 128 at stride (2, 1).
Nothing here is a new kernel form -- the kernel re-reads its vertical halo rows as before (docs/HISTORY.md: the tile-order
experiment) -- the existing bit-identity test only reaches these blocks at det-net sizes.  One launch each: three images,
widths that are and are not a multiple of the 16-pixel tile and span more than one workgroup.  rt_bench_lc compares with the
reference form (k_lc_thin or, where that has no instance, the unfused depthwise + GEMM pair): the arithmetic order per pixel
is the same, so the bar is max |diff| = 0.0."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

BLOCKS = [(64, 64, 1), (32, 64, 1), (64, 128, 21)]   # s3.1, s3.0, s4.0 (21 = stride (2, 1))


@pytest.mark.parametrize("cin,cout,stride", BLOCKS)
@pytest.mark.parametrize("h", [24, 12])
@pytest.mark.parametrize("w", [40, 203])
def test_rec_thin_blocks_equal_the_reference_form(hip_session, cin, cout, stride, h, w):
    form = 3   # k_lc_lds, the production form
    lib, hd = hip_session._hd.lib, hip_session._hd.h
    lib.rt_bench_lc.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    ms, md = C.c_float(), C.c_float(-1.0)
    rc = lib.rt_bench_lc(hd, 3, h, w, cin, cout, stride, form, 1, C.byref(ms), C.byref(md))
    assert rc == 0, lib.rt_last_error(hd)
    assert md.value == 0.0, f"{cin}->{cout} /{stride} form {form} on 3 x {h} x {w}: max |diff| {md.value}"
