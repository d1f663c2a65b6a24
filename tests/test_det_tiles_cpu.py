"""Det tiles (retto_amd/csrc/det_tiles.h) on the CPU: rt_det_tile_plan against the independent Python rule (det_tiles_ref) over a
grid of lengths, tiles and overlaps, the plan's properties, known answers, refusals, the capacity limit, the CLI flags, the
exported symbols, and the same grid through a stand-alone driver built with AddressSanitizer + UBSan (run as a program; nothing
is loaded into Python under a sanitizer).  No GPU."""
import os
import subprocess

import pytest

import retto_amd
from retto_amd import _lib, cli

import det_tiles_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = 8, 9
MAX_PIXELS = 268434432   # RT_DET_MAX_PIXELS


def grid():
    """L in 32 .. 4096, every accepted T up to L (a T beyond L is one tile whatever its value: L + 32 stands for them), every
    accepted O up to 512"""
    for L in range(32, 4096 + 1, 32):
        for T in list(range(64, L + 1, 32)) + [max(L + 32, 64)]:
            for O in range(0, min(512, T // 2) + 1, 32):
                yield L, T, O


def axis_of(L, T, O):
    """rt_det_tile_plan's plan along a column axis of length L (the row axis is 32 long: one tile)"""
    p = retto_amd.det_tile_plan(32, L, T, O)
    assert p["row_origins"] == [0] and p["row_bounds"] == [32] and p["tile_h"] == 32
    return p["tile_w"], p["col_origins"], p["col_bounds"]


def test_plan_equals_the_python_rule_over_the_grid():
    n = 0
    for L, T, O in grid():
        got = axis_of(L, T, O)
        assert got == TR.axis_plan(L, T, O), (L, T, O, got)
        TR.check_axis(L, T, O, *got)
        n += 1
    assert n > 100000
    # both axes at once, rows and columns apart
    for H, W, T, O in [(160, 224, 96, 32), (736, 800, 384, 64), (1184, 736, 384, 64), (64, 224, 96, 32), (224, 96, 96, 32), (320, 416, 384, 64), (320, 384, 384, 64)]:
        assert retto_amd.det_tile_plan(H, W, T, O) == TR.page_plan(H, W, T, O), (H, W, T, O)


def test_known_answers():
    assert axis_of(224, 96, 32) == (96, [0, 64, 128], [80, 144, 224])
    assert axis_of(800, 384, 64) == (384, [0, 320, 416], [352, 560, 800])   # the last pair overlaps by 288 > 64
    assert axis_of(384, 384, 64) == (384, [0], [384])                       # L = T
    assert axis_of(320, 384, 64) == (320, [0], [320])                       # L < T: one tile, shorter than T
    assert axis_of(256, 64, 0) == (64, [0, 64, 128, 192], [64, 128, 192, 256])   # O = 0: bounds at the tile edges
    assert axis_of(224, 0, 64) == (224, [0], [224])                         # off
    p = retto_amd.det_tile_plan(160, 224, 96, 32)
    assert (len(p["row_origins"]), len(p["col_origins"])) == (2, 3) and p["row_origins"] == [0, 64] and p["row_bounds"] == [80, 160]
    p = retto_amd.det_tile_plan(736, 800, 384, 64)
    assert (len(p["row_origins"]), len(p["col_origins"])) == (3, 3) and p["row_origins"] == [0, 320, 352]


@pytest.mark.parametrize("T,O,word", [(48, 0, "tile"), (32, 0, "tile"), (-64, 0, "tile"), (96, 48, "overlap"), (96, 64, "overlap"),
                                      (128, 96, "overlap"), (96, -32, "overlap"), (0, -32, "overlap")])
def test_refusals_name_the_argument(T, O, word):
    assert not TR.accepted(T, O)
    with pytest.raises(retto_amd.InvalidArgument) as e:
        retto_amd.det_tile_plan(160, 224, T, O)
    assert word in str(e.value) and "rt_det_tile_plan" in str(e.value), str(e.value)


def test_bad_pages_and_the_capacity_limit():
    for h, w in [(0, 32), (32, -32), (48, 64), (64, 100)]:
        with pytest.raises(retto_amd.InvalidArgument) as e:
            retto_amd.det_tile_plan(h, w, 96, 32)
        assert "multiples of 32" in str(e.value)
    assert 8192 * 32768 > MAX_PIXELS >= 8192 * 32736
    p = retto_amd.det_tile_plan(8192, 32736, 960, 64)        # the largest page of this shape that passes
    assert len(p["row_origins"]) == 10 and len(p["col_origins"]) == 37
    for T in (0, 960):                                        # tiled or not: DB post-processing reads the whole map
        with pytest.raises(retto_amd.CapacityError) as e:
            retto_amd.det_tile_plan(8192, 32768, T, 64)
        assert str(MAX_PIXELS) in str(e.value)
    # a small row_cap: the counts are still reported
    import ctypes as C
    lib = _lib.load()
    nr, nc = C.c_int(), C.c_int()
    buf = (C.c_int32 * 2)()
    assert lib.rt_det_tile_plan(160, 224, 96, 32, buf, None, 2, buf, None, 2, C.byref(nr), C.byref(nc), None, None) == INVALID
    assert (nr.value, nc.value) == (2, 3) and b"col_cap" in lib.rt_last_error(None)
    assert lib.rt_det_tile_plan(160, 224, 96, 32, None, None, 0, None, None, 0, C.byref(nr), C.byref(nc), None, None) == 0


def test_cli_flags_parse_and_default_to_off():
    a = cli.build_parser().parse_args(["-i", "pages"])
    assert a.det_tile == 0 and a.det_tile_overlap == 64
    a = cli.build_parser().parse_args(["-i", "pages", "--det-tile", "960", "--det-tile-overlap", "128"])
    assert (a.det_tile, a.det_tile_overlap) == (960, 128)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for name in ("rt_set_det_tiles", "rt_det_tiles", "rt_det_tile_plan", "rt_debug_det_tiles"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert "RT_API int %s(" % name in header, name
    assert "#define RT_DET_MAX_PIXELS %d" % MAX_PIXELS in header
    assert hasattr(retto_amd.RettoSession, "set_det_tiles") and isinstance(retto_amd.RettoSession.det_tiles, property)
    assert hasattr(retto_amd.RettoSession, "debug_det_tiles")


# ---- the stand-alone driver under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("det_tiles") / "det_tiles_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), os.path.join(ROOT, "tests", "native", "det_tiles_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the det tiles driver does not build:\n" + r.stderr[-3000:]
    return exe


def test_driver_answers_the_grid_under_the_sanitizers(driver):
    queries, want = [], []
    for L, T, O in grid():
        tlen, xs, bs = TR.axis_plan(L, T, O)
        queries.append("%d %d %d" % (L, T, O))
        want.append("n=%d len=%d x=%s b=%s" % (len(xs), tlen, ",".join(map(str, xs)), ",".join(map(str, bs))))
    for (T, O), word in [((48, 0), "tile"), ((32, 0), "tile"), ((96, 48), "overlap"), ((96, 64), "overlap"), ((-64, 0), "tile"), ((96, -32), "overlap")]:
        queries.append("224 %d %d" % (T, O)); want.append(word)
    queries += ["page 8192 32736 960 64", "page 8192 32768 960 64", "page 8192 32768 0 0", "page 320 384 384 64", "page 320 416 384 64", "page 48 64 96 32",
                "page 2147483616 2147483616 960 64"]
    want += ["page: 0 tiled=1", "page: %d tiled=0" % CAPACITY, "page: %d tiled=0" % CAPACITY, "page: 0 tiled=0", "page: 0 tiled=1", "page: %d tiled=0" % INVALID,
             "page: %d tiled=0" % CAPACITY]
    r = subprocess.run([driver], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for q, g, w in zip(queries, got, want):
        if w in ("tile", "overlap"):
            assert g.startswith("invalid: ") and w in g, (q, g)
        else:
            assert g == w, (q, g, w)
