"""Rec windows (retto_amd/csrc/rec_windows.h) on the CPU: rt_rec_window_plan against the independent Python rule
(rec_windows_ref) over a grid of windows, overlaps and line widths, the plan's properties, the known answers, refusals, the CLI
flags, the exported symbols, and the same grid through a stand-alone driver built with AddressSanitizer + UBSan (run as a
program; nothing is loaded into Python under a sanitizer).  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import retto_amd
from retto_amd import _lib, cli

import rec_windows_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 8

# L, window, overlap -> origins, widths, bounds, T
KNOWN = [
    ((487, 128, 32), ([0, 96, 192, 288, 352], [128, 128, 128, 128, 135], [14, 26, 38, 48, 61], 61)),
    ((330, 128, 64), ([0, 64, 128, 192, 200], [128, 128, 128, 128, 130], [12, 20, 28, 32, 41], 41)),
    ((656, 256, 64), ([0, 192, 384, 400], [256, 256, 256, 256], [28, 52, 65, 82], 82)),
    ((200, 128, 0), ([0, 72], [128, 128], [12, 25], 25)),
    ((135, 128, 32), ([0], [135], [17], 17)),   # whole: last = 0
]


def grid():
    """every window 128 .. 704, every legal overlap, every L in 8 .. 2199"""
    for W in range(128, 704 + 1, 32):
        for O in range(0, W // 2 + 1, 32):
            for L in range(8, 2200):
                yield L, W, O


def plan_of(L, W, O):
    p = retto_amd.rec_window_plan(L, W, O)
    return p["origins"], p["widths"], p["bounds"], p["T"]


def test_plan_equals_the_python_rule_over_the_grid():
    n = 0
    for L, W, O in grid():
        got = plan_of(L, W, O)
        assert got == WR.plan(L, W, O), (L, W, O, got)
        WR.check(L, W, O, *got)
        n += 1
    assert n > 250000
    for L in (8, 9, 127, 128, 3000):   # off: one unit whatever the width, the overlap kept and not read
        assert plan_of(L, 0, 0) == ([0], [L], [WR.tokens(L)], WR.tokens(L))
        assert plan_of(L, 0, 48) == plan_of(L, 0, 0)


def test_known_answers():
    for (L, W, O), want in KNOWN:
        assert plan_of(L, W, O) == want, (L, W, O)
        assert WR.plan(L, W, O) == want, (L, W, O)
    # every L < window + 8 is whole; window + 8 is the first windowed width
    assert all(len(plan_of(L, 128, 32)[0]) == 1 for L in range(8, 136))
    assert plan_of(136, 128, 32) == ([0, 8], [128, 128], [8, 17], 17)
    # the time steps are the rec network's: a trailing partial step of up to 4 columns is dropped
    assert [WR.tokens(L) for L in (8, 12, 13, 16, 320, 324, 325)] == [1, 1, 2, 2, 40, 40, 41]


def test_last_unit_ends_at_T_and_the_intervals_partition_the_steps():
    for L, W, O in [(487, 128, 32), (330, 128, 64), (656, 256, 64), (200, 128, 0), (3077, 640, 128), (2199, 704, 352), (1300, 320, 64)]:
        xs, ws, cs, T = plan_of(L, W, O)
        assert xs[-1] // 8 + WR.tokens(ws[-1]) == T == WR.tokens(L)
        owners = [WR.owner(cs, t) for t in range(T)]
        assert owners == sorted(owners) and set(owners) == set(range(len(xs)))   # every unit owns a run, every step has one owner
        for t, i in enumerate(owners):
            assert 0 <= t - xs[i] // 8 < WR.tokens(ws[i])                          # at a row the unit has


@pytest.mark.parametrize("W,O,word", [(96, 0, "window"), (130, 0, "window"), (-128, 0, "window"), (128, 48, "overlap"),
                                      (128, 96, "overlap"), (256, 160, "overlap"), (128, -32, "overlap"), (0, -32, "overlap")])
def test_refusals_name_the_parameter(W, O, word):
    assert not WR.accepted(W, O)
    with pytest.raises(retto_amd.InvalidArgument) as e:
        retto_amd.rec_window_plan(487, W, O)
    assert word in str(e.value) and "rt_rec_window_plan" in str(e.value), str(e.value)


def test_bad_lines_and_a_small_cap():
    for L in (0, 7, -8):
        with pytest.raises(retto_amd.InvalidArgument) as e:
            retto_amd.rec_window_plan(L, 128, 32)
        assert "at least 8" in str(e.value)
    lib = _lib.load()
    n, T = C.c_int(), C.c_int()
    buf = (C.c_int32 * 2)()
    assert lib.rt_rec_window_plan(487, 128, 32, buf, None, None, 2, C.byref(n), C.byref(T)) == INVALID   # the counts still written
    assert (n.value, T.value) == (5, 61) and b"cap" in lib.rt_last_error(None)
    assert lib.rt_rec_window_plan(487, 128, 32, None, None, None, 0, C.byref(n), C.byref(T)) == 0 and n.value == 5
    assert lib.rt_rec_windows(None, None, None) == INVALID
    assert lib.rt_results_rec_windows(None, 0, 0) == 0


def test_cli_flags_parse_and_default_to_off():
    a = cli.build_parser().parse_args(["-i", "pages"])
    assert a.rec_window == 0 and a.rec_window_overlap == 0
    a = cli.build_parser().parse_args(["-i", "pages", "--rec-window", "640", "--rec-window-overlap", "128"])
    assert (a.rec_window, a.rec_window_overlap) == (640, 128)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for name in ("rt_set_rec_windows", "rt_rec_windows", "rt_rec_window_plan", "rt_results_rec_windows", "rt_debug_rec_windows"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert "RT_API int %s(" % name in header, name
    assert hasattr(retto_amd.RettoSession, "set_rec_windows") and isinstance(retto_amd.RettoSession.rec_windows, property)
    assert hasattr(retto_amd.RettoSession, "debug_rec_windows") and callable(retto_amd.rec_window_plan)
    assert retto_amd.RecProcessorSingleResult("", 0.0).windows == 1


# ---- the stand-alone driver under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec_windows") / "rec_windows_driver")
    src = os.path.join(ROOT, "tests", "native", "rec_windows_driver.cpp")
    includes = [l.strip() for l in open(src) if l.startswith("#include \"")]
    assert includes == ['#include "rec_windows.h"'], includes   # the header stands alone: no HIP header, nothing else of the project
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the rec windows driver does not build:\n" + r.stderr[-3000:]
    return exe


def test_driver_answers_the_grid_under_the_sanitizers(driver):
    queries, want = [], []
    for L, W, O in grid():
        xs, ws, cs, T = WR.plan(L, W, O)
        queries.append("%d %d %d" % (L, W, O))
        want.append("n=%d T=%d x=%s w=%s c=%s" % (len(xs), T, ",".join(map(str, xs)), ",".join(map(str, ws)), ",".join(map(str, cs))))
    for (W, O), word in [((96, 0), "window"), ((130, 0), "window"), ((-128, 0), "window"), ((128, 48), "overlap"), ((128, 96), "overlap")]:
        queries.append("487 %d %d" % (W, O)); want.append(word)
    queries += ["3000 0 0"]   # off
    want += ["n=1 T=375 x=0 w=3000 c=375"]
    r = subprocess.run([driver], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for q, g, w in zip(queries, got, want):
        if w in ("window", "overlap"):
            assert g.startswith("invalid: ") and w in g, (q, g)
        else:
            assert g == w, (q, g, w)
