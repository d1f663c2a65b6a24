"""Rec flip (retto_amd/csrc/rec_flip.h) on the CPU: rt_rec_flip_choose against the numpy restatement (rec_flip_ref) over a grid
that covers zero tokens on either side, ties, NaNs and one-ulp neighbours; the restatement against two mutants; the score
restatement on known rows; the exported symbols, the refusals that need no device, the CLI flag; and the rule and the flat rotate
index arithmetic through a stand-alone driver built with AddressSanitizer + UBSan (run as a program; nothing is loaded into
Python under a sanitizer).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, cli

import rec_flip_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 8


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_choose_equals_the_numpy_rule_over_the_grid():
    lib = _lib.load()
    grid = FR.grid()
    assert len(grid) == 765
    taken = 0
    for n0, s0, n1, s1 in grid:
        got = lib.rt_rec_flip_choose(n0, C.c_float(float(s0)), n1, C.c_float(float(s1)))
        assert got == FR.choose(n0, s0, n1, s1), (n0, s0, n1, s1, got)
        taken += got
    assert 0 < taken < len(grid)
    # the cases the rule names
    one = np.float32(0.5); up = np.nextafter(one, np.float32(1), dtype=np.float32); dn = np.nextafter(one, np.float32(0), dtype=np.float32)
    nan = float("nan")
    ch = lambda *a: lib.rt_rec_flip_choose(a[0], C.c_float(float(a[1])), a[2], C.c_float(float(a[3])))
    assert ch(3, one, 3, one) == 0            # a tie keeps view 0
    assert ch(3, one, 3, up) == 1 and ch(3, one, 3, dn) == 0
    assert ch(3, nan, 3, one) == 0 and ch(3, one, 3, nan) == 0 and ch(3, nan, 3, nan) == 0   # a NaN keeps view 0
    assert ch(0, nan, 3, 0.1) == 1            # view 0 kept nothing
    assert ch(3, 0.1, 0, nan) == 0 and ch(0, nan, 0, nan) == 0   # view 1 kept nothing
    assert ch(0, 0.9, 1, 0.1) == 1 and ch(1, 0.1, 0, 0.9) == 0    # the counts come before the scores


def test_the_restatement_tells_the_mutants():
    grid = FR.grid()
    rule = [FR.choose(*g) for g in grid]
    ge = [FR.choose_ge(*g) for g in grid]
    blind = [FR.choose_ignores_ntok(*g) for g in grid]
    ties = [i for i, (n0, s0, n1, s1) in enumerate(grid) if n0 > 0 and n1 > 0 and s0 == s1]
    assert ties and all(rule[i] == 0 and ge[i] == 1 for i in ties)
    assert [i for i in range(len(grid)) if rule[i] != ge[i]] == ties          # the >= mutant differs exactly on the ties
    diff = [i for i in range(len(grid)) if rule[i] != blind[i]]
    assert diff and all(grid[i][0] <= 0 or grid[i][2] <= 0 for i in diff)     # the blind mutant differs only where a view kept nothing
    assert any(rule[i] == 1 for i in diff) and any(rule[i] == 0 for i in diff)


def test_score_restatement_on_known_rows():
    idx = np.array([0, 5, 5, 0, 5, 7, 7, 0], np.int32)
    prob = np.array([0.9, 0.5, 0.6, 0.9, 0.25, 0.125, 0.7, 0.9], np.float32)
    n, s = FR.score(idx, prob)   # kept: steps 1, 4, 5
    assert n == 3 and s.tobytes() == np.float32(np.float32(np.float32(np.float32(0.5) + np.float32(0.25)) + np.float32(0.125)) / np.float32(3)).tobytes()
    n, s = FR.score(np.zeros(5, np.int32), np.ones(5, np.float32))
    assert n == 0 and np.isnan(s)
    # sequential fp32 in step order, not a pairwise or fp64 sum
    prob = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], np.float32)
    n, s = FR.score(np.array([1, 2, 3, 4]), prob)
    assert n == 4 and s == np.float32(0.25)   # each tiny addend is rounded away in turn
    assert FR.both_ways(0.7, 0.9) and not FR.both_ways(0.9, 0.9) and FR.both_ways(1.0, 2.0) and not FR.both_ways(0.1, 0.0)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for name in ("rt_set_rec_flip", "rt_rec_flip", "rt_rec_flip_choose", "rt_results_rec_flip", "rt_debug_rec_flip"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert "RT_API int %s(" % name in header, name
    assert "NOT been measured" in header[header.index("rt_set_rec_flip") - 4000:header.index("rt_set_rec_flip")]
    assert hasattr(retto_amd.RettoSession, "set_rec_flip") and isinstance(retto_amd.RettoSession.rec_flip, property)
    assert hasattr(retto_amd.RettoSession, "debug_rec_flip")
    assert retto_amd.RecProcessorSingleResult("", 0.0).flip is None
    f = retto_amd.RecFlip(2, 0.25, 0.5)
    assert (f.outcome, f.score0, f.score1) == (2, 0.25, 0.5)


def test_null_and_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.rt_set_rec_flip(None, 0.5) == INVALID and b"rt_set_rec_flip" in lib.rt_last_error(None)
    assert lib.rt_rec_flip(None, None) == INVALID
    s0, s1 = C.c_float(-3.0), C.c_float(-4.0)
    assert lib.rt_results_rec_flip(None, 0, 0, C.byref(s0), C.byref(s1)) == 0 and (s0.value, s1.value) == (-3.0, -4.0)
    crop = np.zeros((4, 8, 3), np.uint8); hw = np.array([4, 8], np.int32); both = np.array([1], np.uint8)
    args = [crop.ctypes.data, hw.ctypes.data, 1, both.ctypes.data, 6.5] + [None] * 9
    assert lib.rt_debug_rec_flip(None, *args) == INVALID and b"rt_debug_rec_flip" in lib.rt_last_error(None)


def test_cli_flag_parses_and_defaults_to_off():
    a = cli.build_parser().parse_args(["-i", "pages"])
    assert a.rec_flip == 0.0
    a = cli.build_parser().parse_args(["-i", "pages", "--rec-flip", "0.95"])
    assert a.rec_flip == 0.95


# ---- the stand-alone driver under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec_flip") / "rec_flip_driver")
    src = os.path.join(ROOT, "tests", "native", "rec_flip_driver.cpp")
    includes = [l.strip() for l in open(src) if l.startswith("#include \"")]
    assert includes == ['#include "rec_flip.h"'], includes   # the header needs nothing of HIP
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the rec flip driver does not build:\n" + r.stderr[-3000:]
    return exe


ROTATE_CASES = [[(1, 1)], [(48, 320)], [(9, 40), (64, 500), (17, 333), (1, 7), (7, 1)], [(30, 200), (48, 96), (2, 2), (3, 5)]]


def test_driver_answers_under_the_sanitizers(driver):
    queries, want = [], []
    for n0, s0, n1, s1 in FR.grid():
        queries.append("c %d %08x %d %08x" % (n0, _bits(s0), n1, _bits(s1))); want.append(str(FR.choose(n0, s0, n1, s1)))
    for sc, below in [(0.7, 0.9), (0.9, 0.9), (0.95, 0.9), (1.0, 1.0), (1.0, 1.5), (0.3, 0.0), (float("nan"), 0.5), (float("nan"), 2.0)]:
        queries.append("b %08x %08x" % (_bits(sc), _bits(below)))
        every = np.float32(below) > 1
        want.append("both=%d every=%d needs=%d" % (FR.both_ways(sc, below), every, np.float32(below) > 0 and not every))
    for below, word in [(float("nan"), "NaN"), (-1.0, "negative"), (float("inf"), "infinite"), (-float("inf"), "negative")]:
        queries.append("b %08x %08x" % (_bits(0.5), _bits(below))); want.append("invalid: cls_below is " + word)
    for sizes in ROTATE_CASES:
        queries.append("r %d %s" % (len(sizes), " ".join("%d %d" % s for s in sizes)))
        flipped = b"".join(FR.rotate180(c).tobytes() for c in FR.pattern_crops(sizes))
        want.append("%016x" % FR.fnv1a(flipped))
    r = subprocess.run([driver], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for q, g, w in zip(queries, got, want):
        assert g == w, (q, g, w)
