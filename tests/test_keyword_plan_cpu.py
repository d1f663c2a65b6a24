"""The keyword part of the rec tail's plan (retto_amd/csrc/rec_tail_plan.h) and the four-kind option rules
(retto_amd/csrc/rec_line_opts.h) without a GPU, through tests/native/keyword_plan_driver.cpp: which lines of a group carry a
list, their rows and table slots, needs_z5, the capacity a group's table has, and how charset / lexicon / pattern / keywords ids
of regions and lines resolve -- the keywords conflict with nothing and are checked last."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("keyword_plan") / "keyword_plan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "retto_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "keyword_plan_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the keyword plan driver does not build:\n" + r.stderr[-3000:]
    return out


def ask(exe, queries):
    r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    out = r.stdout.splitlines()
    assert len(out) == len(queries), out
    return out


T = "5 2 1 3 0 4"
LISTS = "2 10 4 3 300 0 0"   # list 1: 10 entries, 4 + 3 + 3 per bucket: 1 + 2 + 3 waves; list 2: 300 entries of 64 lanes: 300 waves


def test_plan_lists_the_keyword_lines(exe):
    out = ask(exe, ["plan 1 5 0 %s %s 0" % (T, LISTS),                      # no id array: nothing
                    "plan 1 5 0 %s %s 1 0 0 0 0 0" % (T, LISTS),            # every line of list 0: nothing
                    "plan 1 5 0 %s %s 1 2 1 0 1 2" % (T, LISTS),            # lines 1, 3 and the empty line 4 of the group [1, 5)
                    "plan 0 5 0 %s %s 1 2 1 0 1 2" % (T, LISTS),
                    "plan 1 5 2 %s %s 0" % (T, LISTS)])                     # (the candidates alone need z5)
    assert out[0] == out[1] == "rows=8 z5=0 has_kw=0 ktable=0 fits=1 kmax_waves=0 klines=- krows=- other=000"
    assert out[2] == "rows=8 z5=1 has_kw=1 ktable=320 fits=1 kmax_waves=300 klines=0:1:0:1:0,1:0:0:3:10,1:4:1:4:20 krows=0,4,5,6,7 other=000"
    assert out[3] == ("rows=10 z5=1 has_kw=1 ktable=620 fits=1 kmax_waves=300 klines=0:2:1:0:0,2:1:0:1:300,3:0:0:3:310,3:4:1:4:320 "
                      "krows=0,1,2,6,7,8,9 other=000")
    assert out[4].startswith("rows=8 z5=1 has_kw=0")


def test_rows_count_from_the_groups_first_and_waves_follow_the_buckets(exe):
    out = ask(exe, ["plan 2 4 0 %s 1 10 4 3 1 0 0 1 1 0" % T, "plan 0 2 0 2 3 2 2 9 9 0 5 0 5 1 1 2", "plan 0 2 0 2 3 2 1 9 0 9 1 1 1"])
    assert out[0] == "rows=3 z5=1 has_kw=1 ktable=20 fits=1 kmax_waves=6 klines=0:3:0:2:0,3:0:0:3:10 krows=0,1,2 other=000"
    assert "kmax_waves=3 " in out[1] and "ktable=14 " in out[1]     # 9 of 16 lanes: 3 waves; 5 of 32 lanes: 3 waves
    assert "kmax_waves=5 " in out[2] and "ktable=18 " in out[2]     # 9 of 32 lanes: 5 waves


def test_a_groups_table_has_a_capacity(exe):
    """2^26 entries: 1024 lines of a 65536-entry list fit, one more line does not"""
    many = lambda n: "plan 0 %d 0 %d %s 1 65536 0 0 1 %s" % (n, n, " ".join(["1"] * n), " ".join(["1"] * n))
    fits, over = ask(exe, [many(1024), many(1025)])
    assert "ktable=67108864 fits=1" in fits and "ktable=67174400 fits=0" in over


def test_regions_resolve_four_kinds(exe):
    q = ["regions 0 0 0 0 2 2 2 2 2 2 1 0 0 0 0",                                        # nothing given: the defaults (none)
         "regions 1 2 0 2 2 2 2 2 2 2 1 0 0 0 0",                                        # the session defaults
         "regions 1 2 0 2 2 2 2 2 2 2 1 1 0 -1 - 0 0 1 1 -1 0",                          # per region: 0 = none, -1 = default, k = that id
         "regions 1 0 2 1 2 2 2 2 1 2 0 0 0 1 0 -1",                                     # keywords go with a pattern ...
         "regions 1 2 0 1 2 2 2 2 1 2 0 0 0 1 2 1",                                      # ... and with a lexicon
         "regions 0 0 0 0 2 2 2 2 1 2 0 0 0 1 3 0",                                      # an unknown keywords id
         "regions 0 0 0 0 2 2 2 2 1 2 0 0 0 1 0 -2",
         "regions 0 0 0 0 2 2 2 2 2 1 1 0 0 0 1 0 9",                                    # ... names its page and region
         "regions 0 0 0 0 2 2 2 2 1 1 1 9 0 0 1 9",                                      # the charset's error comes first,
         "regions 0 1 0 0 2 2 2 2 1 1 0 0 1 1 1 9",                                      # the pattern / lexicon conflict before the keywords',
         "regions 0 0 0 0 2 2 2 2 2 1 1 1 - 9 0 0 1 9 0"]                                # and page 0's keywords before page 1's charsets
    out = ask(exe, q)
    assert out[0] == "ok 0:0:0:0,0:0:0:0 0:0:0:0"
    assert out[1] == "ok 1:2:0:2,1:2:0:2 1:2:0:2"
    assert out[2] == "ok 0:2:0:1,1:2:0:2 1:2:0:0"
    assert out[3] == "ok 1:0:2:0,1:0:2:1"
    assert out[4] == "ok 1:2:0:2,1:2:0:1"
    assert out[5] == "error: page 0 region 0: unknown keywords id 3"
    assert out[6] == "error: page 0 region 1: unknown keywords id -2"
    assert out[7] == "error: page 1 region 0: unknown keywords id 9"
    assert out[8] == "error: page 0 region 0: unknown charset id 9"
    assert "both a rec pattern (1) and a rec lexicon (1)" in out[9]
    assert out[10] == "error: page 0 region 0: unknown keywords id 9"


def test_lines_expand_four_kinds(exe):
    q = ["lines 0 0 0 2 2 2 2 2 2 2 1 0",                                                # the defaults for every line
         "lines 0 0 0 0 2 2 2 2 2 1 2 1 0 0 0 0 0 1 0 1 1 0 2 2",                        # per-line values; any per kind
         "lines 0 0 0 0 2 2 2 2 1 2 1 0 0 2 1 1 0 0 0",                                  # pattern + keywords on a line: fine
         "lines 0 0 0 3 2 2 2 2 1 1 0",                                                  # an unknown default
         "lines 0 0 0 0 2 2 2 2 1 2 1 0 0 0 0 0 0 0 -1",
         "lines 0 0 0 0 2 2 2 2 1 2 1 0 1 1 9 0 0 0 0",                                  # the conflict comes before the keywords id
         "lines 0 0 0 0 2 2 2 2 1 2 1 9 0 0 9 0 0 0 0"]                                  # and a charset id before both
    out = ask(exe, q)
    assert out[0] == "any=0,0,0,1 lines=0:0:0:2,0:0:0:2,0:0:0:2"
    assert out[1] == "any=1,1,1,1 lines=0:0:0:0,0:1:0:1,1:0:2:2"
    assert out[2] == "any=1,0,1,1 lines=0:0:2:1,1:0:0:0"
    assert out[3] == "error: unknown rec keywords id 3"
    assert out[4] == "error: unknown rec keywords id -1"
    assert out[5] == "error: line 0 carries both a rec pattern and a rec lexicon"
    assert out[6] == "error: unknown rec charset id 9"
