"""The beam part of the rec tail's plan (retto_amd/csrc/rec_tail_plan.h) and the host rule of retto_amd/csrc/ctc_beam.h without
a GPU, through tests/native/beam_plan_driver.cpp, a stand-alone program built with -fsanitize=address,undefined: which lines a
group's beam takes, their rows, trie nodes and token slots, needs_z5, the capacity of a group's trie; bm::line_beams over
exactly sized arrays against the fp64 restatement; bm::check_params."""
import os
import subprocess

import numpy as np
import pytest

import ctc_beam_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("beam_plan") / "beam_plan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), os.path.join(ROOT, "tests", "native", "beam_plan_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the beam plan driver does not build:\n" + r.stderr[-3000:]
    return out


def ask(exe, queries):
    r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(queries), out
    return out


T = "5 2 1 3 0 4"


def test_plan_lists_every_line_of_the_group(exe):
    out = ask(exe, ["plan 1 5 0 %s 0 0" % T,        # off: nothing
                    "plan 1 5 0 %s 4 2" % T,        # lines 1 .. 4 of the call, the empty line 4 included
                    "plan 0 5 0 %s 32 8" % T,
                    "plan 2 3 1 %s 1 1" % T])
    assert out[0] == "rows=8 z5=0 has_beam=0 bnodes=0 fits=1 blines=- brows=- other=0000"
    # nodes: 1 + 4 T per line; token slots: 2 T per line
    assert out[1] == "rows=8 z5=1 has_beam=1 bnodes=36 fits=1 blines=0:1:0:1:0,1:3:5:2:2,4:0:18:3:8,4:4:19:4:8 brows=0,1,2,3,4,5,6,7 other=0000"
    assert out[2] == ("rows=10 z5=1 has_beam=1 bnodes=325 fits=1 blines=0:2:0:0:0,2:1:65:1:16,3:3:98:2:24,6:0:195:3:48,6:4:196:4:48 "
                      "brows=0,1,2,3,4,5,6,7,8,9 other=0000")
    assert out[3] == "rows=3 z5=1 has_beam=1 bnodes=4 fits=1 blines=0:3:0:2:0 brows=0,1,2 other=0000"


def test_a_groups_trie_has_a_capacity(exe):
    """2^26 nodes: 1 + 32 T per line"""
    many = lambda n, t: "plan 0 %d 0 %d %s 32 1" % (n, n, " ".join([str(t)] * n))
    fits, over = ask(exe, [many(2048, 1023), many(2048, 1024)])
    assert "bnodes=%d fits=1" % (2048 * (1 + 32 * 1023)) in fits and "bnodes=%d fits=0" % (2048 * (1 + 32 * 1024)) in over


def test_check_params(exe):
    out = ask(exe, ["check 1 1", "check 32 8", "check 4 4", "check 0 1", "check 33 1", "check 4 0", "check 4 5", "check 32 9"])
    assert out[:3] == ["ok"] * 3
    assert all(o.startswith("error: beam is outside [1, RT_MAX_BEAM (32)]") for o in out[3:5])
    assert all(o.startswith("error: nbest is outside [1, min(beam, RT_MAX_NBEST (8))]") for o in out[5:])


def parse(line):
    parts = line.split()
    n = int(parts[0].split("=")[1])
    hyps = []
    for p in parts[1:]:
        v, s = p.split(":")
        hyps.append((tuple(int(c) for c in s.split(",")) if s else (), float(v)))
    assert len(hyps) == n
    return hyps


def test_host_rule_under_the_sanitizers(exe):
    """random integer logits, exactly sized arrays: N = 2 (one symbol), 3, 9 (all of K_t), 12 (more classes than TOP_C); T = 0, 1
    and up; beams 1, 3, 32.  The strings are the fp64 rule's wherever its own gaps are clear; the logprobs agree."""
    rng = np.random.default_rng(42)
    queries, want = [], []
    for N, T, B, n in ((2, 5, 32, 8), (3, 4, 32, 8), (3, 0, 4, 2), (3, 1, 1, 1), (9, 6, 3, 3), (12, 7, 32, 8), (12, 9, 1, 1), (5, 12, 8, 8)):
        l = rng.integers(-6, 3, (T, N)).astype(np.float64)
        queries.append("beam %d %d %d %d %s" % (N, T, B, n, " ".join(str(int(v)) for v in l.reshape(-1))))
        want.append(BR.beam64(l, B)[:n + 1])
    for q, line, R in zip(queries, ask(exe, queries), want):
        H = parse(line)
        assert len(H) == min(int(q.split()[4]), len(R)), (q, line)
        for k, (s, v) in enumerate(H):
            assert abs(v - R[k][1]) <= 1e-4, (q, k, v, R[k])
            near = (k > 0 and R[k - 1][1] - R[k][1] <= 2e-4) or (k + 1 < len(R) and R[k][1] - R[k + 1][1] <= 2e-4)
            assert near or s == R[k][0], (q, k, s, R[k])
