"""The rec pattern compiler (retto_amd/csrc/ctc_pattern.h) under AddressSanitizer + UBSan on mutated and random pattern bytes
(tests/fuzz/fuzz_pattern.cpp: a stand-alone program, nothing preloaded; CPU only).  Every input ends in a status code; an
accepted one in tables inside the caps whose host Viterbi matches exactly from min_steps on and returns a path the DFA accepts."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz_pattern") / "fuzz_pattern")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "fuzz", "fuzz_pattern.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the sanitizer build failed:\n" + r.stderr[-3000:]
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_compiler_survives_mutated_patterns(exe, seed):
    r = subprocess.run([exe, "20000", str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    words = r.stdout.split()
    assert int(words[0]) > 1000 and int(words[2]) > 1000, r.stdout   # the mutations reach both outcomes
