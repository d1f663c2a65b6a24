"""The host-only plan driver (tests/native/gemm_plan_driver.cpp + the plan sources of retto_amd/csrc, compiled with g++: no GPU,
no HIP runtime), built once per test session and shared by test_gemm_plan_cpu.py, test_lc_plan_cpu.py,
test_rec_tail_plan_cpu.py, test_rec_line_opts_cpu.py and test_lane_split_cpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "retto_amd", "csrc")
_exe = None


def build(tmp_path_factory):
    global _exe
    if _exe is None:
        exe = str(tmp_path_factory.mktemp("plan_driver") / "plan_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
               os.path.join(ROOT, "tests", "native", "gemm_plan_driver.cpp"), os.path.join(CSRC, "gemm_plan.cpp"),
               os.path.join(CSRC, "lc_plan.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, "the plan driver does not build:\n" + r.stderr[-3000:]
        _exe = exe
    return _exe


def run(exe, queries, env=None):
    """One answer line per query line; env: environment switches the plans read when the driver starts."""
    r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    out = r.stdout.splitlines()
    assert len(out) == len(queries)
    return out
