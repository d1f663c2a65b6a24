"""tools/asm_hazard_scan.py: a VALU-written SGPR read by a vector-memory instruction fewer than 5 wait states later (the round-6
fault behind lds_asm.h's s_nop 4 guards).  The scanner on small hand-written snippets, the scanner on the built library's gfx950
code, and the rule that the inline-asm LDS-DMA / atomic primitives live in lds_asm.h only."""
import os
import re
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_hazard_scan  # noqa: E402

CSRC = os.path.join(ROOT, "retto_amd", "csrc")
LLVM = "/opt/rocm/llvm/bin"


def _scan(tmp_path, body):
    p = tmp_path / "k.s"
    p.write_text("_Z1kv:\n" + "".join("\t%s\n" % l if not l.startswith(".") else "%s\n" % l for l in body.strip().splitlines()))
    return asm_hazard_scan.scan(str(p))


DMA = ";;#ASMSTART\ns_mov_b32 m0, s9\ns_nop 0\nbuffer_load_dwordx4 v1, s[4:7], s8 offen lds\n;;#ASMEND"


def _snippet(*lines):
    return "\n".join(l for ls in lines for l in ls.splitlines())


def test_straight_line_hit(tmp_path):
    assert _scan(tmp_path, _snippet("v_readlane_b32 s6, v40, 3", DMA, "s_endpgm")) == 1


def test_guard_clears_it(tmp_path):
    assert _scan(tmp_path, _snippet("v_readlane_b32 s6, v40, 3", ";;#ASMSTART\ns_nop 4", DMA.split("\n", 1)[1], "s_endpgm")) == 0
    # five wait states are needed, four are not enough
    atomic = ";;#ASMSTART\nglobal_atomic_add v1, v2, v3, s[6:7] sc0\n;;#ASMEND"
    assert _scan(tmp_path, _snippet("v_readlane_b32 s6, v40, 3", "s_nop 4", atomic, "s_endpgm")) == 0
    assert _scan(tmp_path, _snippet("v_readlane_b32 s6, v40, 3", "s_nop 3", atomic, "s_endpgm")) == 1


def test_hit_across_a_fall_through_label(tmp_path):
    assert _scan(tmp_path, _snippet("v_readfirstlane_b32 s8, v2", ".LBB0_1:", DMA, "s_endpgm")) == 1


def test_hit_over_a_loop_back_edge(tmp_path):
    # the writer sits at the bottom of the loop: only the back edge reaches the request at the loop head
    body = _snippet("s_mov_b32 s8, 0", "s_nop 7", ".LBB0_1:", DMA, "s_add_u32 s10, s10, 1", "s_nop 7",
                    "v_readlane_b32 s5, v41, 0", "s_cmp_lg_u32 s10, 8", "s_cbranch_scc1 .LBB0_1", "s_endpgm")
    assert _scan(tmp_path, body) == 1


def test_branch_that_skips_the_writer_is_no_excuse(tmp_path):
    # a branch around five wait states of padding joins a path on which the writer is adjacent
    body = _snippet("v_readlane_b32 s4, v40, 1", "s_cbranch_scc0 .LBB0_2", "s_nop 7", ".LBB0_2:", DMA, "s_endpgm")
    assert _scan(tmp_path, body) == 1


def test_non_readlane_valu_writers(tmp_path):
    assert _scan(tmp_path, _snippet("v_cmp_gt_u32_e64 s[6:7], v3, v4", DMA, "s_endpgm")) == 1
    assert _scan(tmp_path, _snippet("v_add_co_u32_e64 v5, s[4:5], v6, v7", DMA, "s_endpgm")) == 1
    # a VALU instruction that only READS the SGPR, and an SALU write, are no hazard
    assert _scan(tmp_path, _snippet("v_cndmask_b32_e64 v5, v6, v7, s[4:5]", "s_mov_b32 s8, 0", DMA, "s_endpgm")) == 0


def test_objdump_branch_targets(tmp_path):
    # llvm-objdump form: the branch offset is printed unsigned (65532 = -4 words: back to the request)
    lines = ["0000000000001000 <_Z1kv>:",
             "\ts_mov_b32 m0, s9                        // 000000001000: BEFC0009",
             "\ts_nop 0                                 // 000000001004: BF800000",
             "\tbuffer_load_dwordx4 v1, s[4:7], s8 offen lds // 000000001008: E05D1000 08010001",
             "\tv_readfirstlane_b32 s8, v2              // 000000001010: 7E100502",
             "\ts_cbranch_scc1 65532                    // 000000001014: BF85FFFC <_Z1kv+0x8>",
             "\ts_endpgm                                // 000000001018: BF810000"]
    p = tmp_path / "k.dis"
    p.write_text("\n".join(lines) + "\n")
    assert asm_hazard_scan.scan(str(p)) == 1


def _code_objects(lib, out_dir):
    """The gfx950 code objects of the library's offload bundles (one per translation unit with device code)."""
    sec = out_dir / "fatbin.bin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, str(sec)])
    data, magic, cos, i = sec.read_bytes(), b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while True:
        j = data.find(magic, i)
        if j < 0: break
        n, p = struct.unpack_from("<Q", data, j + 24)[0], j + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if triple.endswith("gfx950") and size:
                co = out_dir / ("co%d.elf" % len(cos))
                co.write_bytes(data[j + off:j + off + size])
                cos.append(co)
        i = j + len(magic)
    return cos


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm LLVM tools")
def test_built_library_has_no_hazard_site(tmp_path):
    """Every VMEM instruction of every kernel in the built libretto_hip.so (the disassembly: no asm markers, compiler and asm
    instructions alike), all paths into it.  ~20 s."""
    lib = os.path.join(ROOT, "retto_amd", "libretto_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-j8", "-s"])
    cos = _code_objects(lib, tmp_path)
    assert len(cos) >= 3
    n = 0
    kernels = set()
    for co in cos:
        dis = co.with_suffix(".dis")
        with open(dis, "w") as f:
            subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", str(co)], stdout=f)
        for name, code in asm_hazard_scan.parse(str(dis)):
            kernels.add(name)
            n += asm_hazard_scan.scan_function(str(dis), name, code)
    assert any("k_gemm32p" in k for k in kernels) and any("k_gemm_split" in k for k in kernels) and any("k_conv16v2" in k for k in kernels)
    assert n == 0


def test_lds_dma_and_atomic_asm_only_in_lds_asm_h():
    pat = re.compile(r"global_load_lds|buffer_load\w*[^\"]*\blds\b|global_atomic")
    bad = []
    for name in sorted(os.listdir(CSRC)):
        if name == "lds_asm.h" or not name.endswith((".hip", ".h", ".cpp")): continue
        src = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r"asm\s+(?:volatile\s*)?\(\s*((?:\"(?:[^\"\\]|\\.)*\"\s*)+)", src):
            if pat.search(m.group(1)): bad.append("%s:%d" % (name, src.count("\n", 0, m.start()) + 1))
    assert not bad, bad
    hdr = open(os.path.join(CSRC, "lds_asm.h")).read()
    assert hdr.count("#pragma clang diagnostic push") == hdr.count("#pragma clang diagnostic pop") == 1
    # the guard: every asm statement in the header whose VMEM instruction takes a scalar operand opens with s_nop 4 (the
    # 64-bit-address form's only scalar operand goes to M0 through an SALU s_mov: no hazard); the exception says so in its name
    prims = re.findall(r'__device__ __forceinline__ \w+ (\w+)\([^)]*\) \{\s*(?:unsigned \w+;\s*)?asm volatile\("([^"]*)"', hdr)
    vmem = [(name, t) for name, t in prims if re.search(r"(buffer|global)_", t)]
    assert len(vmem) == 6, vmem
    for name, t in vmem:
        if not t.endswith(", off") and not name.endswith("_unguarded"): assert t.startswith("s_nop 4"), (name, t)
