#!/bin/bash
# Compiles the kernel files that use the inline-asm memory primitives (every .hip file that includes lds_asm.h) to assembly (device
# only, gfx950) and scans every vector-memory instruction in them with tools/asm_hazard_scan.py for an SGPR written by a VALU
# instruction fewer than 5 wait states earlier, on any path -- the hazard behind round 6's memory faults.
# ~3.5 minutes on 8 cores.  tests/test_asm_hazard_cpu.py runs the same scan on the built library's disassembly in ~20 s.
set -u
cd "$(dirname "$0")/../retto_amd/csrc"
out=${TMPDIR:-/tmp}/rt_asm_scan; mkdir -p $out
files=$(grep -l '#include "lds_asm.h"' *.hip)
for f in $files; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast --cuda-device-only -S $f -o $out/${f%.hip}.s 2>/dev/null &
done
wait
python3 ../../tools/asm_hazard_scan.py $(for f in $files; do echo $out/${f%.hip}.s; done)
