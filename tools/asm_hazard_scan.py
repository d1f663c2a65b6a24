"""Scans gfx950 device code for the hazard found in round 6: an SGPR written by a VALU instruction and read by a vector-memory
(VMEM) instruction fewer than 5 wait states later.  hipcc's hazard recogniser pads its own instructions but does not look into
inline-asm blocks: a spilled scalar restored by v_readlane right in front of an asm buffer_load ... lds left the load reading
stale descriptor words (memory faults that came and went with the register allocation).  lds_asm.h opens such asm statements
with s_nop 4; the sites of its one unguarded form are clean only as long as this scan says so.

Input: hipcc assembly (-S --cuda-device-only; labels .LBB*) or llvm-objdump -d output of a code object (branch targets as
<symbol+0xoffset>).  Every VMEM instruction is checked, inside asm blocks or not.  The walk back from it follows every path:
fall-through, and at a branch target every branch to it -- back edges included (conservative).  Writers: any VALU instruction
with an SGPR destination -- v_readlane / v_readfirstlane, v_cmp* into an SGPR pair, VOP3b carry-outs (v_add_co_u32 vN, s[a:b]),
v_div_scale, v_mad_u64_u32 ...

Usage: python tools/asm_hazard_scan.py file.s|file.dis [...]; prints every site with the distance found, exits 1 if any."""
import re
import sys

VMEM = re.compile(r"(buffer|global|flat|scratch)_")
SREG = re.compile(r"\bs\[(\d+):(\d+)\]|\bs(\d+)\b|\b(vcc(?:_lo|_hi)?)\b")
NAMED = {"vcc": (106, 107), "vcc_lo": (106,), "vcc_hi": (107,)}   # VCC is s[106:107] on gfx9
SECOND_DST = re.compile(r"^v_\w*(_co_|_co$|div_scale|mad_u64_u32|mad_i64_i32)")   # VOP3b: the second operand is an SGPR destination
NO_FALLTHROUGH = re.compile(r"^(s_branch|s_endpgm|s_setpc_b64)\b")
BRANCH = re.compile(r"^s_(c?branch\w*)\b")
FUNC_S = re.compile(r"^(_Z[\w$.]*|[A-Za-z_][\w$.]*):\s*(;.*)?$")        # hipcc -S: a function's label
LABEL_S = re.compile(r"^(\.L\w+):")
FUNC_D = re.compile(r"^([0-9a-f]+) <([^>]+)>:$")                      # llvm-objdump: "0000000000005200 <name>:"
ADDR_D = re.compile(r"//\s*([0-9A-Fa-f]+):")


def sregs(operands):
    out = set()
    for m in SREG.finditer(operands):
        if m.group(1) is not None: out.update(range(int(m.group(1)), int(m.group(2)) + 1))
        elif m.group(3) is not None: out.add(int(m.group(3)))
        else: out.update(NAMED[m.group(4)])
    return out


def split_ops(ins):
    parts = ins.split(None, 1)
    return parts[0], ([o.strip() for o in parts[1].split(",")] if len(parts) > 1 else [])


def sgpr_dests(ins):
    """SGPRs an instruction writes if it is a VALU instruction (empty otherwise)."""
    op, ops = split_ops(ins)
    if not op.startswith("v_") or not ops: return set()
    dst = set()
    if not ops[0].startswith(("v", "a")) or ops[0].startswith("vcc"): dst |= sregs(ops[0])
    if len(ops) > 1 and SECOND_DST.match(op): dst |= sregs(ops[1])
    return dst


def wait_states(ins):
    m = re.match(r"s_nop\s+(\d+)", ins)
    return int(m.group(1)) + 1 if m else 1


def parse(path):
    """[(function, [instructions])]; an instruction is a dict: text, line, key (branch-target key), target, in_asm."""
    funcs, cur, labels, in_asm = [], None, [], False
    for ln, raw in enumerate(open(path, errors="replace"), 1):
        line = raw.rstrip("\n")
        s = line.strip()
        if s.startswith(";;#ASMSTART"): in_asm = True; continue
        if s.startswith(";;#ASMEND"): in_asm = False; continue
        m = FUNC_D.match(line)
        if m:
            cur = (m.group(2), []); funcs.append(cur); labels = []; continue
        if not line[:1].isspace():
            m = LABEL_S.match(line)
            if m: labels.append(m.group(1)); continue
            m = FUNC_S.match(line)
            if m and not line.startswith("."): cur = (m.group(1), []); funcs.append(cur); labels = []
            continue
        if cur is None: continue
        text = re.split(r"\s*(//|;)", s, 1)[0].strip()
        if not text or text.startswith("."): continue
        ins = {"text": text, "line": ln, "keys": labels, "target": None, "in_asm": in_asm}
        labels = []
        a = ADDR_D.search(s)
        if a: ins["keys"] = [int(a.group(1), 16)]
        ops = split_ops(text)[1]
        if BRANCH.match(text) and ops:
            if a:   # objdump prints the 16-bit word offset unsigned: target = next instruction + 4 * simm16
                off = int(ops[0], 0) & 0xffff
                ins["target"] = int(a.group(1), 16) + 4 + 4 * (off - 0x10000 if off & 0x8000 else off)
            else:
                ins["target"] = ops[-1]
        cur[1].append(ins)
    return funcs


def scan_function(path, name, code):
    at = {}
    for i, ins in enumerate(code):
        for k in ins["keys"]: at[k] = i
    preds = [[] for _ in code]
    for i, ins in enumerate(code):
        if i + 1 < len(code) and not NO_FALLTHROUGH.match(ins["text"]): preds[i + 1].append(i)
        if ins["target"] is not None and ins["target"] in at: preds[at[ins["target"]]].append(i)
    dests = [sgpr_dests(ins["text"]) for ins in code]
    waits = [wait_states(ins["text"]) for ins in code]
    found = 0
    for i, ins in enumerate(code):
        if not VMEM.match(ins["text"]): continue
        used = sregs(" ".join(split_ops(ins["text"])[1]))
        if not used: continue
        # backward walk: (instruction, wait states between it and the VMEM instruction)
        stack, seen, hits = [(p, 0) for p in preds[i]], set(), {}
        while stack:
            j, ws = stack.pop()
            if ws >= 5 or (j, ws) in seen: continue
            seen.add((j, ws))
            w = dests[j] & used
            if w: hits.setdefault(j, (ws, w))
            stack.extend((p, ws + waits[j]) for p in preds[j])
        for j, (ws, w) in sorted(hits.items()):
            print("%s:%d  %s%s\n    in %s: s%s written by `%s` (line %d) %d wait state(s) earlier"
                  % (path, ins["line"], ins["text"], "  [inline asm]" if ins["in_asm"] else "", name[:100],
                     ",s".join(str(r) for r in sorted(w)), code[j]["text"], code[j]["line"], ws))
            found += 1
    return found


def scan(path):
    return sum(scan_function(path, name, code) for name, code in parse(path))


if __name__ == "__main__":
    n = sum(scan(p) for p in sys.argv[1:])
    print("%d hazard site(s)" % n)
    sys.exit(1 if n else 0)
