#!/usr/bin/env python3
"""What the compiler made of K2's on-grid chunk: the instruction mix of the basic block that holds its loads, for the four headline kernels.

    scripts/k2_chunk_isa.py [object] [--dump]

object: the built kernel object (default libzl_amd/lib/obj/libzlhip/zl_kernels.o, what libzl_amd/build.py leaves; a variant's object sits in
lib/obj/libzlhip_<name>/).  The gfx950 code object is taken out of the object's .hip_fatbin section, unbundled and disassembled as scripts/device_code_diff.py does.  A basic block ends at
a branch or in front of a branch target.  Printed for each kernel: every block that issues at least ZL_K2_U = 8 loads of the stereo
on-grid chunk's width (global_load_dwordx2 with one frame per lane, global_load_dwordx4 with two) -- the steady-state chunk (straight-line: the
block with the v_pk_* arithmetic of all its voices), the report-path chunk (its loads; the voices follow in blocks of their own) and, in the pair
kernels, the two-tap chunks, whose loads have the same width.  Per block: loads, VALU instructions by opcode, LDS reads, and VALU per voice-wave
(8 voices are 8 voice-waves with one frame per lane, 16 with two; meaningful where the block holds the voices' arithmetic).  --dump prints the blocks.
A report, not a test."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
U = 8
KERNELS = [("_Z12zl_k2_renderILj0ELi1ELb0EEv7ZlBatch", "global_load_dwordx2", 1), ("_Z18zl_k2_phase_renderILj0EEv7ZlBatch", "global_load_dwordx2", 1),
           ("_Z17zl_k2_pair_render7ZlBatch", "global_load_dwordx4", 2), ("_Z23zl_k2_pair_phase_render7ZlBatch", "global_load_dwordx4", 2)]


def disassemble(obj: str) -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "k.fatbin"), os.path.join(tmp, "k.co")
        # (a host object carries its device code as a bundle in the section .hip_fatbin)
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle",
                        f"--input={fat}", f"--output={co}"], check=True)
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None or not line.strip():
            continue
        ins, _, tail = line.partition("//")
        addr = re.match(r"\s*([0-9A-Fa-f]+):", tail)
        out[name].append((int(addr.group(1), 16) if addr else -1, " ".join(ins.split())))
    return out


def blocks(code: list) -> list:
    """basic blocks of a function: cut behind every branch and in front of every branch target"""
    targets = set()
    for i, (addr, ins) in enumerate(code):
        m = re.match(r"s_c?branch\S*\s+(\d+)", ins)
        if m and i + 1 < len(code):
            off = int(m.group(1))
            off -= 65536 if off >= 32768 else 0
            targets.add(code[i + 1][0] + 4 * off)
    out, cur = [], []
    for addr, ins in code:
        if addr in targets and cur:
            out.append(cur); cur = []
        cur.append(ins)
        if re.match(r"s_c?branch|s_endpgm|s_setpc", ins):
            out.append(cur); cur = []
    if cur:
        out.append(cur)
    return out


def main() -> int:
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    obj = args[0] if args else os.path.join(ROOT, "libzl_amd", "lib", "obj", "libzlhip", "zl_kernels.o")
    fns = disassemble(obj)
    for name, load, frames in KERNELS:
        if name not in fns:
            print(f"{name}: not in {obj}")
            continue
        cand = [b for b in blocks(fns[name]) if sum(i.startswith(load + " ") for i in b) >= U]
        if not cand:
            print(f"{name}: no block with {U} {load}")
            continue
        print(name)
        for blk in cand:
            ops = collections.Counter(re.sub(r"_e(32|64)$", "", i.split()[0]) for i in blk if i.startswith("v_"))
            nload = sum(i.startswith("global_load") for i in blk)
            # a voice is one load of the chunk's width; the pair chunk with loop restarts (zl_k2_chunk_ongrid_pair_wrap) issues a narrower second
            # load per voice, for the frame of a pair that straddles the restart
            nvoice = sum(i.startswith(load + " ") for i in blk)
            what = f"{nload} loads" if nload == nvoice else f"{nload} loads ({nvoice} voices, {nload - nvoice} straddle loads: the chunk with loop restarts)"
            print(f"  block of {len(blk)} instructions ending in {blk[-1].split()[0]}: {what}, {sum(i.startswith('ds_read') for i in blk)} LDS reads, "
                  f"{sum(i.startswith('s_') for i in blk)} scalar, {sum(ops.values())} VALU = {sum(ops.values()) / (nvoice * frames):.1f} per voice-wave")
            print("    " + ", ".join(f"{n} {o}" for o, n in sorted(ops.items(), key=lambda kv: (-kv[1], kv[0]))))
            if "--dump" in sys.argv:
                print("\n".join("        " + i for i in blk))
    return 0


if __name__ == "__main__":
    sys.exit(main())
