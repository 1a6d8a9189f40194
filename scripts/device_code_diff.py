#!/usr/bin/env python3
"""Is the device code of two builds of a kernel source the same, kernel by kernel?

    scripts/device_code_diff.py <tree A> <tree B> [zl_kernels.hip ...]

Compiles each source of libzl_amd/csrc/ in both trees with the library's flags plus --cuda-device-only, unbundles the gfx950 code object,
disassembles it and hashes every function's instructions -- without their own addresses and without symbolised branch targets, which move when
a neighbour does.  The whole file's hash is no use for this: template instantiation order follows the host's launch code, so a pure host edit
reorders the kernels.  Prints the number of functions per side and every name whose hash differs or that exists on one side only; exit
status 1 if there is one.  A host-only change of a .hip file must come out equal."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function"]   # build.py's


def functions(tree: str, source: str, tmp: str, tag: str) -> dict:
    csrc = os.path.join(tree, "libzl_amd", "csrc")
    obj, co = os.path.join(tmp, tag + ".o"), os.path.join(tmp, tag + ".co")
    hipcc = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
    subprocess.run([hipcc] + FLAGS + ["-I", os.path.join(tree, "include"), "-I", csrc, "--cuda-device-only", "-x", "hip", "-c", os.path.join(csrc, source), "-o", obj], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle", f"--input={obj}", f"--output={co}"], check=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    out, name, h = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name, h = m.group(1), hashlib.sha256()
            out[name] = h
            continue
        if name is None or not line.strip():
            continue
        ins = line.split("//")[0]                       # the comment holds the instruction's own address and encoding offset
        ins = re.sub(r"<[^>]*>", "<>", ins)             # symbolised branch targets
        h.update(" ".join(ins.split()).encode() + b"\n")
    return {k: v.hexdigest() for k, v in out.items()}


def main() -> int:
    a, b = sys.argv[1], sys.argv[2]
    sources = sys.argv[3:] or ["zl_kernels.hip", "zl_stretch.hip"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for src in sources:
            fa, fb = functions(a, src, tmp, "a"), functions(b, src, tmp, "b")
            diff = sorted(n for n in set(fa) | set(fb) if fa.get(n) != fb.get(n))
            print(f"{src}: {len(fa)} / {len(fb)} functions, {len(diff)} differ")
            for n in diff:
                print("   ", n, "(one side only)" if n not in fa or n not in fb else "")
            bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
