"""Builds the in-tree native libraries.

    libzl_amd/lib/libzlhip.so      HIP engine + C-ABI (include/zlhip.h), gfx950 only
    oracle/_build/libzl_oracle.so  CPU oracle (test infrastructure; never loaded by the product)
    oracle/_ref/libzl_refvoice.so  the reference's own SamplerSynthVoice.cpp, compiled unmodified (test infrastructure; only where
                                   the reference tree is present, never committed)

hipcc cross-compiles for gfx950 without a GPU, so this runs in the CPU-only build container.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libzl_amd", "csrc")
LIBDIR = os.path.join(ROOT, "libzl_amd", "lib")
LIB = os.path.join(LIBDIR, "libzlhip.so")

HIP_SOURCES = ["zl_kernels.hip", "zl_stretch.hip", "zl_overview.hip", "zl_onset.hip", "zl_tempo.hip", "zl_pitch.hip", "zl_loudness.hip", "zl_loop.hip", "zl_key.hip", "zl_xfade.hip", "zl_edit.hip", "zl_limit.hip", "zl_warp.hip", "zl_decode.hip", "zl_resample.hip", "zl_engine.cpp", "zl_clip_calls.cpp", "zl_libzl.cpp", "zl_group.cpp"]
HEADERS = ["zl_types.h", "zl_arena.h", "zl_plan.h", "zl_order.h", "zl_pair.h", "zl_launch.h", "zl_render.h", "zl_kernels.h", "zl_host.h", "zl_sched.h", "zl_handoff.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_tempo.h", "zl_pitch.h", "zl_loudness.h", "zl_loop.h", "zl_key.h", "zl_xfade.h", "zl_edit.h", "zl_limit.h", "zl_warp.h", "zl_decode.h", "zl_resample.h", "zl_group.h", "zl_member.h", "zl_owned.h", "zl_engine_impl.h",
           os.path.join("..", "..", "include", "zlhip.h"), os.path.join("..", "..", "include", "libzl_hotpath.h")]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (needed to build libzlhip.so for gfx950)")


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build_variant(name: str, flags: list, verbose: bool = False) -> str:
    """A/B and diagnostic builds: libzl_amd/lib/libzlhip_<name>.so with extra -D flags (loaded through the ZLHIP_LIBRARY
    environment variable by scripts/; never by the package itself)."""
    global LIB
    saved, LIB = LIB, os.path.join(LIBDIR, f"libzlhip_{name}.so")
    try:
        return _build_engine(False, verbose, list(flags))
    finally:
        LIB = saved


def build_engine(force: bool = False, verbose: bool = False, stamps: bool = False) -> str:
    """stamps=True builds the diagnostic variant libzlhip_stamps.so (-DZL_STAMPS: per-workgroup
    timestamps in K2; used only by scripts/k2_stamps.py, never by the package)."""
    global LIB
    if stamps:
        out = os.path.join(LIBDIR, "libzlhip_stamps.so")
        saved, LIB = LIB, out
        try:
            return _build_engine(force, verbose, ["-DZL_STAMPS"])
        finally:
            LIB = saved
    return _build_engine(force, verbose, [])


# per source: the headers it includes (a change of one of them recompiles only the sources that see it)
_INC = os.path.join("..", "..", "include")
SOURCE_DEPS = {
    "zl_kernels.hip": ["zl_types.h", "zl_plan.h", "zl_render.h", "zl_order.h", "zl_pair.h", "zl_launch.h", "zl_kernels.h"],
    "zl_stretch.hip": ["zl_types.h", "zl_stretch.h"],
    "zl_overview.hip": ["zl_types.h", "zl_overview.h"],
    "zl_onset.hip": ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h"],
    "zl_tempo.hip": ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_tempo.h"],
    "zl_pitch.hip": ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h"],
    "zl_loudness.hip": ["zl_types.h", "zl_overview.h", "zl_loudness.h"],
    "zl_loop.hip": ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h", "zl_loop.h"],
    "zl_key.hip": ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h", "zl_key.h"],
    "zl_xfade.hip": ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h", "zl_xfade.h"],
    "zl_edit.hip": ["zl_types.h", "zl_overview.h", "zl_edit.h"],
    "zl_limit.hip": ["zl_types.h", "zl_overview.h", "zl_resample.h", "zl_limit.h"],
    "zl_warp.hip": ["zl_types.h", "zl_stretch.h", "zl_warp.h"],
    "zl_decode.hip": ["zl_types.h", "zl_decode.h"],
    "zl_resample.hip": ["zl_types.h", "zl_resample.h"],
    # (zl_stretch.h: through zl_arena.h)
    "zl_engine.cpp": ["zl_types.h", "zl_arena.h", "zl_plan.h", "zl_render.h", "zl_order.h", "zl_pair.h", "zl_launch.h", "zl_host.h", "zl_kernels.h", "zl_member.h", "zl_owned.h", "zl_engine_impl.h", "zl_stretch.h", os.path.join(_INC, "zlhip.h")],
    # the clip services: the engine's state and the services' own headers, none of the render kernels'
    "zl_clip_calls.cpp": ["zl_types.h", "zl_arena.h", "zl_plan.h", "zl_host.h", "zl_owned.h", "zl_engine_impl.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_tempo.h", "zl_pitch.h", "zl_loudness.h", "zl_loop.h", "zl_key.h", "zl_xfade.h", "zl_edit.h", "zl_limit.h", "zl_warp.h", "zl_decode.h", "zl_resample.h", os.path.join(_INC, "zlhip.h")],
    "zl_group.cpp": ["zl_types.h", "zl_plan.h", "zl_order.h", "zl_pair.h", "zl_launch.h", "zl_host.h", "zl_kernels.h", "zl_member.h", "zl_group.h", os.path.join(_INC, "zlhip.h")],
    "zl_libzl.cpp": ["zl_render.h", "zl_types.h", "zl_sched.h", "zl_handoff.h", "zl_stretch.h", os.path.join(_INC, "zlhip.h"), os.path.join(_INC, "libzl_hotpath.h")],
}


def _write_kernel_resources(remarks: str, path: str) -> None:
    """The compiler's per-kernel resource remarks, one line per kernel: name, VGPRs, scratch bytes per lane, waves per SIMD, LDS bytes.
    tests/test_kernel_resources.py holds the kernels to what DESIGN.md states (the resident kernel without scratch memory, K2 without spills)."""
    import re
    rows, cur = [], None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0] + ("Spill" if "Spill" in m.group(1) else "")] = int(m.group(2))
    with open(path, "w") as f:
        for r in rows:
            f.write(f"{r['name']} vgprs={r.get('VGPRs', -1)} scratch={r.get('ScratchSize', -1)} waves={r.get('Occupancy', -1)} lds={r.get('LDS', -1)} vgpr_spill={r.get('VGPRsSpill', -1)}\n")


def _build_engine(force: bool, verbose: bool, extra: list) -> str:
    """One object per source (cached under lib/obj/<library name>/), then one link: editing the host code does not recompile
    the kernels (two minutes)."""
    names = [s for s in HIP_SOURCES if os.path.exists(os.path.join(CSRC, s))]
    envflags = [f for f in os.environ.get("ZL_EXTRA_HIPCC_FLAGS", "").split() if f]
    objdir = os.path.join(LIBDIR, "obj", os.path.splitext(os.path.basename(LIB))[0])
    os.makedirs(objdir, exist_ok=True)
    flagfile = os.path.join(objdir, "flags.txt")
    flags = " ".join(extra + envflags)
    alldeps = [os.path.join(CSRC, n) for n in names] + [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    if not force and not extra and not envflags and not _stale(LIB, alldeps):
        return LIB                      # (the GPU box receives the library without the object cache)
    if not os.path.exists(flagfile) or open(flagfile).read() != flags:
        force = True
    common = [
        _hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
        # the oracle defines an un-fused rounding sequence; never contract a*b+c into fma
        "-ffp-contract=off", "-fno-fast-math",
        "-I", os.path.join(ROOT, "include"), "-I", CSRC,
        "-Wall", "-Wno-unused-function",
    ] + extra + envflags
    objs, rebuilt = [], False
    for name in names:
        src = os.path.join(CSRC, name)
        obj = os.path.join(objdir, os.path.splitext(name)[0] + ".o")
        deps = [src, os.path.abspath(__file__)] + [os.path.join(CSRC, h) for h in SOURCE_DEPS.get(name, HEADERS)]
        if force or _stale(obj, deps):
            cmd = common + ["-x", "hip", "-c", src, "-o", obj]
            kernels = name.endswith(".hip")
            if kernels:
                cmd.append("-Rpass-analysis=kernel-resource-usage")      # registers / scratch / occupancy of every kernel -> kernel_resources.txt
            if verbose:
                print(" ".join(cmd), flush=True)
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                sys.stderr.write(res.stdout + res.stderr)
                raise RuntimeError(f"hipcc failed compiling {name}")
            if kernels:
                # zl_kernels.hip -> <library>_kernel_resources.txt; every other kernel source -> <library>_<source>_kernel_resources.txt
                stem = os.path.splitext(os.path.basename(LIB))[0] + ("" if name == "zl_kernels.hip" else "_" + os.path.splitext(name)[0])
                _write_kernel_resources(res.stderr, os.path.join(os.path.dirname(LIB), stem + "_kernel_resources.txt"))
            elif verbose and res.stderr:
                sys.stderr.write(res.stderr)
            rebuilt = True
        objs.append(obj)
    if rebuilt or not os.path.exists(LIB):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            raise RuntimeError("hipcc failed linking libzlhip.so")
        with open(flagfile, "w") as f:
            f.write(flags)
    return LIB


def build_oracle(force: bool = False) -> str:
    odir = os.path.join(ROOT, "oracle")
    target = os.path.join(odir, "_build", "libzl_oracle.so")
    deps = [os.path.join(odir, "zl_oracle.c"), os.path.join(odir, "zl_oracle.h"), os.path.join(odir, "Makefile")]
    if force or _stale(target, deps):
        res = subprocess.run(["make", "-C", odir, "_build/libzl_oracle.so"], capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            raise RuntimeError("building the CPU oracle failed")
    return target


def reference_dir():
    """The reference tree (zynthbox/libzl): $ZL_REFERENCE_DIR, else /root/reference; None where there is none."""
    for cand in (os.environ.get("ZL_REFERENCE_DIR"), "/root/reference"):
        if cand and os.path.exists(os.path.join(cand, "lib", "SamplerSynthVoice.cpp")):
            return cand
    return None


REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libzl_refvoice.so")
REF_LIB_CONTRACTED = os.path.join(ROOT, "oracle", "_ref", "libzl_refvoice_fma.so")


def build_reference(force: bool = False, contracted: bool = False):
    """oracle/_ref/libzl_refvoice.so: the reference's lib/SamplerSynthVoice.cpp as it stands, compiled against the stand-in
    headers of oracle/ref_shim/ with the oracle's floating-point flags (x86-64 baseline, no contraction), linked with
    oracle/ref_driver.cpp (the neighbours' getters + a C interface) and oracle/zl_oracle.c (juce::ADSR stand-in, positions rows).
    Returns None, leaving an existing oracle/_ref/ alone, where there is no reference tree (the built library travels).
    contracted=True builds libzl_refvoice_fma.so with -mfma -ffp-contract=fast: a measurement of how far a contracting build
    of the reference may sit from the definition, which no test depends on."""
    ref = reference_dir()
    if ref is None:
        return None
    odir = os.path.join(ROOT, "oracle")
    target = REF_LIB_CONTRACTED if contracted else REF_LIB
    voice = os.path.join(ref, "lib", "SamplerSynthVoice.cpp")
    driver = os.path.join(odir, "ref_driver.cpp")
    shim = os.path.join(odir, "ref_shim")
    deps = [voice, driver, os.path.join(odir, "zl_oracle.c"), os.path.join(odir, "zl_oracle.h"), os.path.abspath(__file__)]
    deps += [os.path.join(d, f) for d, _, fs in os.walk(shim) for f in fs]
    deps += [os.path.join(ref, "lib", f) for f in os.listdir(os.path.join(ref, "lib")) if f.endswith(".h")]
    if not force and not _stale(target, deps):
        return target
    os.makedirs(os.path.dirname(target), exist_ok=True)
    fp = ["-O2", "-mfma", "-ffp-contract=fast"] if contracted else ["-O2", "-ffp-contract=off", "-fno-fast-math"]
    cobj = os.path.join(os.path.dirname(target), "zl_oracle_fma.o" if contracted else "zl_oracle.o")
    # (the envelope keeps the oracle's flags in both builds: only the reference's own text is contracted)
    cmds = [["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-c", os.path.join(odir, "zl_oracle.c"), "-o", cobj],
            ["g++", "-std=c++17"] + fp + ["-fPIC", "-shared", "-Wall", "-Wl,-Bsymbolic", "-I", shim, "-I", odir, "-I", os.path.join(ref, "lib"),
                                          "-o", target, voice, driver, cobj, "-lm", "-lpthread"]]
    for cmd in cmds:
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            raise RuntimeError("building the reference voice failed")
    return target


_ZLHIP_H = os.path.join(_INC, "zlhip.h")
_NO_CONTRACT = ["-ffp-contract=off", "-fno-fast-math"]


def _build_harness(name: str, source: str, headers: list, flags: list, force: bool = False) -> str:
    """tests/cpu_harness/<source> -> tests/cpu_harness/_build/lib<name>.so with g++: the host build of HIP-free product headers (paths relative
    to csrc/) for the CPU tier.  (-Bsymbolic: the header-inline code of the library binds to ITS copies, not to libzlhip.so's when both are loaded)"""
    hdir = os.path.join(ROOT, "tests", "cpu_harness")
    target = os.path.join(hdir, "_build", f"lib{name}.so")
    src = os.path.join(hdir, source)
    if force or _stale(target, [src] + [os.path.join(CSRC, h) for h in headers]):
        os.makedirs(os.path.dirname(target), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O2"] + flags + ["-fPIC", "-shared", "-Wl,-Bsymbolic", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", target, src]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            raise RuntimeError(f"building the CPU test harness {source} failed")
    return target


def build_cpu_harness(force: bool = False) -> str:
    """Host builds of the __host__ __device__ planning / per-frame code, the product's ClipCommand scheduler (zl_sched.h) and the clip re-render
    (zl_stretch.h: the CPU tier's bit-exact check and the host side of scripts/rerender_bench.py).  Returns the first."""
    target = _build_harness("zl_plan_host", "plan_host.cpp", ["zl_types.h", "zl_plan.h", "zl_render.h", "zl_host.h", _ZLHIP_H], _NO_CONTRACT, force)
    _build_harness("zl_sched_host", "sched_host.cpp", ["zl_sched.h", _ZLHIP_H], _NO_CONTRACT + ["-Wall"], force)
    _build_harness("zl_stretch_host", "stretch_host.cpp", ["zl_stretch.h", "zl_types.h"], _NO_CONTRACT + ["-Wall", "-pthread"], force)
    return target


def build_order_harness(force: bool = False) -> str:
    """K2's phase order (zl_order.h)."""
    return _build_harness("zl_order_host", "order_host.cpp", ["zl_types.h", "zl_plan.h", "zl_order.h", "zl_host.h", _ZLHIP_H], _NO_CONTRACT + ["-Wall", "-Wno-unused-function"], force)


def build_order_summary_harness(force: bool = False) -> str:
    """The run summary K1o leaves behind the order table (zl_order.h)."""
    return _build_harness("zl_order_summary_host", "order_summary_host.cpp", ["zl_types.h", "zl_order.h"], ["-Wall", "-Wno-unused-function"], force)


def build_ongrid_harness(force: bool = False) -> str:
    """K2's on-grid form (zl_render.h)."""
    return _build_harness("zl_ongrid_host", "ongrid_host.cpp", ["zl_types.h", "zl_render.h"], _NO_CONTRACT + ["-Wall", "-Wno-unused-function"], force)


def build_ongrid_pk_harness(force: bool = False) -> str:
    """K2's packed on-grid mix as restated for the host (zl_render.h, zl_mix_frame_ongrid_pk)."""
    return _build_harness("zl_ongrid_pk_host", "ongrid_pk_host.cpp", ["zl_types.h", "zl_render.h"], _NO_CONTRACT + ["-Wall", "-Wno-unused-function"], force)


def build_pair_harness(force: bool = False) -> str:
    """The gate of K2's two-frames-per-lane kernels (zl_pair.h)."""
    return _build_harness("zl_pair_host", "pair_host.cpp", ["zl_pair.h"], ["-Wall"], force)


def build_pair_wrap_harness(force: bool = False) -> str:
    """The pair kernels' on-grid form for blocks with one loop restart (zl_render.h: zl_voice_ongrid2, zl_ongrid2_lane), with the host planner."""
    plan_host = os.path.join("..", "..", "tests", "cpu_harness", "plan_host.cpp")        # (included by the harness for its ZlSim)
    return _build_harness("zl_pair_wrap_host", "pair_wrap_host.cpp", ["zl_types.h", "zl_plan.h", "zl_render.h", "zl_host.h", _ZLHIP_H, plan_host],
                          _NO_CONTRACT + ["-Wall", "-Wno-unused-function"], force)


def build_pair_scalar_harness(force: bool = False) -> str:
    """The pair kernels' scalar records (zl_render.h: zl_voice_block_class, zl_pair_fast_bits, zl_pair_group_need; zl_pair.h:
    zl_pair_scalar_window), made the way K1c makes them, with the host planner."""
    plan_host = os.path.join("..", "..", "tests", "cpu_harness", "plan_host.cpp")        # (included by the harness for its ZlSim)
    return _build_harness("zl_pair_scalar_host", "pair_scalar_host.cpp", ["zl_types.h", "zl_plan.h", "zl_render.h", "zl_order.h", "zl_pair.h", "zl_host.h", _ZLHIP_H, plan_host],
                          _NO_CONTRACT + ["-Wall", "-Wno-unused-function"], force)


def build_pair_laps_harness(force: bool = False) -> str:
    """The pair kernels' two-slot workgroups (zl_launch.h: zl_k2_launch with pair_laps, zl_k2_pair_laps), with the host planner, the scalar
    records and the host order."""
    hdir = os.path.join("..", "..", "tests", "cpu_harness")
    return _build_harness("zl_pair_laps_host", "pair_laps_host.cpp", ["zl_types.h", "zl_plan.h", "zl_render.h", "zl_order.h", "zl_pair.h", "zl_launch.h", "zl_host.h", _ZLHIP_H,
                                                                      os.path.join(hdir, "plan_host.cpp"), os.path.join(hdir, "pair_scalar_host.cpp")],
                          _NO_CONTRACT + ["-Wall", "-Wno-unused-function"], force)


def build_group_harness(force: bool = False) -> str:
    """The engine group's partition arithmetic and command routing (zl_group.h)."""
    return _build_harness("zl_group_host", "group_host.cpp", ["zl_types.h", "zl_plan.h", "zl_host.h", "zl_group.h", _ZLHIP_H], _NO_CONTRACT + ["-Wall", "-Wno-unused-function"], force)


def build_overview_harness(force: bool = False) -> str:
    """The waveform overviews' column bounds, sample order and cut into pieces (zl_overview.h)."""
    return _build_harness("zl_overview_host", "overview_host.cpp", ["zl_types.h", "zl_overview.h"], ["-Wall"], force)


def build_onset_harness(force: bool = False) -> str:
    """The transient detection's level, hops, windows, select rule and refinement (zl_onset.h)."""
    return _build_harness("zl_onset_host", "onset_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h"], _NO_CONTRACT + ["-Wall", "-pthread"], force)


def build_tempo_harness(force: bool = False) -> str:
    """The tempo estimate's square root, flux, work items, order, doublings and finish (zl_tempo.h)."""
    return _build_harness("zl_tempo_host", "tempo_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_tempo.h"], _NO_CONTRACT + ["-Wall", "-pthread"], force)


def build_pitch_harness(force: bool = False) -> str:
    """The pitch detection's frames, mix, work items, pick, vote and finish (zl_pitch.h)."""
    return _build_harness("zl_pitch_host", "pitch_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h"], _NO_CONTRACT + ["-Wall", "-pthread"], force)


def build_loudness_harness(force: bool = False) -> str:
    """The loudness measurement's design, work items, a wavefront's walk over a call and the finish (zl_loudness.h)."""
    return _build_harness("zl_loudness_host", "loudness_host.cpp", ["zl_types.h", "zl_overview.h", "zl_loudness.h"], _NO_CONTRACT + ["-Wall", "-pthread"], force)


def build_loop_harness(force: bool = False) -> str:
    """The loop finder's candidates, strips, work items, a lane's register tile, the order, the pick, the finish and the seconds (zl_loop.h)."""
    return _build_harness("zl_loop_host", "loop_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h", "zl_loop.h"], _NO_CONTRACT + ["-Wall", "-pthread"], force)


def build_key_harness(force: bool = False) -> str:
    """The key detection's table, frames, work items, a lane's share of a bin, the fold and the finish (zl_key.h)."""
    return _build_harness("zl_key_host", "key_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h", "zl_key.h"], _NO_CONTRACT + ["-Wall", "-pthread"], force)


def build_xfade_harness(force: bool = False) -> str:
    """The loop crossfade's resolve, finish, weights and a call's walk workgroup by workgroup and group by group (zl_xfade.h)."""
    return _build_harness("zl_xfade_host", "xfade_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_overview.h", "zl_onset.h", "zl_pitch.h", "zl_xfade.h", _ZLHIP_H], _NO_CONTRACT + ["-Wall"], force)


def build_edit_harness(force: bool = False) -> str:
    """The clip edit's resolve, region, fades and weights and a call's walk workgroup by workgroup and group by group (zl_edit.h)."""
    return _build_harness("zl_edit_host", "edit_host.cpp", ["zl_types.h", "zl_overview.h", "zl_edit.h", _ZLHIP_H], _NO_CONTRACT + ["-Wall"], force)


def build_limit_harness(force: bool = False) -> str:
    """The peak measurement's and the limiter's resolve, window and tables and a call's walk chunk by chunk and tile by tile (zl_limit.h)."""
    return _build_harness("zl_limit_host", "limit_host.cpp", ["zl_types.h", "zl_overview.h", "zl_resample.h", "zl_limit.h", _ZLHIP_H], _NO_CONTRACT + ["-Wall"], force)


def build_warp_harness(force: bool = False) -> str:
    """The warp's resolve, plan and map and a call's walk workgroup by workgroup, the seek region by region (zl_warp.h)."""
    return _build_harness("zl_warp_host", "warp_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_warp.h", _ZLHIP_H], _NO_CONTRACT + ["-Wall"], force)


def build_decode_harness(force: bool = False) -> str:
    """The PCM upload's conversions, its cut into passes and pieces and a lane's work on one group (zl_decode.h)."""
    return _build_harness("zl_decode_host", "decode_host.cpp", ["zl_types.h", "zl_decode.h"], _NO_CONTRACT + ["-Wall"], force)


def build_resample_harness(force: bool = False) -> str:
    """The rate conversion's ratio, filter and a workgroup's walk over a call (zl_resample.h)."""
    return _build_harness("zl_resample_host", "resample_host.cpp", ["zl_types.h", "zl_resample.h"], _NO_CONTRACT + ["-Wall"], force)


def build_arena_harness(force: bool = False) -> str:
    """The source arena's allocator: first fit, coalescing, segments (zl_arena.h)."""
    return _build_harness("zl_arena_host", "arena_host.cpp", ["zl_types.h", "zl_stretch.h", "zl_arena.h"], ["-Wall"], force)


def build_launch_harness(force: bool = False) -> str:
    """Which K2 kernel a window gets, its grid, and the call's windows (zl_launch.h)."""
    return _build_harness("zl_launch_host", "launch_host.cpp", ["zl_types.h", "zl_order.h", "zl_pair.h", "zl_launch.h"], ["-Wall", "-Wno-unused-function"], force)


if __name__ == "__main__":
    force = "--force" in sys.argv
    print(build_engine(force=force, verbose=True))
    print(build_oracle(force=force))
