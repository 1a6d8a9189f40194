"""The owners of the engine's HIP resources (libzl_amd/csrc/zl_owned.h), CPU tier: tests/cpp/owned_check.cpp compiles the header against
a stand-in for the HIP calls it makes and walks every owner's life, the growth rules and every failure point of a mixed sequence under
AddressSanitizer and UBSan.  tests/test_engine_lifecycle.py holds the engine to a balanced life on the GPU."""
import os
import subprocess

from libzl_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_owner_under_the_sanitizers(tmp_path):
    """Construct, move, self-move, reset and destruct of each owner; "free, then allocate" and the empty state after a failed growth; a
    sequence of mixed allocations with its k-th creating call failing, for every k: the stand-in's live count and the owners' four are
    0 at the end.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the environment
    loads in front of it; a leak ends it too (LeakSanitizer at exit)."""
    exe = str(tmp_path / "owned_check")
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-isystem", hip_include,
                           os.path.join(ROOT, "tests", "cpp", "owned_check.cpp"), "-o", exe])
    rc = subprocess.run([exe], capture_output=True, text=True)
    assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
    assert "owned check ok" in rc.stdout
