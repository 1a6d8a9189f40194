"""largest |difference| and ULP distance between the contraction-off and the -mfma -ffp-contract=fast build of the reference voice, per fixture scene"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from libzl_amd import build as b
import ref_voice as rv, reference_scenes as rs
off, fast = b.build_reference(), b.build_reference(contracted=True)
def ulps(a, c):
    ai, ci = a.view(np.int32).astype(np.int64), c.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7fffffff), ai); ci = np.where(ci < 0, -(ci & 0x7fffffff), ci)
    return np.abs(ai - ci)
for name, make in rs.FIXTURES.items():
    x = rv.run_reference(make(), off)["ref"]["bus"]; y = rv.run_reference(make(), fast)["ref"]["bus"]
    ok = np.isfinite(x) & np.isfinite(y)
    d = np.abs(x[ok].astype(np.float64) - y[ok]); u = ulps(x[ok], y[ok])
    print(f"| {name} | {(u > 0).mean() * 100:.1f} % | {d.max():.3g} | {int(u.max())} | {np.abs(x[ok]).max():.3g} |")
