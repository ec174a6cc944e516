#!/usr/bin/env python3
"""Records tests/golden/rgbd_bits.npz: what the cases of tests/test_rgbd_bits.py (CASES: the pyramid, the seam and the whole call
with its reverse pass, on the scenes of tests/test_rgbd_odometry.py) leave behind, packed as that file's `pack` packs them --
small arrays whole, large ones as SHA-256 and shape.  Run it on an MI355X with the library whose bits are to be pinned; every
case is run twice and must repeat itself.

    python3 tools/gen_golden_rgbd_bits.py [LIBRARY] [OUT.npz]

LIBRARY is the libgradslam_hip.so to record (default: the in-tree build).  The file in the repository was recorded with the
library built from the commit before the pixel's arithmetic moved into gs_rgbd_pixel.hpp (d13c0fa).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gradslam_amd import _native  # noqa: E402

if len(sys.argv) > 1:
    _native.LIB_PATH = os.path.abspath(sys.argv[1])  # before the first call loads it
from tests import test_rgbd_bits as S  # noqa: E402

out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "rgbd_bits.npz")
out = {}
for case, run in S.CASES.items():
    r, again = S.pack(case, run()), S.pack(case, run())
    assert sorted(r) == sorted(again), case
    assert all(S.same_bits(r[k], again[k]) for k in r), [k for k in r if not S.same_bits(r[k], again[k])]
    out.update(r)
    print(case, sorted(k[len(case) + 1:] for k in r))
np.savez_compressed(out_path, **out)
print("recorded", _native.LIB_PATH, "->", out_path, os.path.getsize(out_path), "bytes")
