#!/usr/bin/env python3
"""Records tests/golden/rgbd_bits.npz, tests/golden/sdf_bits.npz or tests/golden/sdf_grad_bits.npz: what the cases of
tests/test_rgbd_bits.py (CASES: the pyramid, the seam and the whole call with its reverse pass, on the scenes of
tests/test_rgbd_odometry.py), of tests/test_sdf_bits.py (CASES: the seam and the whole call, on the scenes of
tests/test_sdf_odometry.py) or of tests/test_sdf_grad_bits.py (CASES: the reverse pass of the seam and of the whole call, as
tests/test_sdf_odometry_grads.py's seam_device and whole_device run them) leave behind, packed as test_rgbd_bits' `pack` packs
them -- small arrays whole, large ones as SHA-256 and shape.  Run it on an MI355X with the library whose bits are to be pinned;
every case is run twice and must repeat itself.

    python3 tools/gen_golden_rgbd_bits.py [--module rgbd|sdf|sdf_grad] [LIBRARY] [OUT.npz]

LIBRARY is the libgradslam_hip.so to record (default: the in-tree build).  rgbd_bits.npz in the repository was recorded with the
library built from the commit before the pixel's arithmetic moved into gs_rgbd_pixel.hpp (d13c0fa); sdf_bits.npz with the library
built from the commit before the loops' shared parts moved into gs_gn_step.hpp (9ff1be4); sdf_grad_bits.npz with the library
built from the commit before the loops' kernels moved there too (fb7fd6c).
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gradslam_amd import _native  # noqa: E402

args = sys.argv[1:]
module = "rgbd"
if args and args[0] == "--module":
    module, args = args[1], args[2:]
assert module in ("rgbd", "sdf", "sdf_grad"), module
if len(args) > 0:
    _native.LIB_PATH = os.path.abspath(args[0])  # before the first call loads it
from tests.test_rgbd_bits import pack, same_bits  # noqa: E402

S = importlib.import_module("tests.test_{}_bits".format(module))
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "tests", "golden", module + "_bits.npz")
out = {}
for case, run in S.CASES.items():
    r, again = pack(case, run()), pack(case, run())
    assert sorted(r) == sorted(again), case
    assert all(same_bits(r[k], again[k]) for k in r), [k for k in r if not same_bits(r[k], again[k])]
    out.update(r)
    print(case, sorted(k[len(case) + 1:] for k in r))
np.savez_compressed(out_path, **out)
print("recorded", _native.LIB_PATH, "->", out_path, os.path.getsize(out_path), "bytes")
