#!/usr/bin/env python3
"""Records tests/golden/step_chain.npz: for the three scenes of tests/test_step_chain.py (make_scenes) the inputs and what
gs_icp_point_to_plane leaves behind -- pose, trace rows, both state copies, as int32 words.  Run it on an MI355X with the build
whose bits are to be pinned (the file in the repository was recorded with the build of the commit before the step's chain was
reordered); every scene is run twice and must repeat itself.

    python3 tools/gen_golden_step_chain.py [OUT.npz]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_step_chain as S  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_chain.npz")
out = {}
for name, sc in S.make_scenes().items():
    r = S.run_point_to_plane(sc["src"], sc["tgt"], sc["nrm"], sc["damp"])
    again = S.run_point_to_plane(sc["src"], sc["tgt"], sc["nrm"], sc["damp"])
    for k in r:
        assert torch.equal(r[k], again[k]), (name, k)
    for k in ("src", "tgt", "nrm"):
        out[name + "." + k] = sc[k].numpy()
    out[name + ".damp"] = np.float32(sc["damp"])
    for k in r:
        out[name + "." + k] = r[k].numpy()
    print(name, "accepted", r["trace"].view(torch.float32)[:, 45].tolist())
np.savez(out_path, **out)
print("wrote", out_path, os.path.getsize(out_path), "bytes")
