"""The SDF odometry (csrc/sdf.hip) against recorded results, bit for bit.

The SDF loop shares its constants, its start-up and step kernels and its host checks with the RGB-D loop (gs_gn_step.hpp); how
that code is arranged is free as long as every value it produces stays what it was: same operands, same fp32 operations in the
same order.  tests/golden/sdf_bits.npz holds what a build left behind on the MI355X for
the scenes of tests/test_sdf_odometry.py (the file holds no inputs, only results; tools/gen_golden_rgbd_bits.py records it with
the library it is given):

  seam      ops.sdf_rows_raw at 5x7 (one block, 221 of its lanes past the grid) and 30x45s2 (stride 2: 15 x 23 = 345 pixels, two
            blocks, the second partly filled), at the deltas "true" and "turned": valid, rows, sums;
  whole     ops.sdf_odometry from INIT: T and info -- 48x64 with its own schedule and with an empty middle level (its info row
            stays zero), 30x45s2, and 30x45s2 with batch element 1's depth all zero (status FEW at every level: D stays at INIT).

Packed and compared as tests/test_rgbd_bits.py does: equal bits, whatever a float's value is.
"""
import numpy as np
import pytest
import torch

from tests import test_sdf_odometry as fw
from tests.test_rgbd_bits import host, pack, same_bits

SEAM_CASES = tuple("seam.{}.{}".format(n, w) for n in ("5x7", "30x45s2") for w in ("true", "turned"))
GAP_COUNTS = (10, 0, 3)
# the transform every whole call starts from, both batch elements: a millimetre and a milliradian off the identity
INIT = np.stack([fw.make_pose(fw.rot(0.001, 0.002, -0.001), (0.003, -0.002, 0.001))] * 2).astype(np.float32)


def run_seam(name, which):
    valid, rows, sums = fw.dev_rows(name, which)
    return dict(valid=host(valid), rows=host(rows), sums=host(sums))


def run_whole(name, counts=None, zero_depth=None):
    T, info = fw.run_device(name, numiters=counts, init=fw.dev_T(INIT), zero_depth=zero_depth)
    return dict(T=host(T), info=host(info))


CASES = {**{c: (lambda c=c: run_seam(*c.split(".")[1:])) for c in SEAM_CASES},
         "whole.48x64.own": lambda: run_whole("48x64"),
         "whole.48x64.gap": lambda: run_whole("48x64", counts=GAP_COUNTS),
         "whole.30x45s2.own": lambda: run_whole("30x45s2"),
         "whole.30x45s2.few": lambda: run_whole("30x45s2", zero_depth=1)}


@pytest.fixture(scope="module")
def rec(golden):
    return golden("sdf_bits")


def test_fixture_covers_what_it_is_for(rec):
    """CPU: the recorded results show what the cases were chosen for."""
    assert all(any(k.startswith(c + ".") for k in rec) for c in CASES) and all(k.startswith(tuple(c + "." for c in CASES)) for k in rec)
    for c in SEAM_CASES:
        H, W, stride = fw.SIZES[c.split(".")[1]][:3]
        assert rec[c + ".valid"].shape == (2, -(-H // stride), -(-W // stride)), c
        assert set(np.unique(rec[c + ".valid"]).tolist()) == {0, 1}, c
        assert (rec[c + ".sums"][:, 28] == rec[c + ".valid"].sum((1, 2))).all(), c
    assert rec["seam.5x7.true.valid"][0].size == 35 and rec["seam.30x45s2.true.valid"][0].size == 345  # 1 block | 2, the second partly filled
    # a step that was applied and one that was not, in one call: FEW for element 1 at every level, D left at INIT
    few = rec["whole.30x45s2.few.info"]
    assert (few[1, :, 2] == 1).all() and (few[0, :, 2] == 0).all() and (few[1, :, 0] == 0).all()
    assert few[:, :, 3].tolist() == [list(map(float, fw.SIZES["30x45s2"][4]))] * 2
    assert same_bits(rec["whole.30x45s2.few.T"][1], INIT[1]) and not same_bits(rec["whole.30x45s2.few.T"][0], INIT[0])
    assert same_bits(rec["whole.30x45s2.few.T"][0], rec["whole.30x45s2.own.T"][0])  # the other element is unaffected
    # the empty middle level: its iteration word is 0 and its whole row stays zero
    gap = rec["whole.48x64.gap.info"]
    assert gap[:, :, 3].tolist() == [list(map(float, GAP_COUNTS))] * 2 and not gap[:, 1].any() and gap[:, 0].all(axis=0)[[0, 1, 3]].all()
    for c in ("whole.48x64.own", "whole.48x64.gap", "whole.30x45s2.own"):
        assert (rec[c + ".info"][:, :, 2] == 0).all() and not same_bits(rec[c + ".T"], INIT), c


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_sdf_matches_recorded_bits(rec, case):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    got = pack(case, CASES[case]())
    assert sorted(got) == sorted(k for k in rec if k.startswith(case + "."))
    for k, a in got.items():
        assert same_bits(a, rec[k]), k
