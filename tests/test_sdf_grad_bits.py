"""The SDF odometry's reverse pass (csrc/sdf.hip, csrc/gs_sdf_bwd.hpp, the loop's shared kernels of csrc/gs_gn_step.hpp) against
recorded results, bit for bit.

tests/test_sdf_odometry_grads.py holds these gradients to float64 autograd within a tolerance; how the code that computes them is
arranged is free as long as every value stays what it was: same operands, same fp32 operations in the same order.
tests/golden/sdf_grad_bits.npz holds what a build left behind on the MI355X for that file's seam_device and whole_device on its
smallest scenes (the file holds no inputs, only results; tools/gen_golden_rgbd_bits.py --module sdf_grad records it with the
library it is given):

  seam      ops.sdf_rows_bwd_raw of sum(sum_weights() * sums): valid and the four gradients -- 5x7 at "true" (one block, 221 of
            its lanes past the grid) and 30x45s2 at "turned" (stride 2, two blocks, the second partly filled);
  whole     ops.sdf_odometry(differentiable=True) and its backward of sum(loss_weights() * T): T, info and the four gradients --
            5x7 (one level), 30x45s2 (two levels: the 12-sum rows of one level's last pixel pass are folded by the next level's
            first step reverse), 30x45s2 with batch element 1's depth all zero (no step of it is applied: the adjoint rows are
            not live and grad_T passes through to init), 48x64 with an empty middle level, and 30x45s2 with only the depth's
            gradient wanted (no rows of the poses' adjoint, no fold: the step reverse takes its branch without them).

Packed and compared as tests/test_rgbd_bits.py does: equal bits, whatever a float's value is.
"""
import numpy as np
import pytest
import torch

from tests import test_sdf_odometry_grads as gr
from tests.test_rgbd_bits import host, pack, same_bits

WHOLE_GRADS = ("g_depth", "g_poses", "g_init", "g_tsdf")
SEAM_GRADS = ("g_depth", "g_poses", "g_D", "g_tsdf")


def run_seam(name, which):
    valid, grads = gr.seam_device(name, which)
    return dict(valid=valid, **dict(zip(SEAM_GRADS, grads)))


def run_whole(name, **kw):
    T, info, grads = gr.whole_device(name, **kw)
    return dict(T=host(T), info=host(info), **{k: host(g) for k, g in zip(WHOLE_GRADS, grads) if g is not None})


CASES = {"seam.5x7.true": lambda: run_seam("5x7", "true"),
         "seam.30x45s2.turned": lambda: run_seam("30x45s2", "turned"),
         "whole.5x7.own": lambda: run_whole("5x7"),
         "whole.30x45s2.own": lambda: run_whole("30x45s2"),
         "whole.30x45s2.few": lambda: run_whole("30x45s2", zero_depth=1),
         "whole.48x64.gap": lambda: run_whole("48x64", counts=gr.GAP_COUNTS),
         "whole.30x45s2.depth": lambda: run_whole("30x45s2", only_depth=True)}


@pytest.fixture(scope="module")
def rec(golden):
    return golden("sdf_grad_bits")


def keys_of(rec, case):
    return sorted(k[len(case) + 1:] for k in rec if k.startswith(case + "."))


def test_fixture_covers_what_it_is_for(rec):
    """CPU: the recorded results show what the cases were chosen for."""
    assert all(any(k.startswith(c + ".") for k in rec) for c in CASES) and all(k.startswith(tuple(c + "." for c in CASES)) for k in rec)
    digest = lambda k: [k + ".sha256", k + ".shape"]
    # the volume's gradient (and 48x64's depth gradient) as a digest, everything else whole; every gradient that was asked for
    for c in ("seam.5x7.true", "seam.30x45s2.turned"):
        assert keys_of(rec, c) == sorted(["valid", "g_depth", "g_poses", "g_D"] + digest("g_tsdf")), c
        assert rec[c + ".g_poses"].shape == rec[c + ".g_D"].shape == (2, 3, 4), c
    assert rec["seam.5x7.true.valid"][0].size == 35 and rec["seam.30x45s2.turned.valid"][0].size == 345  # 1 block | 2, stride 2
    for c in ("whole.5x7.own", "whole.30x45s2.own", "whole.30x45s2.few"):
        assert keys_of(rec, c) == sorted(["T", "info", "g_depth", "g_poses", "g_init"] + digest("g_tsdf")), c
    assert keys_of(rec, "whole.48x64.gap") == sorted(["T", "info", "g_poses", "g_init"] + digest("g_depth") + digest("g_tsdf"))
    assert keys_of(rec, "whole.30x45s2.depth") == ["T", "g_depth", "info"]  # nothing else was wanted
    for c in CASES:
        if c.startswith("whole."):
            name = c.split(".")[1]
            counts = gr.GAP_COUNTS if c.endswith(".gap") else gr.size_of(name)[4]
            assert rec[c + ".info"][:, :, 3].tolist() == [list(map(float, counts))] * 2, c  # (48x64.gap: the empty middle level)
            assert rec[c + ".T"].shape == (2, 4, 4) and (rec[c + ".info"][0, :, 2] == 0).all(), c
        for k in keys_of(rec, c):
            if k.startswith("g_") and not k.endswith((".sha256", ".shape")):
                assert np.isfinite(rec[c + "." + k]).all() and rec[c + "." + k][0].any(), (c, k)
    assert len(gr.size_of("30x45s2")[4]) == 2 and len(gr.size_of("5x7")[4]) == 1  # two levels | one
    # steps that were applied and steps that were not, in one call: FEW for element 1 at every level, its T left at the
    # identity, its gradients zero but init's, which is grad_T's rows 0..2 handed through bit for bit; element 0 is unaffected
    few, own = "whole.30x45s2.few.", "whole.30x45s2.own."
    assert (rec[few + "info"][1, :, 2] == 1).all() and (rec[few + "info"][1, :, 0] == 0).all()
    assert same_bits(rec[few + "T"][1], np.eye(4, dtype=np.float32))
    assert same_bits(rec[few + "g_init"][1, :3], gr.loss_weights()[1].astype(np.float32)) and not rec[few + "g_init"][1, 3].any()
    assert not rec[few + "g_depth"][1].any() and not rec[few + "g_poses"][1].any()
    assert not same_bits(rec[own + "g_init"][1, :3], gr.loss_weights()[1].astype(np.float32)) and rec[own + "g_depth"][1].any()
    for k in ("T", "g_depth", "g_poses", "g_init"):
        assert same_bits(rec[few + k][0], rec[own + k][0]), k
    assert not same_bits(rec[few + "g_tsdf.sha256"], rec[own + "g_tsdf.sha256"])
    # with only the depth wanted, its gradient and the forward keep their bits
    for k in ("T", "info", "g_depth"):
        assert same_bits(rec["whole.30x45s2.depth." + k], rec[own + k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_sdf_gradients_match_recorded_bits(rec, case):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    got = pack(case, CASES[case]())
    assert sorted(got) == sorted(k for k in rec if k.startswith(case + "."))
    for k, a in got.items():
        assert same_bits(a, rec[k]), k
