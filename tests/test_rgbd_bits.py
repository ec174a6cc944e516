"""The dense RGB-D odometry (csrc/rgbd.hip) against recorded results, bit for bit.

The forward kernel and the reverse pass must take the same decisions for every pixel, so the pixel's arithmetic is stated once
(gs_rgbd_pixel.hpp) -- and how the code is arranged is free as long as every value it produces stays what it was: same operands,
same fp32 operations in the same order.  tests/golden/rgbd_bits.npz holds what a build left behind on the MI355X for the scenes
of tests/test_rgbd_odometry.py (the file holds no inputs, only results; tools/gen_golden_rgbd_bits.py records it with the
library it is given):

  pyramid   gs_rgbd_pyramid, both frames of 30x45 at 2 levels (an odd width: the last column is dropped; the sphere's rim: blocks
            that lose a depth to depth_diff_max);
  seam      gs_rgbd_rows and gs_rgbd_rows_bwd at 5x7 and 30x45, at the transforms "true" and "outside": valid, rows, sums and the
            five gradients of sum(sum_weights() * sums);
  whole     ops.rgbd_odometry(differentiable=True) and its backward of sum(loss_weights() * T): T, info, the tape, the five
            gradients, and the plain call's T and info -- 30x45 with its own schedule, 48x64 with an empty middle level, 30x45 with
            batch element 1's source depth all zero (status FEW: steps that are not applied).

An array of at most WHOLE_MAX bytes is stored whole, a larger one as the SHA-256 of its bytes and its shape: 30x45's one- and
two-word per-pixel arrays are whole; its 14-word rows and 3-word colour gradients, and everything per pixel at 48x64, are
digests.  Comparisons are on the bytes or on the digests: equal bits, whatever a float's value is.
"""
import hashlib

import numpy as np
import pytest
import torch

from tests import test_rgbd_odometry as fw
from tests.test_rgbd_odometry_grads import GAP_COUNTS, loss_weights, sum_weights

DEV = "cuda:0"
WHOLE_MAX = 22 * 1024
SEAM_CASES = tuple("seam.{}.{}".format(n, w) for n in ("5x7", "30x45") for w in ("true", "outside"))
GRADS = ("g_td", "g_tc", "g_sd", "g_sc")
# gs_rgbd_pixel.hpp: a tape row's stride, the words of it the step writes (the rest is padding that holds whatever the allocation
# held), and its word "the step was applied"
TAPE_WORDS, TAPE_WRITTEN, TAPE_APPLIED = 64, 52, 51


def host(t):
    return t.detach().cpu().contiguous().numpy()


def run_pyramid():
    from gradslam_amd import ops

    t = fw.dev_scene("30x45")
    out = {}
    for frame, (d, c) in (("target", ("td", "tc")), ("source", ("sd", "sc"))):
        for l, p in enumerate(ops.rgbd_pyramid_raw(t[d], t[c], 2)):
            out["{}.level{}".format(frame, l)] = host(p)
    return out


def run_seam(name, which):
    from gradslam_amd import ops

    t = fw.dev_scene(name)
    T = fw.dev_T(fw.transforms(name)[which])
    g_sums = torch.from_numpy(sum_weights().astype(np.float32)).to(DEV)
    valid, rows, sums = ops.rgbd_rows_raw(t["td"], t["tc"], t["sd"], t["sc"], t["K"], T)
    grads = ops.rgbd_rows_bwd_raw(t["td"], t["tc"], t["sd"], t["sc"], t["K"], T, g_sums)
    out = dict(valid=host(valid), rows=host(rows), sums=host(sums))
    out.update({k: host(g) for k, g in zip(GRADS + ("g_T",), grads)})
    return out


def run_whole(name, counts=None, zero_source=None):
    from gradslam_amd import ops

    _, _, levels, numiters = fw.SIZES[name]
    t = fw.dev_scene(name)
    if zero_source is not None:
        t["sd"] = t["sd"].clone()
        t["sd"][zero_source] = 0.0
    eye = torch.eye(4, device=DEV).repeat(2, 1, 1)
    kw = dict(numiters=counts or numiters, levels=levels)
    T_plain, info_plain = ops.rgbd_odometry(t["td"], t["tc"], t["sd"], t["sc"], t["K"], init=eye, **kw)
    leaves = [x.clone().requires_grad_(True) for x in (t["td"], t["tc"], t["sd"], t["sc"], eye)]
    T, info = ops.rgbd_odometry(*leaves[:4], t["K"], init=leaves[4], differentiable=True, **kw)
    n = 2 * sum(kw["numiters"])  # rows: one per iteration and batch element, in the order the iterations ran
    tape = T.grad_fn.saved_tensors[5][:n * TAPE_WORDS].view(n // 2, 2, TAPE_WORDS)[..., :TAPE_WRITTEN].clone()
    W = torch.from_numpy(loss_weights().astype(np.float32)).to(DEV)
    (W * T[:, :3]).sum().backward()
    out = dict(T=host(T), info=host(info), tape=host(tape), T_plain=host(T_plain), info_plain=host(info_plain))
    out.update({k: host(x.grad) for k, x in zip(GRADS + ("g_init",), leaves)})
    return out


CASES = {"pyramid.30x45": run_pyramid,
         **{c: (lambda c=c: run_seam(*c.split(".")[1:])) for c in SEAM_CASES},
         "whole.30x45.own": lambda: run_whole("30x45"),
         "whole.48x64.gap": lambda: run_whole("48x64", counts=GAP_COUNTS),
         "whole.30x45.few": lambda: run_whole("30x45", zero_source=1)}


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def pack(case, arrays):
    """What the fixture holds for one case: `case.key` whole, or `case.key.sha256` and `case.key.shape`."""
    out = {}
    for k, a in arrays.items():
        if a.nbytes <= WHOLE_MAX:
            out[case + "." + k] = a
        else:
            out[case + "." + k + ".sha256"] = digest(a)
            out[case + "." + k + ".shape"] = np.array(a.shape, dtype=np.int64)
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def rec(golden):
    return golden("rgbd_bits")


def test_fixture_covers_what_it_is_for(rec):
    """CPU: the recorded results show what the cases were chosen for."""
    assert all(any(k.startswith(c + ".") for k in rec) for c in CASES) and all(k.startswith(tuple(c + "." for c in CASES)) for k in rec)
    # a step that was applied and one that was not, on one tape
    tape = rec["whole.30x45.few.tape"]
    assert tape.shape == (sum(fw.SIZES["30x45"][3]), 2, TAPE_WRITTEN)
    assert (tape[:, 0, TAPE_APPLIED] == 1).all() and (tape[:, 1, TAPE_APPLIED] == 0).all()
    assert (rec["whole.30x45.few.info"][1, :, 2] == 1).all() and (rec["whole.30x45.few.info"][0, :, 2] == 0).all()
    assert rec["whole.48x64.gap.info"][:, :, 3].tolist() == [list(map(float, GAP_COUNTS))] * 2  # the empty middle level
    for c in ("whole.30x45.own", "whole.48x64.gap", "whole.30x45.few"):  # the taped forward's bits are the plain call's
        assert same_bits(rec[c + ".T"], rec[c + ".T_plain"]) and same_bits(rec[c + ".info"], rec[c + ".info_plain"]), c
    for c in SEAM_CASES:
        assert set(np.unique(rec[c + ".valid"]).tolist()) == {0, 1}, c
    # the pyramid: a level-1 pixel whose 2 x 2 block lost a positive depth to depth_diff_max -- its depth is the mean of fewer
    # values than the block has positive ones -- and the odd width's last column, which no block holds
    ddm = np.float32(fw.DDM)
    for frame in ("target", "source"):
        d0, d1 = rec["pyramid.30x45.{}.level0".format(frame)][..., 1], rec["pyramid.30x45.{}.level1".format(frame)][..., 1]
        assert d0.shape == (2, 30, 45) and d1.shape == (2, 15, 22)
        blk = d0[:, :30, :44].reshape(2, 15, 2, 22, 2).transpose(0, 1, 3, 2, 4).reshape(2, 15, 22, 4)
        dmin = np.where(blk > 0, blk, np.inf).min(-1, keepdims=True)
        lost = ((blk > 0) & ~(blk - dmin <= ddm)).any(-1)
        assert lost.sum() >= 4 and (d1[lost] > 0).all() and (d1[lost] < blk.max(-1)[lost]).all(), frame


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_rgbd_matches_recorded_bits(rec, case):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    got = pack(case, CASES[case]())
    assert sorted(got) == sorted(k for k in rec if k.startswith(case + "."))
    for k, a in got.items():
        assert same_bits(a, rec[k]), k
