"""The reverse pass of the dense RGB-D odometry (csrc/rgbd.hip: gs_rgbd_odometry_taped, gs_rgbd_odometry_bwd, gs_rgbd_rows_bwd;
ops.rgbd_odometry(differentiable=True), ops.rgbd_rows_bwd_raw; RGBDOdometryProvider(differentiable=True);
KinectFusion(odom="rgbd", odom_gradients=True, pose_gradients=True)).

The reference is tests/rgbd_grad_reference.py: a torch transcription of the rule of include/gradslam_hip.h, the decisions held
constant, differentiated by torch autograd.  float64 autograd is the reference.  float32 autograd of the same code measures what
fp32 alone costs (in autograd's order of operations, not the device's): WHOLE_DEVIATION, SEAM_DEVIATION and SEAM_GT_96 below
hold, per differentiable input, max |g32 - g64| over the input divided by the largest |g64| entry of that input -- measured on
the CPU, recomputed and asserted by test_recorded_deviations_are_what_the_float32_transcription_gives, never taken from the
device -- and the device must agree with float64 within FOUR times those, normalised the same way.  Scenes, sizes and the numpy
references of the forward pass are tests/test_rgbd_odometry.py's.

At the seam fp32 and float64 must take the same decisions: the source depth is first zeroed at the pixels that file's `left_out`
rule marks as float64 sees them (at most 5 %), and the device's valid flags on the edited input must equal the reference's.
"""
import ctypes
import os
import re
from functools import lru_cache

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops
from gradslam_amd.odometry import RGBDOdometryProvider
from tests import rgbd_grad_reference as ref
from tests import test_rgbd_odometry as fw

DEV = "cuda:0"
NEW_SYMBOLS = {"gs_rgbd_odometry_tape_size": 3, "gs_rgbd_odometry_taped": 21, "gs_rgbd_odometry_bwd_ws_size": 5,
               "gs_rgbd_odometry_bwd": 24, "gs_rgbd_rows_bwd": 21}
WHOLE_SIZES = ("48x64", "30x45")
SEAM_SIZES = ("48x64", "30x45", "5x7")
SEAM_TRANSFORMS = ("true", "outside")  # not the identity: there every pixel ties
INPUTS = ("td", "tc", "sd", "sc", "T")  # target depth, target rgb, source depth, source rgb, init / T (rows 0..2)
# 48x64: a level with zero iterations between levels that have some -- the reverse driver skips the level and carries the
# 12-sum rows and the tape position across it.  The schedule has to converge: a loop that has not converged amplifies every
# validity flip, and float32 autograd of the transcription is then 0.1 to 1.6 of the largest entry away from float64 ((3, 0, 2),
# (10, 0, 5), (8, 0, 6), (6, 0, 6), (10, 0, 3)), whatever the gap; with (10, 0, 10) it deviates as it does for (10, 5, 3).
GAP_COUNTS = (10, 0, 10)

# max |g32 - g64| / max |g64| per input (INPUTS' order), the larger of the two batch elements; see the module docstring
WHOLE_DEVIATION = {"48x64": (4.5e-4, 4.2e-4, 4.2e-4, 3.6e-4, 1.7e-5), "30x45": (6.8e-5, 9.2e-5, 7.3e-5, 1.0e-4, 6.5e-6)}
GAP_DEVIATION = (4.3e-4, 4.0e-4, 4.1e-4, 3.5e-4, 1.6e-5)  # 48x64 with GAP_COUNTS
# per transform, over SEAM_SIZES and the batch elements
SEAM_DEVIATION = {"true": (3.9e-6, 6.5e-6, 8.3e-6, 3.0e-6, 1.9e-6), "outside": (4.6e-6, 1.1e-5, 6.4e-6, 4.0e-6, 3.8e-6)}
# g_T alone at 96x130 (49 blocks: more than one partial row per fold group)
SEAM_GT_96 = {"true": 3.7e-6, "outside": 1.2e-5}


# What the two size queries return, pinned as tests/golden/ws_sizes.json pins the older ones (a size that drifts changes
# allocations): [arguments, bytes], the shapes of tools/gen_golden_ws_sizes.py's scenarios.
RECORDED_SIZES = {
    "gs_rgbd_odometry_tape_size": [[[1, 1, 0], 256], [[1, 3, 10], 2560], [[2, 3, 3], 1536], [[1, 3, 2], 512], [[1, 3, -1], 0], [[0, 3, 2], 0]],
    "gs_rgbd_odometry_bwd_ws_size": [[[1, 1, 1, 1, 0], 0], [[1, 120, 160, 3, 10], 1503488], [[2, 48, 64, 3, 3], 481792],
                                     [[1, 480, 640, 3, 10], 24020992], [[1, 12, 16, 3, 2], 0], [[1, 12, 16, 3, -1], 0], [[0, 12, 16, 3, 2], 0],
                                     [[1, 1024, 1024, 3, 2], 81986304], [[1, 1024, 1025, 3, 2], 82056192]],
}


# ------------------------------------------------------------------ the reference's inputs and gradients
def loss_weights(B=2):
    return np.random.default_rng(7).standard_normal((B, 3, 4))


def sum_weights(B=2):
    return np.random.default_rng(11).standard_normal((B, 29))


def frames(name, b):
    s = fw.scene(name)
    return [s[k][b] for k in ("td", "tc", "sd", "sc")]


@lru_cache(maxsize=None)
def whole_reference(name, dt_name, counts=None):
    """Per batch element: (T (3,4), {input: gradient}) of sum(W * T) through the whole loop from init = the identity."""
    dt = getattr(torch, dt_name)
    _, _, levels, numiters = fw.SIZES[name]
    out = []
    for b in range(2):
        td, tc, sd, sc, init = ref.leaves(frames(name, b) + [np.eye(4)[:3]], dt)
        T = ref.odometry(td, tc, sd, sc, fw.scene(name)["K"], levels, counts or numiters, dt, init=init)
        (torch.tensor(loss_weights()[b], dtype=dt) * T).sum().backward()
        out.append((T.detach().double().numpy(), {k: t.grad.double().numpy() for k, t in zip(INPUTS, (td, tc, sd, sc, init))}))
    return out


@lru_cache(maxsize=None)
def seam_frames(name, which, b):
    """The frames with the source depth zeroed where float64 sees a tie, and that mask."""
    td, tc, sd, sc = frames(name, b)
    out = fw.left_out(fw.rows_reference(name, which, b)[0][2])
    assert out.mean() <= 0.05, (name, which, b, float(out.mean()))
    sd = sd.copy()
    sd[out] = 0.0
    return td, tc, sd, sc


@lru_cache(maxsize=None)
def seam_reference(name, which, dt_name):
    """Per batch element: (sums (29), {input: gradient}, valid mask, mask of the target pixels a valid pixel's cell touches)."""
    dt = getattr(torch, dt_name)
    H, W = fw.scene(name)["H"], fw.scene(name)["W"]
    out = []
    for b in range(2):
        td, tc, sd, sc, T = ref.leaves(list(seam_frames(name, which, b)) + [fw.transforms(name)[which][b][:3]], dt)
        sums, (vs, us, i, j) = ref.seam(td, tc, sd, sc, fw.scene(name)["K"], T, dt)
        (torch.tensor(sum_weights()[b, :28], dtype=dt) * sums[:28]).sum().backward()
        valid, touched = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
        valid[vs.numpy(), us.numpy()] = True
        for dj, di in ((0, 0), (0, 1), (1, 0), (1, 1)):
            touched[j.numpy() + dj, i.numpy() + di] = True
        out.append((sums.detach().double().numpy(), {k: t.grad.double().numpy() for k, t in zip(INPUTS, (td, tc, sd, sc, T))}, valid, touched))
    return out


def deviation(got, want):
    """max |got - want| / max |want| per input."""
    return [float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in INPUTS]


def measure_constants():
    """What the recorded constants were measured with (python -c "import tests.test_rgbd_odometry_grads as t; print(t.measure_constants())")."""
    worst = lambda rows: tuple(max(r[k] for r in rows) for k in range(len(rows[0])))
    whole = {n: worst([deviation(whole_reference(n, "float32")[b][1], whole_reference(n, "float64")[b][1]) for b in range(2)]) for n in WHOLE_SIZES}
    gap = worst([deviation(whole_reference("48x64", "float32", GAP_COUNTS)[b][1], whole_reference("48x64", "float64", GAP_COUNTS)[b][1])
                 for b in range(2)])
    seam = {w: worst([deviation(seam_reference(n, w, "float32")[b][1], seam_reference(n, w, "float64")[b][1]) for n in SEAM_SIZES for b in range(2)])
            for w in SEAM_TRANSFORMS}
    gt96 = {w: max(deviation(seam_reference("96x130", w, "float32")[b][1], seam_reference("96x130", w, "float64")[b][1])[4] for b in range(2))
            for w in SEAM_TRANSFORMS}
    return whole, gap, seam, gt96


# ------------------------------------------------------------------ CPU: ABI, contracts, the reference itself
def test_new_symbols_load_and_are_declared():
    lib = nv.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^)]*)\);", header, flags=re.M)  # (the comments name the functions too)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
    for name, nargs in fw.NEW_SYMBOLS.items():  # the existing entry points keep their argument counts
        assert len(nv.SIGNATURES[name][1]) == nargs, name
    assert lib.gs_abi_version() == 3
    assert hasattr(ops, "rgbd_rows_bwd_raw")


@pytest.mark.parametrize("name", sorted(RECORDED_SIZES))
def test_size_queries_return_what_was_recorded(name):
    fn = getattr(nv.lib(), name)
    assert [[args, int(fn(*args))] for args, _ in RECORDED_SIZES[name]] == RECORDED_SIZES[name]


def test_new_entry_points_refuse_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    lib = nv.lib()
    P = 4096
    inf, nan = float("inf"), float("nan")
    align = lambda n: -(-n // 256) * 256
    assert lib.gs_rgbd_odometry_tape_size(2, 3, 18) == 256 * 2 * 18 and lib.gs_rgbd_odometry_tape_size(1, 1, 0) == 256
    for bad in ((0, 3, 18), (65536, 3, 18), (1, 0, 1), (1, 9, 1), (1, 3, -1), (1, 1, (1 << 20) + 1)):
        assert lib.gs_rgbd_odometry_tape_size(*bad) == 0, bad
    pix = 48 * 64 + 24 * 32 + 12 * 16
    want = (align(64 * 2) + align(128 * 2 * 18) + align(48 * 12 * 2) + 2 * align(8 * pix * 2) + align(16 * pix * 2)
            + 256 + align(4 * 2 * 48 * 64) + align(32 * 2 * 48 * 64))
    assert lib.gs_rgbd_odometry_bwd_ws_size(2, 48, 64, 3, 18) == want
    assert lib.gs_rgbd_odometry_bwd_ws_size(2, 48, 64, 3, 0) == lib.gs_rgbd_odometry_bwd_ws_size(2, 48, 64, 3, 1)
    for bad in ((0, 48, 64, 3, 1), (1, 48, 64, 0, 1), (1, 48, 64, 5, 1), (1, 3, 64, 1, 1), (1, 8192, 4096, 1, 1), (1, 48, 64, 3, -1)):
        assert lib.gs_rgbd_odometry_bwd_ws_size(*bad) == 0, bad
    assert lib.gs_rgbd_odometry_ws_bytes(2, 48, 64, 3) == align(64 * 2) + align(116 * 12 * 2) + 2 * align(8 * pix * 2)  # as it was

    counts = (ctypes.c_int * 3)(2, 1, 1)
    #     td tc sd sc B  H   W   K  init L  counts  lam  ddm   damp  scale T  info ws  bytes    stream tape
    ok = [P, P, P, P, 1, 48, 64, P, P, 3, counts, 0.9, 0.07, 1e-8, 1.0, P, P, P, 1 << 24, None, P]
    for pos in (0, 1, 2, 3, 7, 10, 15, 16, 20):  # (init may be NULL: the identity)
        args = list(ok)
        args[pos] = None
        assert lib.gs_rgbd_odometry_taped(*args) == -1, pos
    for pos, bad in ((4, 0), (5, 0), (6, 15), (9, 0), (9, 5), (11, 1.01), (11, nan), (12, 0.0), (12, inf), (13, -1e-8), (14, nan),
                     (10, (ctypes.c_int * 3)(2, -1, 1))):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_rgbd_odometry_taped(*args) == -1, (pos, bad)
    assert b"gs_rgbd_odometry_taped" in lib.gs_last_error()
    args = list(ok)
    args[18] = lib.gs_rgbd_odometry_ws_bytes(1, 48, 64, 3) - 1
    assert lib.gs_rgbd_odometry_taped(*args) == -2

    #     td tc sd sc B  H   W   K  L  counts  lam  ddm   damp  scale tape gT g_td g_tc g_sd g_sc g_init ws bytes   stream
    ok = [P, P, P, P, 1, 48, 64, P, 3, counts, 0.9, 0.07, 1e-8, 1.0, P, P, P, P, P, P, P, P, 1 << 26, None]
    for pos in (0, 1, 2, 3, 7, 9, 14, 15):  # (any of the five outputs may be NULL)
        args = list(ok)
        args[pos] = None
        assert lib.gs_rgbd_odometry_bwd(*args) == -1, pos
    for pos, bad in ((4, 0), (4, 65536), (5, 0), (6, 15), (8, 0), (8, 5), (8, 9), (10, -0.01), (10, nan), (11, 0.0), (11, nan), (12, -1.0),
                     (12, inf), (13, inf), (9, (ctypes.c_int * 3)(2, 1, -5))):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_rgbd_odometry_bwd(*args) == -1, (pos, bad)
    assert b"gs_rgbd_odometry_bwd" in lib.gs_last_error()
    args = list(ok)
    args[22] = lib.gs_rgbd_odometry_bwd_ws_size(1, 48, 64, 3, 4) - 1
    assert lib.gs_rgbd_odometry_bwd(*args) == -2
    args = list(ok)
    args[21], args[22] = None, 0
    assert lib.gs_rgbd_odometry_bwd(*args) == -2

    #     td tc sd sc B  H   W   K  T  lam  ddm   scale g_sums g_td g_tc g_sd g_sc g_T ws bytes    stream
    ok = [P, P, P, P, 1, 48, 64, P, P, 0.9, 0.07, 1.0, P, P, P, P, P, P, P, 1 << 26, None]
    for pos in (0, 1, 2, 3, 7, 8, 12):
        args = list(ok)
        args[pos] = None
        assert lib.gs_rgbd_rows_bwd(*args) == -1, pos
    for pos, bad in ((4, 0), (5, 3), (6, -4), (9, -0.5), (9, nan), (10, 0.0), (10, inf), (11, nan)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_rgbd_rows_bwd(*args) == -1, (pos, bad)
    assert b"gs_rgbd_rows_bwd" in lib.gs_last_error()
    args = list(ok)
    args[19] = lib.gs_rgbd_odometry_bwd_ws_size(1, 48, 64, 1, 1) - 1
    assert lib.gs_rgbd_rows_bwd(*args) == -2


def test_provider_and_ops_contracts():
    with pytest.raises(TypeError, match="differentiable"):
        RGBDOdometryProvider(differentiable=1)
    assert RGBDOdometryProvider().differentiable is False
    fr = fw.cpu_frames()
    grad = gs.RGBDImages(fr.rgb_image, fr.depth_image.clone().requires_grad_(True), fr.intrinsics)
    with pytest.raises(NotImplementedError, match="gradients"):  # the default provider still refuses
        RGBDOdometryProvider(2, levels=1).provide(fr, grad)
    diff = RGBDOdometryProvider(2, levels=1, differentiable=True)
    for cf in (False, True):
        f = fw.cpu_frames(channels_first=cf)
        g = gs.RGBDImages(f.rgb_image, f.depth_image.clone().requires_grad_(True), f.intrinsics, channels_first=cf)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            diff.provide(fw.cpu_frames(channels_first=cf), g)
    d, c, K = fr.depth_image[:, 0], fr.rgb_image[:, 0], fr.intrinsics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgbd_odometry(d.clone().requires_grad_(True), c, d, c, K, levels=1, numiters=1, differentiable=True)
    # the intrinsics are not differentiable: with differentiable=True refused, not cut silently
    Kg = K.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="intrinsics"):
        ops.rgbd_odometry(d, c, d, c, Kg, levels=1, numiters=1, differentiable=True)
    with pytest.raises(NotImplementedError, match="intrinsics"):
        diff.provide(gs.RGBDImages(fr.rgb_image, fr.depth_image, Kg), gs.RGBDImages(fr.rgb_image, fr.depth_image, Kg))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (the plain call detaches them, as it did)
        ops.rgbd_odometry(d, c, d, c, Kg, levels=1, numiters=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgbd_rows_bwd_raw(d, c, d, c, K, torch.eye(4).view(1, 4, 4), torch.zeros(1, 29))
    with pytest.raises(ValueError, match="g_sums"):
        ops.rgbd_rows_bwd_raw(d, c, d, c, K, torch.eye(4).view(1, 4, 4), torch.zeros(1, 28))
    from gradslam_amd.slam import KinectFusion

    kw = dict(dims=(8, 8, 8), voxel_size=0.1, device="cuda:0", odom="rgbd")
    assert KinectFusion(odom_gradients=True, **kw).odomprov.differentiable is True
    assert KinectFusion(odom_gradients=True, pose_gradients=True, **kw).odomprov.differentiable is True
    assert KinectFusion(**kw).odomprov.differentiable is False
    assert KinectFusion(pose_gradients=True, **kw).odomprov.differentiable is False  # as it was: the refusal stays
    with pytest.raises(TypeError, match="odom_gradients"):
        KinectFusion(odom_gradients=1, **kw)
    with pytest.raises(ValueError, match="odom_gradients"):
        KinectFusion(**{**kw, "odom": "icp"}, odom_gradients=True)


@pytest.mark.parametrize("name", WHOLE_SIZES)
def test_float64_transcription_forward_equals_the_numpy_reference(name):
    for b in range(2):
        T = whole_reference(name, "float64")[b][0]
        assert np.abs(T - fw.odometry_reference(name, b)[0][:3]).max() <= 1e-12
    T = whole_reference("48x64", "float64", GAP_COUNTS)[0][0]
    s = fw.scene("48x64")
    want = fw.ref_odometry(s["td"][0], s["tc"][0], s["sd"][0], s["sc"][0], s["K"], 3, GAP_COUNTS, np.float64)[0]
    assert np.abs(T - want[:3]).max() <= 1e-12


@pytest.mark.parametrize("which", SEAM_TRANSFORMS)
@pytest.mark.parametrize("name", SEAM_SIZES)
def test_float64_transcription_sums_equal_the_numpy_reference(name, which):
    s = fw.scene(name)
    for b in range(2):
        td, tc, sd, sc = seam_frames(name, which, b)
        sums, _, valid, _ = seam_reference(name, which, "float64")[b]
        (tI, tD), (sI, sD) = fw.ref_level0(td, tc, np.float64), fw.ref_level0(sd, sc, np.float64)
        ok, rows, _ = fw.ref_rows(tI, tD, sI, sD, fw.level_K(s["K"], 0, np.float64), fw.transforms(name)[which][b], np.float64)
        want = fw.sums29(rows, ok, np.float64)
        assert np.array_equal(ok, valid)
        assert (np.abs(sums - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (name, which, b)


def directional(fn, xs, rng):
    """(autograd's, central differences') derivative of the scalar fn(xs, decisions) along one random direction of all inputs,
    float64, h = 1e-5 of each input's scale, the base run's decisions replayed at the two displaced points."""
    dec = ref.Decisions()
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    fn(xs, dec).backward()
    dirs = [torch.from_numpy(rng.standard_normal(tuple(x.shape))) for x in xs]
    dirs = [d / d.norm() * float(x.detach().abs().max()) for d, x in zip(dirs, xs)]  # unit directions, in the input's scale
    ad = sum(float((x.grad * d).sum()) for x, d in zip(xs, dirs))
    h = 1e-5
    with torch.no_grad():
        up = float(fn([x + h * d for x, d in zip(xs, dirs)], dec.replay()))
        dn = float(fn([x - h * d for x, d in zip(xs, dirs)], dec.replay()))
    return ad, (up - dn) / (2 * h)


@pytest.mark.parametrize("name", WHOLE_SIZES)
def test_reference_gradients_equal_central_differences_of_itself(name):
    """Truncation is about 1e-10 and rounding about 1e-11 of the derivative: agreement to 1e-6 has ample margin, and worse than
    that means the reference is wrong."""
    dt = torch.float64
    _, _, levels, numiters = fw.SIZES[name]
    K = fw.scene(name)["K"]
    rng = np.random.default_rng(3)
    for b in range(2):
        W = torch.tensor(loss_weights()[b])
        whole = lambda xs, dec: (W * ref.odometry(xs[0], xs[1], xs[2], xs[3], K, levels, numiters, dt, init=xs[4], dec=dec)).sum()
        ad, fd = directional(whole, ref.leaves(frames(name, b) + [np.eye(4)[:3]], dt), rng)
        print(name, "b", b, "whole call: autograd", ad, "central differences", fd)
        assert abs(ad) > 1e-6 and abs(ad - fd) <= 1e-6 * abs(ad), (name, b, ad, fd)
        for which in SEAM_TRANSFORMS:
            g = torch.tensor(sum_weights()[b, :28])
            one = lambda xs, dec: (g * ref.seam(xs[0], xs[1], xs[2], xs[3], K, xs[4], dt, dec=dec)[0][:28]).sum()
            ad, fd = directional(one, ref.leaves(list(seam_frames(name, which, b)) + [fw.transforms(name)[which][b][:3]], dt), rng)
            print(name, which, "b", b, "seam: autograd", ad, "central differences", fd)
            assert abs(ad) > 1e-6 and abs(ad - fd) <= 1e-6 * abs(ad), (name, which, b, ad, fd)


def test_recorded_deviations_are_what_the_float32_transcription_gives():
    """The constants the GPU bounds are built from: recomputed here from float32 autograd of the transcription, never from the
    device; recorded from this, not padded."""
    whole, gap, seam, gt96 = measure_constants()
    print("whole", whole, "gap", gap, "seam", seam, "g_T at 96x130", gt96)
    pairs = [(whole[n][k], WHOLE_DEVIATION[n][k], (n, k)) for n in WHOLE_SIZES for k in range(5)]
    pairs += [(gap[k], GAP_DEVIATION[k], ("gap", k)) for k in range(5)]
    pairs += [(seam[w][k], SEAM_DEVIATION[w][k], (w, k)) for w in SEAM_TRANSFORMS for k in range(5)]
    pairs += [(gt96[w], SEAM_GT_96[w], ("96x130", w)) for w in SEAM_TRANSFORMS]
    for got, recorded, what in pairs:
        assert 0.5 * recorded <= got <= recorded, (what, got, recorded)


# ------------------------------------------------------------------ GPU
def dev_leaves(arrays):
    return [torch.from_numpy(np.stack(a).astype(np.float32)).to(DEV).requires_grad_(True) for a in arrays]


def dev_K(name):
    return fw.dev_scene(name)["K"]


def seam_device(name, which):
    """-> (valid, the five gradients as numpy (B, ...)) of the device at the edited frames."""
    fr = [np.stack([seam_frames(name, which, b)[k] for b in range(2)]) for k in range(4)]
    td, tc, sd, sc = (torch.from_numpy(a).to(DEV) for a in fr)
    T = fw.dev_T(fw.transforms(name)[which])
    g_sums = torch.from_numpy(sum_weights().astype(np.float32)).to(DEV)
    valid, _, _ = ops.rgbd_rows_raw(td, tc, sd, sc, dev_K(name), T)
    grads = ops.rgbd_rows_bwd_raw(td, tc, sd, sc, dev_K(name), T, g_sums)
    assert tuple(grads[4].shape) == (2, 3, 4)
    return valid.cpu().numpy().astype(bool), [g.cpu().numpy() for g in grads]


@pytest.mark.gpu
@pytest.mark.parametrize("which", SEAM_TRANSFORMS)
@pytest.mark.parametrize("name", SEAM_SIZES)
def test_seam_gradients_match_float64_autograd(name, which):
    valid, grads = seam_device(name, which)
    bound = [4 * x for x in SEAM_DEVIATION[which]]
    for b in range(2):
        _, want, ref_valid, touched = seam_reference(name, which, "float64")[b]
        assert np.array_equal(valid[b], ref_valid), (name, which, b)
        got = {k: g[b] for k, g in zip(INPUTS, grads)}
        dev = deviation(got, want)
        print(name, which, "b", b, "deviation per input", dev, "bound", bound)
        for k in range(5):
            assert dev[k] <= bound[k], (name, which, b, INPUTS[k], dev[k], bound[k])
        # zero exactly where it must be
        assert not got["sd"][~ref_valid].any() and not got["sc"][~ref_valid].any()
        assert not got["td"][~touched].any() and not got["tc"][~touched].any()
        assert got["sd"][ref_valid].any() and got["tc"][touched].any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", SEAM_TRANSFORMS)
def test_seam_transform_gradient_with_more_than_one_partial_row_per_group(which):
    name = "96x130"
    valid, grads = seam_device(name, which)
    for b in range(2):
        _, want, ref_valid, _ = seam_reference(name, which, "float64")[b]
        assert np.array_equal(valid[b], ref_valid)
        dev = float(np.abs(grads[4][b] - want["T"]).max() / np.abs(want["T"]).max())
        print(name, which, "b", b, "g_T deviation", dev, "bound", 4 * SEAM_GT_96[which])
        assert dev <= 4 * SEAM_GT_96[which], (which, b, dev)


def whole_device(name, counts=None, zero_source=None, deterministic=False, no_target_grad=False):
    """-> (T, info, [g_td, g_tc, g_sd, g_sc, g_init]) of sum(W * T[:, :3]) on the device, init = the identity."""
    _, _, levels, numiters = fw.SIZES[name]
    fr = [[frames(name, b)[k] for b in range(2)] for k in range(4)]
    if zero_source is not None:
        fr[2][zero_source] = np.zeros_like(fr[2][zero_source])
    td, tc, sd, sc, init = dev_leaves(fr + [[np.eye(4)] * 2])
    if no_target_grad:
        td, tc = td.detach(), tc.detach()
    W = torch.from_numpy(loss_weights().astype(np.float32)).to(DEV)
    torch.use_deterministic_algorithms(deterministic)
    try:
        T, info = ops.rgbd_odometry(td, tc, sd, sc, dev_K(name), init=init, numiters=counts or numiters, levels=levels, differentiable=True)
        assert T.requires_grad and not info.requires_grad
        (W * T[:, :3]).sum().backward()
    finally:
        torch.use_deterministic_algorithms(False)
    return T.detach(), info, [t.grad for t in (td, tc, sd, sc, init)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", WHOLE_SIZES)
def test_whole_call_gradients_match_float64_autograd(name):
    T, info, grads = whole_device(name)
    T_plain, info_plain = fw.run_device(name, init=fw.dev_T(np.stack([np.eye(4)] * 2)))
    assert torch.equal(T, T_plain) and torch.equal(info, info_plain)  # the taped forward's bits are the plain call's
    assert tuple(grads[4].shape) == (2, 4, 4) and not grads[4][:, 3].any()
    bound = [4 * x for x in WHOLE_DEVIATION[name]]
    for b in range(2):
        want = whole_reference(name, "float64")[b][1]
        got = {k: g[b].cpu().numpy() for k, g in zip(INPUTS, grads)}
        got["T"] = got["T"][:3]
        dev = deviation(got, want)
        print(name, "b", b, "deviation per input", dev, "bound", bound)
        for k in range(5):
            assert dev[k] <= bound[k], (name, b, INPUTS[k], dev[k], bound[k])


@pytest.mark.gpu
def test_gradients_repeat_bit_for_bit_and_under_deterministic_algorithms():
    for name in WHOLE_SIZES:
        runs = [whole_device(name), whole_device(name), whole_device(name, deterministic=True)]
        for other in runs[1:]:
            assert torch.equal(runs[0][0], other[0])
            for a, b in zip(runs[0][2], other[2]):
                assert torch.equal(a, b), name
        assert all(g.abs().max() > 0 and torch.isfinite(g).all() for g in runs[0][2])


@pytest.mark.gpu
def test_no_iterations_hand_the_gradient_to_init():
    W = torch.from_numpy(loss_weights().astype(np.float32)).to(DEV)
    T, _, grads = whole_device("48x64", counts=(0, 0, 0))
    assert torch.equal(T[:, :3], torch.eye(4, device=DEV)[:3].expand(2, 3, 4))
    assert torch.equal(grads[4][:, :3], W) and not grads[4][:, 3].any()
    assert not any(g.any() for g in grads[:4])


@pytest.mark.gpu
def test_a_source_without_valid_depth_passes_its_gradient_through():
    W = torch.from_numpy(loss_weights().astype(np.float32)).to(DEV)
    _, _, full = whole_device("48x64")
    T, info, grads = whole_device("48x64", zero_source=1)
    assert (info[1][:, 2] == 1).all()  # status bit FEW at every level
    assert torch.equal(grads[4][1, :3], W[1]) and not grads[4][1, 3].any()
    assert not any(g[1].any() for g in grads[:4])
    for a, b in zip(grads, full):
        assert torch.equal(a[0], b[0])  # the other element: the unedited run's bits


@pytest.mark.gpu
def test_a_level_without_iterations_between_levels_that_have_some():
    T, info, grads = whole_device("48x64", counts=GAP_COUNTS)
    assert info[:, :, 3].cpu().tolist() == [list(map(float, GAP_COUNTS))] * 2
    T_plain, info_plain = fw.run_device("48x64", numiters=GAP_COUNTS, init=fw.dev_T(np.stack([np.eye(4)] * 2)))
    assert torch.equal(T, T_plain) and torch.equal(info, info_plain)
    again = whole_device("48x64", counts=GAP_COUNTS)[2]
    for g, g2 in zip(grads, again):
        assert torch.equal(g, g2) and torch.isfinite(g).all() and g.abs().max() > 0
    assert not grads[4][:, 3].any()
    bound = [4 * x for x in GAP_DEVIATION]
    for b in range(2):
        want = whole_reference("48x64", "float64", GAP_COUNTS)[b][1]
        got = {k: g[b].cpu().numpy() for k, g in zip(INPUTS, grads)}
        got["T"] = got["T"][:3]
        dev = deviation(got, want)
        print("b", b, "deviation per input", dev, "bound", bound)
        for k in range(5):
            assert dev[k] <= bound[k], (b, INPUTS[k], dev[k], bound[k])


@pytest.mark.gpu
def test_without_a_target_gradient_the_others_are_the_same_bits():
    """Only the source and init require gradients: the reverse pass skips the corner fold, and what it returns is unchanged."""
    _, _, full = whole_device("30x45")
    T, _, part = whole_device("30x45", no_target_grad=True)
    assert part[0] is None and part[1] is None
    for a, b in zip(part[2:], full[2:]):
        assert torch.equal(a, b)
    # the seam likewise: its C entry point with the two target outputs NULL
    name, which = "30x45", "true"
    fr = [np.stack([seam_frames(name, which, b)[k] for b in range(2)]) for k in range(4)]
    td, tc, sd, sc = (torch.from_numpy(a).to(DEV) for a in fr)
    Tq, K = fw.dev_T(fw.transforms(name)[which]).reshape(2, 16).contiguous(), dev_K(name)
    g_sums = torch.from_numpy(sum_weights().astype(np.float32)).to(DEV)
    want = ops.rgbd_rows_bwd_raw(td, tc, sd, sc, K, Tq.view(2, 4, 4), g_sums)
    g_sd, g_sc, g_T = torch.empty_like(sd), torch.empty_like(sc), torch.empty(2, 3, 4, device=DEV)
    ws = nv.workspace(nv.ws_bytes("gs_rgbd_odometry_bwd_ws_size", 2, 30, 45, 1, 1), td.device, "rgbd_grads_test")
    nv.call("gs_rgbd_rows_bwd", nv.ptr(td), nv.ptr(tc), nv.ptr(sd), nv.ptr(sc), 2, 30, 45, nv.ptr(K), nv.ptr(Tq), fw.LAM, fw.DDM, fw.SCALE,
            nv.ptr(g_sums), None, None, nv.ptr(g_sd), nv.ptr(g_sc), nv.ptr(g_T), nv.ptr(ws), ws.numel(), nv.stream())
    assert torch.equal(g_sd, want[2]) and torch.equal(g_sc, want[3]) and torch.equal(g_T, want[4])


@pytest.mark.gpu
@pytest.mark.parametrize("channels_first", [False, True])
def test_differentiable_provider_carries_the_graph(channels_first):
    target, source = fw.plane_frames()
    if channels_first:
        target, source = target.to_channels_first(), source.to_channels_first()
    with torch.no_grad():
        T_plain = RGBDOdometryProvider().provide(target, source)
    leaves = []
    for fr in (target, source):
        fr.rgb_image = fr.rgb_image.clone().requires_grad_(True)
        fr.depth_image = fr.depth_image.clone().requires_grad_(True)
        leaves += [fr.rgb_image, fr.depth_image]
    prov = RGBDOdometryProvider(differentiable=True)
    T = prov.provide(target, source)
    assert T.shape == (1, 1, 4, 4) and T.requires_grad and not prov.last_info.requires_grad
    assert torch.equal(T.detach(), T_plain)
    T[0, 0, :3, 3].sum().backward()
    for t in leaves:
        assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0


@pytest.mark.gpu
def test_kinectfusion_rgbd_with_pose_gradients():
    from tests import test_kinectfusion as tk

    fr = tk.frames(1)
    keep = fr[:, :3]
    with torch.no_grad():
        poses_plain = tk.kf(1, odom="rgbd", numiters=(4, 2, 2))(keep)[1]

    def run():
        depth, rgb = keep.depth_image.clone().requires_grad_(True), keep.rgb_image.clone().requires_grad_(True)
        seq = gs.RGBDImages(rgb, depth, keep.intrinsics, keep.poses)
        poses = tk.kf(1, odom="rgbd", numiters=(4, 2, 2), pose_gradients=True, odom_gradients=True)(seq)[1]
        poses[:, -1, :3, 3].sum().backward()
        return poses.detach(), depth.grad, rgb.grad

    poses, g_depth, g_rgb = run()
    assert torch.equal(poses, poses_plain)
    for g in (g_depth, g_rgb):
        assert torch.isfinite(g).all()
        assert g[:, 0].abs().max() > 0 and g[:, 1].abs().max() > 0
    _, g_depth2, g_rgb2 = run()
    assert torch.equal(g_depth, g_depth2) and torch.equal(g_rgb, g_rgb2)
