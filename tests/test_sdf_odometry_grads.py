"""The reverse pass of the SDF odometry (csrc/sdf.hip, csrc/gs_sdf_bwd.hpp: gs_sdf_odometry_taped, gs_sdf_odometry_bwd,
gs_sdf_rows_bwd; ops.sdf_odometry(differentiable=True), ops.sdf_rows_bwd_raw; SDFOdometryProvider(differentiable=True);
KinectFusion(odom="gradsdf")).

The reference is tests/sdf_grad_reference.py: a torch transcription of the rule of include/gradslam_hip.h, the decisions held
constant, differentiated by torch autograd.  float64 autograd is the reference.  float32 autograd of the same code measures what
fp32 alone costs (in autograd's order of operations, not the device's): WHOLE_DEVIATION, GAP_DEVIATION and SEAM_DEVIATION below
hold, per differentiable input, max |g32 - g64| over the input divided by the largest |g64| entry of that input, the larger of
the two batch elements -- measured on the CPU, recomputed and asserted by
test_recorded_deviations_are_what_the_float32_transcription_gives, never taken from the device -- and the device must agree with
float64 within FOUR times those, normalised the same way.  Scenes, volumes, deltas and the numpy references of the forward pass
are tests/test_sdf_odometry.py's; none is added.

At the seam fp32 and float64 must take the same decisions: the depth is first zeroed at the pixels where that file's ref_rows
`tie` mask holds as float64 sees it (at most 5 %), and the device's valid flags on the edited input must equal the reference's.
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
from gradslam_amd.odometry import SDFOdometryProvider
from tests import sdf_grad_reference as ref
from tests import test_sdf_odometry as fw

DEV = "cuda:0"
NEW_SYMBOLS = {"gs_sdf_odometry_tape_bytes_for": 6, "gs_sdf_odometry_bwd_room": 10, "gs_sdf_odometry_taped": 25,
               "gs_sdf_odometry_bwd": 29, "gs_sdf_rows_bwd": 25}
WHOLE_SIZES = ("5x7", "30x45s2", "48x64")
SEAM_SIZES = ("5x7", "30x45s2", "48x64", "96x130")  # 96x130: 49 blocks, more than one partial row per fold group
SEAM_DELTAS = ("true", "turned")
WHOLE_INPUTS = ("depth", "poses", "init", "tsdf")  # rows 0..2 of poses and init
SEAM_INPUTS = ("depth", "poses", "D", "tsdf")
# 48x64: a level with zero iterations between two that have some -- the reverse driver skips it and carries the 12-sum rows and
# the tape position across it.  The schedule has to converge (tests/test_rgbd_odometry_grads.py says why an unconverged loop
# cannot be compared); chosen on the CPU with measure_gap_candidates: this loop converges early -- (3, 0, 2), (6, 0, 6), (10, 0, 5)
# and (10, 0, 10) all leave float32 autograd of the transcription where (10, 5, 3) leaves it or nearer (depth 1.9e-4 .. 3.6e-4 of
# the largest entry, poses and init 2e-6, tsdf 3e-5) -- so the longest of them is taken.
GAP_COUNTS = (10, 0, 10)
NX, NY, NZ = fw.DIMS

# max |g32 - g64| / max |g64| per input, the larger of the two batch elements; see the module docstring
WHOLE_DEVIATION = {"5x7": (9.3e-7, 1.5e-6, 1.3e-6, 2.0e-5), "30x45s2": (1.7e-5, 7.9e-7, 8.0e-7, 3.4e-5), "48x64": (8.0e-4, 2.0e-6, 2.7e-6, 8.4e-5)}
GAP_DEVIATION = (3.6e-4, 1.6e-6, 2.1e-6, 3.0e-5)  # 48x64 with GAP_COUNTS
# per delta and size (SEAM_INPUTS' order)
SEAM_DEVIATION = {"true": {"5x7": (9.5e-7, 5.3e-7, 6.1e-7, 3.3e-6), "30x45s2": (5.7e-6, 2.0e-6, 1.9e-6, 4.0e-6),
                           "48x64": (6.4e-6, 7.5e-7, 8.4e-7, 2.9e-6), "96x130": (5.8e-6, 7.6e-7, 8.4e-7, 3.2e-6)},
                  "turned": {"5x7": (1.2e-6, 1.1e-6, 8.7e-7, 4.3e-6), "30x45s2": (3.9e-6, 8.6e-7, 8.8e-7, 6.7e-6),
                             "48x64": (4.7e-6, 4.6e-7, 4.9e-7, 2.0e-6), "96x130": (5.0e-6, 4.9e-7, 5.2e-7, 1.3e-6)}}

# What the two size queries return, pinned (a size that drifts changes allocations): [arguments, bytes]
RECORDED_SIZES = {
    "gs_sdf_odometry_tape_bytes_for": [[[1, 48, 64, 1, 1, 0], 2048], [[1, 48, 64, 1, 3, 18], 6400], [[2, 48, 64, 1, 3, 18], 12288],
                                       [[2, 30, 45, 2, 2, 12], 6912], [[1, 480, 640, 1, 3, 18], 144128], [[1, 480, 640, 4, 3, 60], 24320],
                                       [[1, 48, 64, 1, 3, -1], 0], [[0, 48, 64, 1, 3, 2], 0]],
    "gs_sdf_odometry_bwd_room": [[[1, 48, 64, 1, 3, 18, 24, 20, 16, 1], 158208], [[2, 48, 64, 1, 3, 18, 24, 20, 16, 1], 315136],
                                 [[2, 48, 64, 1, 3, 18, 24, 20, 16, 0], 7680], [[2, 30, 45, 2, 2, 12, 24, 20, 16, 1], 311552],
                                 [[1, 480, 640, 1, 3, 18, 256, 256, 256, 1], 335662592], [[1, 480, 640, 1, 3, 18, 256, 256, 256, 0], 118016],
                                 [[1, 48, 64, 1, 1, 1, 24, 20, 16, 1], 156160], [[1, 48, 64, 1, 3, 18, 0, 20, 16, 1], 0]],
}


def size_of(name):
    return {**fw.SIZES, **fw.MORE_SIZES}[name]


# ------------------------------------------------------------------ the reference's inputs and gradients
def loss_weights(B=2):
    return np.random.default_rng(7).standard_normal((B, 3, 4))


def sum_weights(B=2):
    return np.random.default_rng(11).standard_normal((B, 29))


def ref_volume(b, tsdf):
    v = fw.volume(b)
    return dict(tsdf=tsdf, weight=v["weight"], origin=v["origin"], v=fw.F32(fw.V), trunc=fw.F32(fw.TRUNC))


@lru_cache(maxsize=None)
def whole_reference(name, dt_name, counts=None):
    """Per batch element: (D (3,4), {input: gradient}) of sum(W * D) through the whole loop from init = the identity."""
    dt = getattr(torch, dt_name)
    _, _, stride, levels, numiters = size_of(name)
    s = fw.scene(name)
    out = []
    for b in range(2):
        depth, P, init, tsdf = ref.leaves([s["depth"][b], s["P"][b][:3], np.eye(4)[:3], fw.volume(b)["tsdf"]], dt)
        D = ref.odometry(depth, s["K"], P, ref_volume(b, tsdf), stride, levels, counts or numiters, dt, init=init)
        (torch.tensor(loss_weights()[b], dtype=dt) * D).sum().backward()
        out.append((D.detach().double().numpy(), {k: t.grad.double().numpy() for k, t in zip(WHOLE_INPUTS, (depth, P, init, tsdf))}))
    return out


@lru_cache(maxsize=None)
def seam_depth(name, which, b):
    """The depth with the pixels zeroed where float64 sees a tie (full resolution; the grid's pixels are [::stride, ::stride])."""
    stride = size_of(name)[2]
    s = fw.scene(name)
    tie = fw.ref_rows(s["depth"][b], s["K"], s["P"][b], fw.deltas(which)[b], fw.volume(b), np.float64, stride=stride)[2]["tie"]
    assert tie.mean() <= 0.05, (name, which, b, float(tie.mean()))
    depth = s["depth"][b].copy()
    depth[::stride, ::stride][tie] = 0.0
    return depth


@lru_cache(maxsize=None)
def seam_reference(name, which, dt_name):
    """Per batch element: (sums (29), {input: gradient}, valid mask on the grid, mask of the voxels a valid pixel's cell touches)."""
    dt = getattr(torch, dt_name)
    H, W, stride = size_of(name)[:3]
    s = fw.scene(name)
    out = []
    for b in range(2):
        depth, P, D, tsdf = ref.leaves([seam_depth(name, which, b), s["P"][b][:3], fw.deltas(which)[b][:3], fw.volume(b)["tsdf"]], dt)
        sums, (hs, ws, ix, iy, iz) = ref.seam(depth, s["K"], P, D, ref_volume(b, tsdf), dt, stride=stride)
        (torch.tensor(sum_weights()[b, :28], dtype=dt) * sums[:28]).sum().backward()
        valid, touched = np.zeros((-(-H // stride), -(-W // stride)), dtype=bool), np.zeros((NZ, NY, NX), dtype=bool)
        valid[hs.numpy() // stride, ws.numpy() // stride] = True
        for c in range(8):
            touched[iz.numpy() + (c >> 2), iy.numpy() + ((c >> 1) & 1), ix.numpy() + (c & 1)] = True
        out.append((sums.detach().double().numpy(), {k: t.grad.double().numpy() for k, t in zip(SEAM_INPUTS, (depth, P, D, tsdf))}, valid, touched))
    return out


def deviation(got, want, inputs):
    """max |got - want| / max |want| per input."""
    return [float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in inputs]


def measure_constants():
    """What the recorded constants were measured with (python -c "import tests.test_sdf_odometry_grads as t; print(t.measure_constants())")."""
    worst = lambda rows: tuple(max(r[k] for r in rows) for k in range(len(rows[0])))
    w = lambda n, c=None: worst([deviation(whole_reference(n, "float32", c)[b][1], whole_reference(n, "float64", c)[b][1], WHOLE_INPUTS)
                                 for b in range(2)])
    whole = {n: w(n) for n in WHOLE_SIZES}
    gap = w("48x64", GAP_COUNTS)
    seam = {d: {n: worst([deviation(seam_reference(n, d, "float32")[b][1], seam_reference(n, d, "float64")[b][1], SEAM_INPUTS) for b in range(2)])
                for n in SEAM_SIZES} for d in SEAM_DELTAS}
    return whole, gap, seam


def measure_gap_candidates(candidates=((3, 0, 2), (6, 0, 6), (10, 0, 5), (10, 0, 10))):
    """How GAP_COUNTS was chosen, on the CPU: per candidate (n, 0, m) the float32 transcription's deviation from float64 per
    input -- a loop that has not converged amplifies every flipped decision."""
    out = {}
    for c in candidates:
        dev = [deviation(whole_reference("48x64", "float32", c)[b][1], whole_reference("48x64", "float64", c)[b][1], WHOLE_INPUTS) for b in range(2)]
        out[c] = [max(d[k] for d in dev) for k in range(4)]
    return out


# ------------------------------------------------------------------ CPU: ABI, contracts, the reference itself
def test_new_symbols_load_and_are_declared():
    lib = nv.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^)]*)\);", header, flags=re.M)  # (the comments name the functions too)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
        assert not {"ws", "ws_bytes", "tape_bytes", "tape_size"} & set(re.findall(r"\w+", decl.group(1))), name  # named buffers with capacities
    for name, nargs in fw.NEW_SYMBOLS.items():  # the existing entry points keep their argument counts
        assert len(nv.SIGNATURES[name][1]) == nargs, name
    assert lib.gs_abi_version() == 3
    assert hasattr(ops, "sdf_rows_bwd_raw")


def tape_formula(B, H, W, stride, total):
    align = lambda n: -(-n // 256) * 256
    R = -(-(-(-H // stride) * -(-W // stride)) // 256)
    return align(64 * B) + align(116 * R * B) + align(256 * max(total, 1) * B)


def room_formula(B, H, W, stride, total, nvox, want_tsdf):
    align = lambda n: -(-n // 256) * 256
    R = -(-(-(-H // stride) * -(-W // stride)) // 256)
    fold = 256 + align(4 * B * nvox) + align(16 * B * nvox) if want_tsdf else 0
    return 2 * align(64 * B) + align(128 * max(total, 1) * B) + 2 * align(48 * R * B) + fold


def test_size_queries_equal_the_header_formulas_and_what_was_recorded():
    lib = nv.lib()
    for (B, H, W, stride, levels, total) in ((2, 48, 64, 1, 3, 18), (2, 30, 45, 2, 2, 12), (1, 480, 640, 1, 3, 18), (2, 5, 7, 1, 1, 6),
                                             (2, 48, 64, 1, 3, 0), (1, 96, 130, 1, 1, 1), (3, 120, 160, 4, 2, 7)):
        assert lib.gs_sdf_odometry_tape_bytes_for(B, H, W, stride, levels, total) == tape_formula(B, H, W, stride, total)
        for dims in ((24, 20, 16), (256, 256, 256), (1, 1, 1)):
            nvox = dims[0] * dims[1] * dims[2]
            for want in (0, 1):
                got = lib.gs_sdf_odometry_bwd_room(B, H, W, stride, levels, total, *dims, want)
                assert got == room_formula(B, H, W, stride, total, nvox, want), (B, H, W, stride, levels, total, dims, want)
    assert lib.gs_sdf_odometry_tape_bytes_for(2, 48, 64, 1, 3, 0) == lib.gs_sdf_odometry_tape_bytes_for(2, 48, 64, 1, 3, 1)
    # 20 bytes per voxel, and only with the volume's gradient
    with_, without = (lib.gs_sdf_odometry_bwd_room(1, 48, 64, 1, 3, 18, 256, 256, 256, k) for k in (1, 0))
    assert with_ - without == 256 + 20 * 256 ** 3 and without < 1 << 16
    for bad in ((0, 48, 64, 1, 3, 1), (65536, 8, 8, 1, 1, 1), (1, 48, 64, 0, 3, 1), (1, 48, 64, 1, 0, 1), (1, 48, 64, 1, 9, 1), (1, 48, 64, 1, 5, 1),
                (1, 3, 64, 1, 1, 1), (1, 8192, 4096, 1, 1, 1), (1, 48, 64, 1, 3, -1), (1, 48, 64, 1, 1, (1 << 20) + 1)):
        assert lib.gs_sdf_odometry_tape_bytes_for(*bad) == 0, bad
        assert lib.gs_sdf_odometry_bwd_room(*bad, 24, 20, 16, 1) == 0, bad
    for dims in ((0, 20, 16), (24, -1, 16), (1024, 1024, 1024)):
        assert lib.gs_sdf_odometry_bwd_room(2, 48, 64, 1, 3, 18, *dims, 1) == 0, dims
    for name, rows in RECORDED_SIZES.items():
        assert len(rows) >= 5 and [[args, int(getattr(lib, name)(*args))] for args, _ in rows] == rows, name


def test_new_entry_points_refuse_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    lib = nv.lib()
    P = 4096
    inf, nan = float("inf"), float("nan")
    counts = (ctypes.c_int * 3)(2, 1, 1)
    #     d  B  H   W   K  P  init tsdf w  nx  ny  nz  o  v     trunc minw stride L counts damp  T  info tape cap     stream
    ok = [P, 1, 48, 64, P, P, P, P, P, 24, 20, 16, P, 0.05, 0.15, 1.0, 1, 3, counts, 1e-8, P, P, P, 1 << 24, None]
    assert len(ok) == NEW_SYMBOLS["gs_sdf_odometry_taped"]
    for pos in (0, 4, 5, 7, 8, 12, 18, 20, 21):  # (init may be NULL: the identity)
        args = list(ok)
        args[pos] = None
        assert lib.gs_sdf_odometry_taped(*args) == -1, pos
    for pos, bad in ((1, 0), (1, 65536), (2, 0), (3, -1), (16, 0), (16, 5), (17, 0), (17, 9), (17, 5), (9, 0), (10, -3), (13, 0.0), (13, nan),
                     (14, inf), (14, -0.1), (15, nan), (19, -1e-8), (19, nan), (19, inf), (18, (ctypes.c_int * 3)(2, -1, 1)),
                     (18, (ctypes.c_int * 3)(2, 1, (1 << 20) + 1))):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_sdf_odometry_taped(*args) == -1, (pos, bad)
    assert b"gs_sdf_odometry_taped" in lib.gs_last_error()
    args = list(ok)
    args[23] = lib.gs_sdf_odometry_tape_bytes_for(1, 48, 64, 1, 3, 4) - 1
    assert lib.gs_sdf_odometry_taped(*args) == -2 and b"tape too small" in lib.gs_last_error()
    args = list(ok)
    args[22], args[23] = None, 0
    assert lib.gs_sdf_odometry_taped(*args) == -2

    #     d  B  H   W   K  P  tsdf w  nx  ny  nz  o  v     trunc minw stride L counts damp  tape cap    gT g_d g_P g_i g_t room cap      stream
    ok = [P, 1, 48, 64, P, P, P, P, 24, 20, 16, P, 0.05, 0.15, 1.0, 1, 3, counts, 1e-8, P, 1 << 24, P, P, P, P, P, P, 1 << 26, None]
    assert len(ok) == NEW_SYMBOLS["gs_sdf_odometry_bwd"]
    for pos in (0, 4, 5, 6, 7, 11, 17, 21):  # (any of the four outputs may be NULL)
        args = list(ok)
        args[pos] = None
        assert lib.gs_sdf_odometry_bwd(*args) == -1, pos
    for pos, bad in ((1, 0), (1, 65536), (2, 0), (3, 3), (15, 0), (16, 0), (16, 5), (16, 9), (8, 0), (12, 0.0), (12, nan), (13, inf), (14, nan),
                     (18, -1.0), (18, inf), (17, (ctypes.c_int * 3)(2, 1, -5))):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_sdf_odometry_bwd(*args) == -1, (pos, bad)
    assert b"gs_sdf_odometry_bwd" in lib.gs_last_error()
    args = list(ok)
    args[20] = lib.gs_sdf_odometry_tape_bytes_for(1, 48, 64, 1, 3, 4) - 1
    assert lib.gs_sdf_odometry_bwd(*args) == -2 and b"tape too small" in lib.gs_last_error()
    args = list(ok)
    args[19], args[20] = None, 0
    assert lib.gs_sdf_odometry_bwd(*args) == -2
    args = list(ok)
    args[27] = lib.gs_sdf_odometry_bwd_room(1, 48, 64, 1, 3, 4, 24, 20, 16, 1) - 1
    assert lib.gs_sdf_odometry_bwd(*args) == -2 and b"room too small" in lib.gs_last_error()
    args[25], args[27] = None, lib.gs_sdf_odometry_bwd_room(1, 48, 64, 1, 3, 4, 24, 20, 16, 0) - 1  # without g_tsdf: the smaller room
    assert lib.gs_sdf_odometry_bwd(*args) == -2 and b"room too small" in lib.gs_last_error()
    args = list(ok)
    args[26], args[27] = None, 0
    assert lib.gs_sdf_odometry_bwd(*args) == -2

    #     d  B  H   W   K  P  D  tsdf w  nx  ny  nz  o  v     trunc minw stride g_sums g_d g_P g_D g_t room cap      stream
    ok = [P, 1, 48, 64, P, P, P, P, P, 24, 20, 16, P, 0.05, 0.15, 1.0, 1, P, P, P, P, P, P, 1 << 26, None]
    assert len(ok) == NEW_SYMBOLS["gs_sdf_rows_bwd"]
    for pos in (0, 4, 5, 6, 7, 8, 12, 17):
        args = list(ok)
        args[pos] = None
        assert lib.gs_sdf_rows_bwd(*args) == -1, pos
    for pos, bad in ((1, 0), (2, 3), (3, -4), (16, 0), (16, 17), (9, -1), (13, 0.0), (13, nan), (14, inf), (14, -1.0), (15, nan)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_sdf_rows_bwd(*args) == -1, (pos, bad)
    assert b"gs_sdf_rows_bwd" in lib.gs_last_error()
    args = list(ok)
    args[23] = lib.gs_sdf_odometry_bwd_room(1, 48, 64, 1, 1, 1, 24, 20, 16, 1) - 1
    assert lib.gs_sdf_rows_bwd(*args) == -2 and b"room too small" in lib.gs_last_error()


def test_ops_provider_and_kinectfusion_contracts():
    from gradslam_amd.slam import KinectFusion

    fr, vol = fw.cpu_frames(), fw.cpu_volume()
    d, K, P = fr.depth_image[:, 0], fr.intrinsics, fr.poses[:, 0]
    state = (vol.tsdf, vol.weight, vol.origin, vol.voxel_size, vol.trunc)
    one = dict(levels=1, numiters=1)
    g = lambda t: t.clone().requires_grad_(True)
    cases = (((g(d), K, P, *state), {}), ((d, K, g(P), *state), {}), ((d, K, P, g(vol.tsdf), *state[1:]), {}), ((d, K, P, *state), dict(init=g(P))))
    for args, kw in cases:
        with pytest.raises(NotImplementedError, match="gradients"):  # the default still refuses
            ops.sdf_odometry(*args, **one, **kw)
        with pytest.raises(NotImplementedError, match="gradients"):
            ops.sdf_odometry(*args, **one, **kw, differentiable=False)
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # the flag lets them through to the device check
            ops.sdf_odometry(*args, **one, **kw, differentiable=True)
    Kg = g(K)
    with pytest.raises(NotImplementedError, match="intrinsics"):  # not differentiable: refused, not cut silently
        ops.sdf_odometry(d, Kg, P, *state, **one, differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (the plain call detaches them, as it did)
        ops.sdf_odometry(d, Kg, P, *state, **one)
    eye = torch.eye(4).view(1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sdf_rows_bwd_raw(d, K, P, eye, torch.zeros(1, 29), *state)
    with pytest.raises(ValueError, match="g_sums"):
        ops.sdf_rows_bwd_raw(d, K, P, eye, torch.zeros(1, 28), *state)
    with pytest.raises(TypeError, match="D to be a tensor"):
        ops.sdf_rows_bwd_raw(d, K, P, None, torch.zeros(1, 29), *state)

    with pytest.raises(TypeError, match="differentiable"):
        SDFOdometryProvider(differentiable=1)
    assert SDFOdometryProvider().differentiable is False
    grad_d = gs.RGBDImages(fr.rgb_image, g(fr.depth_image), fr.intrinsics, fr.poses)
    grad_v = fw.cpu_volume()
    grad_v.tsdf = grad_v.tsdf.requires_grad_(True)
    diff = SDFOdometryProvider(2, levels=1, differentiable=True)
    for v_, f_ in ((vol, grad_d), (grad_v, fr)):
        with pytest.raises(NotImplementedError, match="gradients"):
            SDFOdometryProvider(2, levels=1).provide(v_, f_)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            diff.provide(v_, f_)
    with pytest.raises(NotImplementedError, match="intrinsics"):
        diff.provide(vol, gs.RGBDImages(fr.rgb_image, fr.depth_image, g(fr.intrinsics), fr.poses))

    kw = dict(dims=(8, 8, 8), voxel_size=0.1, device="cuda:0")
    slam = KinectFusion(odom="gradsdf", numiters=(4, 2), levels=2, damp=1e-6, dsratio=2, min_weight=2.0, color=False, **kw)
    prov = slam.odomprov
    assert isinstance(prov, SDFOdometryProvider) and prov.differentiable is True
    assert (prov.numiters, prov.levels, prov.damp, prov.stride, prov.min_weight) == ((4, 2), 2, 1e-6, 2, 2.0)
    assert KinectFusion(odom="sdf", **kw).odomprov.differentiable is False
    with pytest.raises(ValueError, match="not supported.*'gradsdf', 'sdf'$"):
        KinectFusion(odom="orb", **kw)
    messages = []
    for odom in ("sdf", "gradsdf"):
        with pytest.raises(ValueError, match="odom_gradients") as e:
            KinectFusion(odom=odom, odom_gradients=True, **kw)
        messages.append(str(e.value))
    assert messages[0] == messages[1]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KinectFusion(odom="gradsdf", levels=1, dsratio=1, **kw).step(vol, grad_d, fw.cpu_frames())


@pytest.mark.parametrize("name", WHOLE_SIZES)
def test_float64_transcription_forward_equals_the_numpy_reference(name):
    for b in range(2):
        D = whole_reference(name, "float64")[b][0]
        assert np.abs(D - fw.odometry_reference(name, b)[0][:3]).max() <= 1e-12
    if name == "48x64":
        s = fw.scene(name)
        for b in range(2):
            want = fw.ref_odometry(s["depth"][b], s["K"], s["P"][b], fw.volume(b), 1, 3, GAP_COUNTS, np.float64)[0]
            assert np.abs(whole_reference(name, "float64", GAP_COUNTS)[b][0] - want[:3]).max() <= 1e-12


@pytest.mark.parametrize("which", SEAM_DELTAS)
@pytest.mark.parametrize("name", SEAM_SIZES)
def test_float64_transcription_sums_equal_the_numpy_reference(name, which):
    s, stride = fw.scene(name), size_of(name)[2]
    for b in range(2):
        sums, grads, valid, touched = seam_reference(name, which, "float64")[b]
        assert np.array_equal(grads["tsdf"] != 0, touched)  # the volume's gradient: exactly the voxels a valid pixel's cell touches
        ok, rows, aux = fw.ref_rows(seam_depth(name, which, b), s["K"], s["P"][b], fw.deltas(which)[b], fw.volume(b), np.float64, stride=stride)
        want = fw.sums29(rows, ok, np.float64)
        assert np.array_equal(ok, valid) and not aux["tie"].any() and ok.sum() >= 6
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


def entries(fn, xs, picks, h=1e-6):
    """Per input, a few entries: (autograd's, central differences') partial derivative, the decisions replayed."""
    dec = ref.Decisions()
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    fn(xs, dec).backward()
    out = []
    for k, idx in picks:
        e = torch.zeros_like(xs[k])
        e[idx] = h * max(1.0, float(xs[k].detach().abs().max()))
        with torch.no_grad():
            up = float(fn([x + e if j == k else x for j, x in enumerate(xs)], dec.replay()))
            dn = float(fn([x - e if j == k else x for j, x in enumerate(xs)], dec.replay()))
        out.append((k, idx, float(xs[k].grad[idx]), (up - dn) / (2 * float(e[idx]))))
    return out


@pytest.mark.parametrize("name", ("30x45s2", "48x64"))
def test_reference_gradients_equal_central_differences_of_itself(name):
    """Truncation is about 1e-10 and rounding about 1e-10 of the derivative: agreement to 1e-6 has ample margin, and worse than
    that means the reference is wrong.  One random direction over all inputs, and a few single entries per input -- the largest
    of its gradient and two more -- to 1e-5 of the input's largest gradient entry."""
    dt = torch.float64
    _, _, stride, levels, numiters = size_of(name)
    s = fw.scene(name)
    rng = np.random.default_rng(3)
    for b in range(2):
        Wt = torch.tensor(loss_weights()[b])
        vol = lambda t: ref_volume(b, t)
        whole = lambda xs, dec: (Wt * ref.odometry(xs[0], s["K"], xs[1], vol(xs[3]), stride, levels, numiters, dt, init=xs[2], dec=dec)).sum()
        xs = ref.leaves([s["depth"][b], s["P"][b][:3], np.eye(4)[:3], fw.volume(b)["tsdf"]], dt)
        ad, fd = directional(whole, xs, rng)
        print(name, "b", b, "whole call: autograd", ad, "central differences", fd)
        assert abs(ad) > 1e-6 and abs(ad - fd) <= 1e-6 * abs(ad), (name, b, ad, fd)
        want = whole_reference(name, "float64")[b][1]
        picks = []
        for k, key in enumerate(WHOLE_INPUTS):
            order = np.argsort(-np.abs(want[key]).reshape(-1))
            picks += [(k, tuple(int(i) for i in np.unravel_index(order[j], want[key].shape))) for j in (0, 3, 11)]
        for k, idx, a, f in entries(whole, xs, picks):
            scale = float(np.abs(want[WHOLE_INPUTS[k]]).max())
            assert abs(a - want[WHOLE_INPUTS[k]][idx]) <= 1e-12 * scale
            assert abs(a - f) <= 1e-5 * scale, (name, b, WHOLE_INPUTS[k], idx, a, f)
        for which in SEAM_DELTAS:
            gsum = torch.tensor(sum_weights()[b, :28])
            one = lambda xs, dec: (gsum * ref.seam(xs[0], s["K"], xs[1], xs[2], vol(xs[3]), dt, stride=stride, dec=dec)[0][:28]).sum()
            xs1 = ref.leaves([seam_depth(name, which, b), s["P"][b][:3], fw.deltas(which)[b][:3], fw.volume(b)["tsdf"]], dt)
            ad, fd = directional(one, xs1, rng)
            print(name, which, "b", b, "seam: autograd", ad, "central differences", fd)
            assert abs(ad) > 1e-6 and abs(ad - fd) <= 1e-6 * abs(ad), (name, which, b, ad, fd)


def test_recorded_deviations_are_what_the_float32_transcription_gives():
    """The constants the GPU bounds are built from: recomputed here from float32 autograd of the transcription, never from the
    device; recorded from this, not padded."""
    whole, gap, seam = measure_constants()
    print("whole", whole, "gap", gap, "seam", seam)
    pairs = [(whole[n][k], WHOLE_DEVIATION[n][k], (n, k)) for n in WHOLE_SIZES for k in range(4)]
    pairs += [(gap[k], GAP_DEVIATION[k], ("gap", k)) for k in range(4)]
    pairs += [(seam[d][n][k], SEAM_DEVIATION[d][n][k], (d, n, k)) for d in SEAM_DELTAS for n in SEAM_SIZES for k in range(4)]
    for got, recorded, what in pairs:
        assert 0.5 * recorded <= got <= recorded, (what, got, recorded)


# ------------------------------------------------------------------ GPU
def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def seam_device(name, which, want_tsdf=True):
    """-> (valid, [g_depth, g_poses, g_D, g_tsdf] as numpy (B, ...)) of the device at the edited depth."""
    t, stride = fw.dev_scene(name), size_of(name)[2]
    depth = dev32(np.stack([seam_depth(name, which, b) for b in range(2)]))
    D, g_sums = fw.dev_T(fw.deltas(which)), dev32(sum_weights())
    valid, _, _ = ops.sdf_rows_raw(depth, t["K"], t["P"], D, t["tsdf"], t["weight"], t["origin"], fw.V, fw.TRUNC, stride=stride)
    grads = ops.sdf_rows_bwd_raw(depth, t["K"], t["P"], D, g_sums, t["tsdf"], t["weight"], t["origin"], fw.V, fw.TRUNC, stride=stride,
                                 want_tsdf=want_tsdf)
    assert tuple(grads[1].shape) == (2, 3, 4) and tuple(grads[2].shape) == (2, 3, 4)
    return valid.cpu().numpy().astype(bool), [None if g is None else g.cpu().numpy() for g in grads]


@pytest.mark.gpu
@pytest.mark.parametrize("which", SEAM_DELTAS)
@pytest.mark.parametrize("name", SEAM_SIZES)
def test_seam_gradients_match_float64_autograd(name, which):
    valid, grads = seam_device(name, which)
    _, again = seam_device(name, which)
    bound = [4 * x for x in SEAM_DEVIATION[which][name]]
    for b in range(2):
        _, want, ref_valid, touched = seam_reference(name, which, "float64")[b]
        assert np.array_equal(valid[b], ref_valid), (name, which, b)
        got = {k: g[b] for k, g in zip(SEAM_INPUTS, grads)}
        dev = deviation(got, want, SEAM_INPUTS)
        print(name, which, "b", b, "deviation per input", dev, "bound", bound)
        for k in range(4):
            assert dev[k] <= bound[k], (name, which, b, SEAM_INPUTS[k], dev[k], bound[k])
        # zero exactly where it must be: pixels that are not valid (and off the grid), voxels no valid pixel's cell touches
        stride = size_of(name)[2]
        on_grid = np.zeros_like(got["depth"], dtype=bool)
        on_grid[::stride, ::stride] = ref_valid
        assert not got["depth"][~on_grid].any() and got["depth"][on_grid].any()
        assert np.array_equal(got["tsdf"] != 0, touched), (name, which, b, int((got["tsdf"] != 0).sum()), int(touched.sum()))
        slab = fw.volume(b)["slab"]  # (two voxels thick: every cell with a corner in it fails the weight gate, so all of it stays zero)
        assert slab.sum() >= 2 * min(NX * NY, NY * NZ, NX * NZ) and not got["tsdf"][slab].any()
    for g, g2 in zip(grads, again):
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32))  # bit for bit from run to run


def whole_device(name, counts=None, deterministic=False, only_depth=False, zero_depth=None):
    """-> (T, info, [g_depth, g_poses, g_init, g_tsdf]) of sum(W * T[:, :3]) on the device, init = the identity; `zero_depth`:
    a batch element whose depth is all zero (no valid pixel: none of its steps is applied)."""
    _, _, stride, levels, numiters = size_of(name)
    t = fw.dev_scene(name)
    if zero_depth is not None:
        t["depth"][zero_depth] = 0.0  # (dev_scene's tensors are this call's own)
    depth, P, init, tsdf = (x.clone().requires_grad_(True) for x in (t["depth"], t["P"], torch.eye(4, device=DEV).repeat(2, 1, 1), t["tsdf"]))
    if only_depth:
        P, init, tsdf = P.detach(), init.detach(), tsdf.detach()
    Wt = dev32(loss_weights())
    torch.use_deterministic_algorithms(deterministic)
    try:
        T, info = ops.sdf_odometry(depth, t["K"], P, tsdf, t["weight"], t["origin"], fw.V, fw.TRUNC, init=init, numiters=counts or numiters,
                                   levels=levels, stride=stride, differentiable=True)
        assert T.requires_grad and not info.requires_grad
        (Wt * T[:, :3]).sum().backward()
    finally:
        torch.use_deterministic_algorithms(False)
    return T.detach(), info, [x.grad for x in (depth, P, init, tsdf)]


def compare_whole(name, grads, counts, bound):
    assert tuple(grads[1].shape) == (2, 4, 4) and tuple(grads[2].shape) == (2, 4, 4) and not grads[1][:, 3].any() and not grads[2][:, 3].any()
    for b in range(2):
        want = whole_reference(name, "float64", counts)[b][1]
        got = {k: g[b].cpu().numpy() for k, g in zip(WHOLE_INPUTS, grads)}
        got["poses"], got["init"] = got["poses"][:3], got["init"][:3]
        dev = deviation(got, want, WHOLE_INPUTS)
        print(name, counts, "b", b, "deviation per input", dev, "bound", bound)
        for k in range(4):
            assert dev[k] <= bound[k], (name, b, WHOLE_INPUTS[k], dev[k], bound[k])


@pytest.mark.gpu
@pytest.mark.parametrize("name", WHOLE_SIZES)
def test_whole_call_gradients_match_float64_autograd(name):
    T, info, grads = whole_device(name)
    T_plain, info_plain = fw.run_device(name, init=fw.dev_T(np.stack([np.eye(4)] * 2)))
    assert torch.equal(T, T_plain) and torch.equal(info, info_plain)  # the taped forward's bits are the plain call's
    compare_whole(name, grads, None, [4 * x for x in WHOLE_DEVIATION[name]])


@pytest.mark.gpu
def test_a_level_without_iterations_between_levels_that_have_some():
    T, info, grads = whole_device("48x64", counts=GAP_COUNTS)
    assert info[:, :, 3].cpu().tolist() == [list(map(float, GAP_COUNTS))] * 2
    T_plain, info_plain = fw.run_device("48x64", numiters=GAP_COUNTS, init=fw.dev_T(np.stack([np.eye(4)] * 2)))
    assert torch.equal(T, T_plain) and torch.equal(info, info_plain)
    compare_whole("48x64", grads, GAP_COUNTS, [4 * x for x in GAP_DEVIATION])


@pytest.mark.gpu
def test_gradients_repeat_bit_for_bit_and_under_deterministic_algorithms():
    for name in WHOLE_SIZES:
        runs = [whole_device(name), whole_device(name), whole_device(name, deterministic=True)]
        for other in runs[1:]:
            assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])
            for a, b in zip(runs[0][2], other[2]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert all(g.abs().max() > 0 and torch.isfinite(g).all() for g in runs[0][2])


@pytest.mark.gpu
def test_no_iterations_hand_the_gradient_to_init():
    Wt = dev32(loss_weights())
    T, _, grads = whole_device("48x64", counts=(0, 0, 0))
    assert torch.equal(T[:, :3], torch.eye(4, device=DEV)[:3].expand(2, 3, 4))
    assert torch.equal(grads[2][:, :3], Wt) and not grads[2][:, 3].any()
    assert not grads[0].any() and not grads[1].any() and not grads[3].any()


@pytest.mark.gpu
def test_with_only_the_depth_wanted_the_room_has_no_fold_and_the_depth_gradient_keeps_its_bits(monkeypatch):
    name = "30x45s2"
    H, W, stride, levels, numiters = size_of(name)
    asked = []
    real = ops.ws_bytes
    monkeypatch.setattr(ops, "ws_bytes", lambda q, *a: (asked.append((q, a)), real(q, *a))[1])
    _, _, full = whole_device(name)
    _, _, part = whole_device(name, only_depth=True)
    rooms = [a for q, a in asked if q == "gs_sdf_odometry_bwd_room"]
    assert [a[-1] for a in rooms] == [1, 0] and rooms[0][:-1] == rooms[1][:-1] == (2, H, W, stride, levels, sum(numiters), NX, NY, NZ)
    with_, without = (real("gs_sdf_odometry_bwd_room", *a) for a in rooms)
    assert with_ - without == 256 + -(-4 * 2 * NX * NY * NZ // 256) * 256 + 16 * 2 * NX * NY * NZ
    assert part[1] is None and part[2] is None and part[3] is None
    assert torch.equal(part[0].view(torch.int32), full[0].view(torch.int32))
    # the seam likewise: without g_tsdf the other three keep their bits
    _, a = seam_device(name, "true")
    _, b = seam_device(name, "true", want_tsdf=False)
    assert b[3] is None and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[:3], b[:3]))


GUARD = 4096


def guarded(nbytes, poison):
    buf = torch.full((nbytes + 2 * GUARD,), poison, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + GUARD


def intact(buf, nbytes, poison):
    return bool((buf[:GUARD] == poison).all()) and bool((buf[GUARD + nbytes:] == poison).all())


@pytest.mark.gpu
def test_the_three_entry_points_stay_inside_exactly_the_queried_tape_and_room():
    """Each of gs_sdf_odometry_taped, gs_sdf_odometry_bwd and gs_sdf_rows_bwd with a tape and a room of exactly the queried size,
    between 4096-byte guard bands of 0xA5 and of 0xFF: the guards stay intact, the outputs are a roomy run's bits, and one byte
    less is refused (code -2) with the outputs untouched.  This file holds the exact-size discipline for them: they take named
    buffers with capacities, not (ws, ws_bytes)."""
    name = "30x45s2"
    H, W, stride, levels, numiters = size_of(name)
    total = sum(numiters)
    t = fw.dev_scene(name)
    init, Wt, g_sums, D = torch.eye(4, device=DEV).repeat(2, 1, 1), dev32(np.concatenate([loss_weights(), np.zeros((2, 1, 4))], 1)), dev32(sum_weights()), fw.dev_T(fw.deltas("true"))
    counts = (ctypes.c_int * levels)(*numiters)
    vol = (nv.ptr(t["tsdf"]), nv.ptr(t["weight"]), NX, NY, NZ, nv.ptr(t["origin"]), fw.V, fw.TRUNC, 1.0, stride)
    frame = (nv.ptr(t["depth"]), 2, H, W, nv.ptr(t["K"]), nv.ptr(t["P"]))
    tape_n = nv.ws_bytes("gs_sdf_odometry_tape_bytes_for", 2, H, W, stride, levels, total)
    room_n = nv.ws_bytes("gs_sdf_odometry_bwd_room", 2, H, W, stride, levels, total, NX, NY, NZ, 1)
    seam_n = nv.ws_bytes("gs_sdf_odometry_bwd_room", 2, H, W, stride, 1, 1, NX, NY, NZ, 1)
    assert tape_n == tape_formula(2, H, W, stride, total) and room_n == room_formula(2, H, W, stride, total, NX * NY * NZ, 1)
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # (a fill no output holds)
    shapes = dict(fwd=[(2, 4, 4), (2, levels, 4)], bwd=[(2, H, W), (2, 16), (2, 16), (2, NZ, NY, NX)], seam=[(2, H, W), (2, 12), (2, 12), (2, NZ, NY, NX)])

    def forward(tape_ptr, cap, outs):
        nv.call("gs_sdf_odometry_taped", *frame, nv.ptr(init), *vol, levels, counts, 1e-8, *(nv.ptr(o) for o in outs), tape_ptr, cap, nv.stream())

    def backward(tape_ptr, tape_cap, room_ptr, cap, outs):
        nv.call("gs_sdf_odometry_bwd", *frame, *vol, levels, counts, 1e-8, tape_ptr, tape_cap, nv.ptr(Wt), *(nv.ptr(o) for o in outs), room_ptr, cap,
                nv.stream())

    def rows_bwd(room_ptr, cap, outs):
        nv.call("gs_sdf_rows_bwd", *frame, nv.ptr(D), *vol, nv.ptr(g_sums), *(nv.ptr(o) for o in outs), room_ptr, cap, nv.stream())

    same = lambda xs, ys: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(xs, ys))
    untouched = lambda xs: all(bool(torch.isnan(x).all()) for x in xs)
    # roomy runs
    big_tape, big_room = (torch.empty(4 * n + 4096, dtype=torch.uint8, device=DEV) for n in (tape_n, room_n))
    ref_f, ref_b, ref_s = ([new(*s) for s in shapes[k]] for k in ("fwd", "bwd", "seam"))
    forward(nv.ptr(big_tape), big_tape.numel(), ref_f)
    backward(nv.ptr(big_tape), big_tape.numel(), nv.ptr(big_room), big_room.numel(), ref_b)
    rows_bwd(nv.ptr(big_room), big_room.numel(), ref_s)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(x).any()) for x in ref_f + ref_b + ref_s)
    plain = fw.run_device(name, init=init)
    assert same(ref_f, plain)
    for poison in (0xA5, 0xFF):
        tbuf, tptr = guarded(tape_n, poison)
        rbuf, rptr = guarded(room_n, poison)
        sbuf, sptr = guarded(seam_n, poison)
        got_f, got_b, got_s = ([new(*s) for s in shapes[k]] for k in ("fwd", "bwd", "seam"))
        forward(tptr, tape_n, got_f)
        backward(tptr, tape_n, rptr, room_n, got_b)
        rows_bwd(sptr, seam_n, got_s)
        torch.cuda.synchronize()
        for what, buf, n in (("tape", tbuf, tape_n), ("room", rbuf, room_n), ("seam's room", sbuf, seam_n)):
            assert intact(buf, n, poison), "0x{:02X}: wrote outside the {}".format(poison, what)
        assert same(got_f, ref_f) and same(got_b, ref_b) and same(got_s, ref_s), hex(poison)
        # one byte less: refused before any device work, the outputs untouched
        for run, outs, msg in ((lambda o: forward(tptr, tape_n - 1, o), shapes["fwd"], "tape too small"),
                               (lambda o: backward(tptr, tape_n - 1, rptr, room_n, o), shapes["bwd"], "tape too small"),
                               (lambda o: backward(tptr, tape_n, rptr, room_n - 1, o), shapes["bwd"], "room too small"),
                               (lambda o: rows_bwd(sptr, seam_n - 1, o), shapes["seam"], "room too small")):
            outs = [new(*s) for s in outs]
            with pytest.raises(RuntimeError) as e:
                run(outs)
            assert msg in str(e.value) and "code -2" in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert untouched(outs), msg


@pytest.mark.gpu
@pytest.mark.parametrize("channels_first", [False, True])
def test_differentiable_provider_carries_the_graph(channels_first):
    name = "48x64"
    H, W, stride, levels, counts = size_of(name)
    t = fw.dev_scene(name)
    depth, poses = t["depth"].view(2, 1, H, W, 1).clone().requires_grad_(True), t["P"].view(2, 1, 4, 4).clone().requires_grad_(True)
    frames = gs.RGBDImages(torch.zeros(2, 1, H, W, 3, device=DEV), depth, t["K"].view(2, 1, 4, 4), poses)
    if channels_first:
        frames = frames.to_channels_first()
    vol = gs.TSDFVolume(fw.DIMS, fw.V, origin=t["origin"], trunc=fw.TRUNC, color=False, device=DEV)
    vol.tsdf, vol.weight = t["tsdf"].clone().requires_grad_(True), t["weight"]
    prov = SDFOdometryProvider(counts, levels, stride, differentiable=True)
    T = prov.provide(vol, frames)
    assert T.shape == (2, 1, 4, 4) and T.requires_grad and not prov.last_info.requires_grad
    assert torch.equal(T[:, 0].detach(), fw.run_device(name)[0])
    T[:, 0, :3, 3].sum().backward()
    for x in (depth, poses, vol.tsdf):
        assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0


@pytest.mark.gpu
def test_kinectfusion_gradsdf_tracks_as_sdf_and_carries_gradients_to_earlier_frames():
    from tests import test_kinectfusion as tk

    fr = tk.frames(2)
    keep = fr[:, :3]
    with torch.no_grad():
        poses_plain = tk.kf(2, **fw.KF)(keep)[1]
        poses_grad = tk.kf(2, **{**fw.KF, "odom": "gradsdf"})(keep)[1]
    assert torch.equal(poses_grad, poses_plain)  # bit for bit

    def run():
        depth = keep.depth_image.clone().requires_grad_(True)
        seq = gs.RGBDImages(keep.rgb_image, depth, keep.intrinsics, keep.poses)
        poses = tk.kf(2, **{**fw.KF, "odom": "gradsdf"}, pose_gradients=True)(seq)[1]
        poses[:, -1, :3, 3].sum().backward()
        return poses.detach(), depth.grad

    poses, g_depth = run()
    assert torch.equal(poses, poses_plain)
    assert torch.isfinite(g_depth).all()
    assert g_depth[:, 0].abs().max() > 0 and g_depth[:, 1].abs().max() > 0 and g_depth[:, 2].abs().max() > 0
    _, g_depth2 = run()
    assert torch.equal(g_depth.view(torch.int32), g_depth2.view(torch.int32))
