"""Pose gradients of the TSDF volume (gs_tsdf_integrate_backward_poses, gs_tsdf_raycast_backward_poses, the pose slots of
ops._TsdfIntegrateFn / _TsdfRaycastFn, TSDFVolume.raycast's attached poses, KinectFusion(pose_gradients=...)).

The scenes and the forward references are test_tsdf.py's and test_tsdf_raycast.py's, imported, not copied.  New here:
* ref_integrate_pose_backward / ref_cast_pose_backward: the header's pose formulas in numpy float64, checked against torch
  float64 autograd of the forward with the pose as the variable and every decision (pixels, skips, ending sample, cells) held
  constant.  absolute=True gives A, per entry the sum of the absolute terms.
* the float32 transcriptions integrate_pose_f32 / cast_pose_f32: the kernels' terms in the kernels' order and the reduction in
  its stated order (64-lane butterfly, 4 waves, rows r, r + 64, .., 64 partial sums).  Their deviation from float64 at the same
  decisions, in units of 2^-24 A, is recorded below (INTEGRATE_DEV, CAST_DEV) on the very shapes the GPU tests use, with the
  decisions taken on the CPU; the test recomputes it and the device gets four times that.  Like test_tsdf_raycast.py's
  gradients, the cast's formulas are evaluated at the float32 samples (fractions, values, cells of the float32 transcription of
  the forward, promoted).
* pose refinement against the volume: the same loop (gradient steps with backtracking on xi through se3_exp) with the float64
  reference on the CPU gave REFINE_REF; the device has to end within twice that.
"""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops
from gradslam_amd.geometry import se3utils
from gradslam_amd.synthetic import make_intrinsics, make_sequence
from tests import test_kinectfusion as tk
from tests import test_tsdf as tt
from tests import test_tsdf_raycast as tr
from tests.helpers import block_rows_f32, fold_rows_f32
from tests.test_tsdf import ref_centres, ref_integrate, small_cpu_scene, torch_integrate
from tests.test_tsdf_raycast import POSES, STEPS, host_volume, ref_cast, reference, torch_cast

DEV = "cuda:0"
U = 2.0 ** -24
F32 = np.float32
NEW_SYMBOLS = {"gs_tsdf_integrate_backward_poses_ws_bytes": 8, "gs_tsdf_integrate_backward_poses": 25,
               "gs_tsdf_raycast_backward_poses_ws_bytes": 9, "gs_tsdf_raycast_backward_poses": 26}

# the largest |float32 transcription - float64| / (2^-24 A) over the entries of g_poses ((rotation column, translation column) for
# the integration; (rotation block, translation column) for the cast), on the GPU tests' shapes with the CPU's decisions; asserted
# to lie in [0.5, 1] x these by test_float32_transcriptions_...; the device gets 4 x
INTEGRATE_DEV = (1.1, 0.8)
CAST_DEV = (2.7, 1.35)
# pose refinement with the float64 reference on the CPU (refine_reference): final translation [m] and rotation [rad] error
REFINE_REF = (1.71e-3, 1.14e-3)

# the integration's GPU scene: nx no multiple of 4, 819 voxels = 4 blocks of 256 with the last one partial; 12 x 16 images
I_DIMS, I_ORIGINS, I_H, I_W, I_B = (13, 9, 7), [(-0.3, -0.2, 1.85), (-0.25, -0.15, 1.9)], 12, 16, 2
# the cast's: test_tsdf_raycast.py's volumes and poses seen through a 20 x 28 camera (no multiple of 16: partial tiles, several
# blocks per camera) with an integer principal point, so that the identity pose has rays parallel to the axes
C_H, C_W = 20, 28
C_NAMES = [("rotated", "identity"), ("inside", "outside")]  # per batch element: L = 2


def make_K20():
    K = np.eye(4, dtype=F32); K[0, 0] = K[1, 1] = 26.25; K[0, 2] = 14.0; K[1, 2] = 10.0
    return K


# ------------------------------------------------------------------ the reduction, as the header states it (tests/helpers.py)
def voxel_blocks(terms):
    """(nvox, N) per-voxel terms -> (nblocks, 4, 64, N): thread = voxel, 256 consecutive voxels per block."""
    n, N = terms.shape
    pad = -n % 256
    return np.concatenate([terms, np.zeros((pad, N), F32)]).reshape(-1, 4, 64, N)


def pixel_blocks(terms, Ho, Wo):
    """(Ho * Wo, N) per-pixel terms -> (tiles, 4, 64, N): a block is 16 x 16 pixels, wave w its 8 x 8 tile (w >> 1, w & 1),
    lane its pixel (lane >> 3, lane & 7); blocks in row-major order."""
    N = terms.shape[-1]
    ty, tx = -(-Ho // 16), -(-Wo // 16)
    x = np.zeros((ty * 16, tx * 16, N), F32)
    x[:Ho, :Wo] = terms.reshape(Ho, Wo, N)
    x = x.reshape(ty, 2, 8, tx, 2, 8, N).transpose(0, 3, 1, 4, 2, 5, 6)
    return np.ascontiguousarray(x).reshape(ty * tx, 4, 64, N)


# ------------------------------------------------------------------ integration: reference and transcription
def ref_integrate_pose_backward(rec, cent, P, g_f, trunc, absolute=False):
    """One batch element in float64: rec from ref_integrate (L frames), cent (n, 3) the voxel centres, P (L, 4, 4) the poses,
    g_f (n,) the adjoint of the new tsdf -> g_poses (L, 4, 4).  Per frame S0 = sum gd, S_j = sum gd (c_j - t_j) over the voxels
    the frame updates, gd = g / (W + 1) / trunc inside the linear band; [j][2] = -S_j, [j][3] = R[j][2] S0.
    absolute=True: the sums of the absolute terms."""
    trunc = float(F32(trunc))
    ab = np.abs if absolute else (lambda x: x)
    L = len(rec)
    g = g_f.astype(np.float64).copy()
    c, P = cent.astype(np.float64), np.asarray(P).astype(np.float64)
    out = np.zeros((L, 4, 4))
    for l in reversed(range(L)):
        upd, lin, Wb = rec[l]["upd"], rec[l]["lin"], rec[l]["W"]
        den = Wb + 1.0
        gd = np.where(lin, g / den / trunc, 0.0)
        g = np.where(upd, g * (Wb / den), g)
        S0 = ab(gd).sum()
        Sj = ab(gd[:, None] * (c - P[l, :3, 3])).sum(0)
        out[l, :3, 2] = Sj if absolute else -Sj
        out[l, :3, 3] = ab(P[l, :3, 2]) * S0
    return out


def integrate_pose_f32(rec, cent, P, g_f, trunc):
    """The kernels' float32 chain: per frame, last to first, gd = (g / (W + 1)) / trunc, g = g (W / (W + 1)); the terms gd and
    gd (c_j - t_j); the reduction in its stated order; [j][2] = -S_j, [j][3] = R[j][2] S0."""
    trunc = F32(trunc)
    L = len(rec)
    g = g_f.astype(F32).copy()
    c, P = cent.astype(F32), np.asarray(P).astype(F32)
    out = np.zeros((L, 4, 4), F32)
    for l in reversed(range(L)):
        upd, lin, Wb = rec[l]["upd"], rec[l]["lin"], rec[l]["W"].astype(F32)
        den = Wb + F32(1.0)
        keep = Wb / den
        gd = np.where(lin, (g / den) / trunc, F32(0.0)).astype(F32)
        gd = np.where(upd, gd, F32(0.0))
        g = np.where(upd, g * keep, g)
        terms = np.stack([gd, gd * (c[:, 0] - P[l, 0, 3]), gd * (c[:, 1] - P[l, 1, 3]), gd * (c[:, 2] - P[l, 2, 3])], -1)
        assert terms.dtype == F32 and g.dtype == F32
        S = fold_rows_f32(block_rows_f32(voxel_blocks(terms), 4), 64)
        out[l, :3, 2] = -S[1:]
        out[l, :3, 3] = P[l, :3, 2] * S[0]
    return out


def tilt(poses, rx=0.02, rz=-0.015):
    """The sequence's cameras rotated a little about their own x and z axes, so that every R[j][2] is non-zero (make_poses
    rotates about y alone).  float32 in, float32 out."""
    Rl = np.eye(4)
    Rl[:3, :3] = tr.rot(rx, 0.0, rz)
    return (poses.astype(np.float64) @ Rl).astype(F32)


@lru_cache(maxsize=None)
def integrate_scene(L):
    """The integration's GPU scene on the host: (colors, depths, K, poses) of make_sequence with tilted poses, B = 2."""
    colors, depths, K, poses = make_sequence(I_B, L, I_H, I_W, seed=7, band=2)
    return colors, depths, K, torch.from_numpy(tilt(poses.numpy()))


def integrate_inputs(L, seed=5):
    """The prior state (weights in {0, 1, 2}) and the upstream adjoints of the integration tests, (B, n[, 3]) float32."""
    n = I_DIMS[0] * I_DIMS[1] * I_DIMS[2]
    rng = np.random.RandomState(seed + L)
    f0 = rng.uniform(-1, 1, (I_B, n)).astype(F32)
    w0 = rng.randint(0, 3, (I_B, n)).astype(F32)
    c0 = rng.uniform(0, 255, (I_B, n, 3)).astype(F32)
    g_f, g_c = rng.randn(I_B, n).astype(F32), rng.randn(I_B, n, 3).astype(F32)
    return f0, w0, c0, g_f, g_c


def integrate_deviation(recs, P, g_f):
    """max |float32 transcription - float64| / (2^-24 A) over the cameras: (rotation column, translation column); also the
    float64 reference and A, (B, L, 4, 4) each."""
    worst = np.zeros(2)
    want, A = [], []
    for b in range(I_B):
        cent = ref_centres(I_DIMS, tt.V, I_ORIGINS[b])
        w = ref_integrate_pose_backward(recs[b], cent, P[b], g_f[b], tt.TRUNC)
        a = ref_integrate_pose_backward(recs[b], cent, P[b], g_f[b], tt.TRUNC, absolute=True)
        t32 = integrate_pose_f32(recs[b], cent, P[b], g_f[b], tt.TRUNC)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(t32 - w) / (U * a)
        worst = np.maximum(worst, [np.nanmax(r[:, :3, 2]), np.nanmax(r[:, :3, 3])])
        want.append(w)
        A.append(a)
    return worst, np.stack(want), np.stack(A)


# ------------------------------------------------------------------ cast: reference and transcription
def cast_dirs(K, Ho, Wo, stride):
    """(dx, dy) (Ho * Wo,) float32 of the strided grid, as the ray rule forms them."""
    K = np.asarray(K, F32)
    w = np.arange(Wo, dtype=F32)[None, :] * F32(stride)
    h = np.arange(Ho, dtype=F32)[:, None] * F32(stride)
    dx = np.broadcast_to((w - K[0, 2]) / K[0, 0], (Ho, Wo)).reshape(-1)
    dy = np.broadcast_to((h - K[1, 2]) / K[1, 1], (Ho, Wo)).reshape(-1)
    assert dx.dtype == F32 and dy.dtype == F32
    return dx, dy


def cast_pose_terms(vol, rec, K, Ho, Wo, stride, g_depth, g_rgb, dt):
    """The twelve terms of every pixel (zero off the hits), (Ho * Wo, 12) in dtype dt, in the kernel's order of operations:
    3 i + j: ((z0 u0 + z1 u1) + z* w)_i d_j, 9 + i: ((u0 + u1) + w)_i."""
    dims, v = vol["dims"], dt(F32(vol["v"]))
    hit = rec["hit"]
    n = len(hit)
    D = lambda x: x[hit].astype(dt)
    f0, f1, dz, dw, a0, a1, ah = D(rec["f0"]), D(rec["f1"]), D(rec["dz"]), D(rec["dw"]), D(rec["a0"]), D(rec["a1"]), D(rec["ah"])
    k = rec["k"][hit]
    ids0, ids1, idsh = (tr.corner_ids(rec[key][hit], dims) for key in ("i0", "i1", "ih"))
    dx, dy = (x[hit].astype(dt) for x in cast_dirs(K, Ho, Wo, stride))
    F = vol["tsdf"].reshape(-1).astype(dt)
    gz = g_depth.reshape(-1)[hit].astype(dt)
    w = np.zeros((int(hit.sum()), 3), dt)
    if vol.get("color") is not None and g_rgb is not None:
        col = vol["color"].reshape(-1, 3).astype(dt)
        grgb = g_rgb.reshape(-1, 3)[hit].astype(dt)
        for ch in range(3):
            g = tr.trigrad(col[:, ch][idsh], ah)
            gz = gz + grgb[:, ch] * (((g[:, 0] * dw[:, 0] + g[:, 1] * dw[:, 1]) + g[:, 2] * dw[:, 2]) / v)
            w = w + grgb[:, ch][:, None] * (g / v)
    den = f0 - f1
    den2, gs_ = den * den, gz * dz
    c0, c1 = gs_ * ((-f1) / den2), gs_ * (f0 / den2)
    u0 = c0[:, None] * (tr.trigrad(F[ids0], a0) / v)
    u1 = c1[:, None] * (tr.trigrad(F[ids1], a1) / v)
    z0, z1 = ((k - 1).astype(F32) * rec["dz"][hit]).astype(dt), (k.astype(F32) * rec["dz"][hit]).astype(dt)  # z_k: fp32 by the rule
    if dt == F32:
        zs = ((k - 1).astype(F32) + f0 / den) * dz
    else:
        zs = ((k - 1).astype(dt) + f0 / den) * dz
    q = (z0[:, None] * u0 + z1[:, None] * u1) + zs[:, None] * w
    tr_ = (u0 + u1) + w
    t = np.concatenate([np.stack([q[:, i] * dx, q[:, i] * dy, q[:, i]], -1) for i in range(3)] + [tr_], -1)
    assert t.dtype == dt and t.shape[1] == 12
    out = np.zeros((n, 12), dt)
    out[hit] = t
    return out


def sums_to_pose(S):
    out = np.zeros((4, 4), S.dtype)
    out[:3, :3] = S[:9].reshape(3, 3)
    out[:3, 3] = S[9:]
    return out


def ref_cast_pose_backward(vol, rec, K, Ho, Wo, stride, g_depth, g_rgb, absolute=False):
    """The header's formulas in float64 at the records rec -> g_poses (4, 4); absolute=True: the sums of the absolute terms."""
    t = cast_pose_terms(vol, rec, K, Ho, Wo, stride, g_depth, g_rgb, np.float64)
    return sums_to_pose(np.abs(t).sum(0) if absolute else t.sum(0))


def cast_pose_f32(vol, rec, K, Ho, Wo, stride, g_depth, g_rgb):
    t = cast_pose_terms(vol, rec, K, Ho, Wo, stride, g_depth, g_rgb, F32)
    return sums_to_pose(fold_rows_f32(block_rows_f32(pixel_blocks(t, Ho, Wo), 4), 64))


@lru_cache(maxsize=None)
def cast20(b, pose, step, stride, dt=np.float64):
    """ref_cast of the common volume through the 20 x 28 camera; computed once, never written to."""
    return ref_cast(host_volume(b), make_K20(), POSES[pose], C_H, C_W, stride, step, dt=dt)


def cast_records(b, pose, step, stride):
    """As test_tsdf_raycast.gradient_records: the float32 transcription's records with the tying pixels taken out, the tape that
    goes with them and the share of the ties."""
    r64, r32 = cast20(b, pose, step, stride), cast20(b, pose, step, stride, dt=F32)
    good = ~r64["tie"]
    assert np.array_equal(r64["k_end"][good], r32["k_end"][good])
    rec = dict(r32["rec"], hit=r32["rec"]["hit"] & good.reshape(-1))
    return rec, np.where(good, r32["k_end"], 0).astype(np.int32), float((~good).mean())


def cast_upstream(stride, seed=9):
    Ho, Wo = -(-C_H // stride), -(-C_W // stride)
    rng = np.random.RandomState(seed + stride)
    return rng.randn(2, 2, Ho, Wo).astype(F32), rng.randn(2, 2, Ho, Wo, 3).astype(F32)


def cast_deviation(step, stride, color):
    """max |float32 transcription - float64| / (2^-24 A) over the four cameras: (rotation block, translation column); also the
    float64 reference and A, (B, L, 4, 4) each."""
    Ho, Wo = -(-C_H // stride), -(-C_W // stride)
    gd, gc = cast_upstream(stride)
    worst, want, A = np.zeros(2), np.zeros((2, 2, 4, 4)), np.zeros((2, 2, 4, 4))
    for b in range(2):
        hv = host_volume(b) if color else dict(host_volume(b), color=None)
        for l, name in enumerate(C_NAMES[b]):
            rec = cast_records(b, name, step, stride)[0]
            args = (hv, rec, make_K20(), Ho, Wo, stride, gd[b, l], gc[b, l] if color else None)
            want[b, l], A[b, l] = ref_cast_pose_backward(*args), ref_cast_pose_backward(*args, absolute=True)
            t32 = cast_pose_f32(*args)
            if rec["hit"].any():
                with np.errstate(invalid="ignore", divide="ignore"):
                    r = np.abs(t32 - want[b, l]) / (U * A[b, l])
                worst = np.maximum(worst, [np.nanmax(r[:3, :3]), np.nanmax(r[:3, 3])])
            else:
                assert not t32.any() and not want[b, l].any()
    return worst, want, A


# ------------------------------------------------------------------ CPU: ABI and error contracts
def test_pose_symbols_load_and_are_declared():
    lib = nv.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
        assert name + "(" in header, name
        decl = header[header.index(name + "("):]
        assert decl[: decl.index(";")].count(",") + 1 == nargs, name
    assert len(nv.SIGNATURES["gs_tsdf_integrate_backward"][1]) == 24 and len(nv.SIGNATURES["gs_tsdf_raycast_backward"][1]) == 25
    assert lib.gs_abi_version() == 3
    assert hasattr(ops, "tsdf_integrate_backward_poses_raw") and hasattr(ops, "tsdf_raycast_backward_poses_raw")


def test_pose_c_entry_points_refuse_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    lib = nv.lib()
    P = 4096
    nan, inf = float("nan"), float("inf")
    fold = lib.gs_tsdf_integrate_backward_ws_bytes(2, 3, 8, 8)
    # 819 voxels are 4 blocks: 16 B per (b, frame, block); more than one chunk adds the carried adjoints
    al = lambda n: -(-n // 256) * 256
    assert lib.gs_tsdf_integrate_backward_poses_ws_bytes(2, 3, 8, 8, 13, 9, 7, 1) == fold + al(16 * 2 * 3 * 4)
    one = lib.gs_tsdf_integrate_backward_ws_bytes(1, 40, 8, 8)
    assert lib.gs_tsdf_integrate_backward_poses_ws_bytes(1, 40, 8, 8, 13, 9, 7, 0) == one + al(16 * 32 * 4) + al(4 * 819)
    assert lib.gs_tsdf_integrate_backward_poses_ws_bytes(1, 40, 8, 8, 13, 9, 7, 1) == one + al(16 * 32 * 4) + al(4 * 819) + al(12 * 819)
    assert lib.gs_tsdf_integrate_backward_poses_ws_bytes(0, 3, 8, 8, 4, 4, 4, 1) == 0
    assert lib.gs_tsdf_integrate_backward_poses_ws_bytes(1, 3, 8, 8, 1024, 1024, 513, 1) == 0
    #     depth K poses B L  H  W  nx ny nz v  o  trunc maxw w  gt gc gti gci gd grgb gposes ws bytes   stream
    ok = [P, P, P, 1, 2, 8, 8, 4, 4, 4, 0.1, P, 0.3, 8.0, P, P, P, P, P, P, P, P, P, 1 << 20, None]
    for pos in (0, 1, 2, 11, 14, 15, 21):
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_integrate_backward_poses(*args) == -1, pos
    args = list(ok)
    args[16] = None  # g_color_in and g_rgb need g_color_out
    assert lib.gs_tsdf_integrate_backward_poses(*args) == -1
    for pos, bad in ((3, 0), (3, 65536), (4, 0), (5, 0), (6, -1), (7, 0), (8, -3), (9, 0), (7, 1 << 30), (10, 0.0), (10, nan), (12, 0.0),
                     (12, inf), (13, -1.0), (13, nan)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_integrate_backward_poses(*args) == -1, (pos, bad)
    assert b"gs_tsdf_integrate_backward_poses" in lib.gs_last_error()
    args = list(ok)
    args[22], args[23] = None, 0
    assert lib.gs_tsdf_integrate_backward_poses(*args) == -2
    args = list(ok)
    args[23] = lib.gs_tsdf_integrate_backward_poses_ws_bytes(1, 2, 8, 8, 4, 4, 4, 1) - 1
    assert lib.gs_tsdf_integrate_backward_poses(*args) == -2

    n = 2 * 42 * 22 * 56
    assert lib.gs_tsdf_raycast_backward_poses_ws_bytes(2, 42, 22, 56, 1, 2, 20, 28, 1) == \
        lib.gs_tsdf_raycast_backward_ws_bytes(2, 42, 22, 56, 1) + 48 * 2 * 2 * 4  # 20 x 28 pixels are 2 x 2 tiles
    assert lib.gs_tsdf_raycast_backward_poses_ws_bytes(2, 42, 22, 56, 0, 2, 20, 28, 3) == 256 + 4 * n + 16 * n + al(48 * 2 * 2 * 1)
    assert lib.gs_tsdf_raycast_backward_poses_ws_bytes(0, 4, 4, 4, 1, 2, 8, 8, 1) == 0
    assert lib.gs_tsdf_raycast_backward_poses_ws_bytes(1, 4, 4, 4, 1, 0, 8, 8, 1) == 0
    assert lib.gs_tsdf_raycast_backward_poses_ws_bytes(1, 4, 4, 4, 1, 2, 8, 8, 0) == 0
    #     tsdf w col B  nx ny nz v    o  K  P  L  H  W  s  step  minw kend gd grgb gt gc gposes ws bytes   stream
    ok = [P, P, P, 1, 4, 4, 4, 0.1, P, P, P, 2, 8, 8, 1, 0.05, 1.0, P, P, P, P, P, P, P, 1 << 20, None]
    for pos in (0, 1, 8, 9, 10, 17, 22):
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_raycast_backward_poses(*args) == -1, pos
    for drop in ((2,), (20,)):  # g_color and g_rgb need color; g_color needs g_tsdf
        args = list(ok)
        for pos in drop:
            args[pos] = None
        assert lib.gs_tsdf_raycast_backward_poses(*args) == -1, drop
    for pos, bad in ((3, 0), (4, 0), (7, -1.0), (11, 0), (11, 65536), (12, 0), (14, 0), (15, 0.0), (15, nan), (15, inf), (15, 1e-7), (16, nan)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_raycast_backward_poses(*args) == -1, (pos, bad)
    assert b"gs_tsdf_raycast_backward_poses" in lib.gs_last_error()
    args = list(ok)
    args[23], args[24] = None, 0
    assert lib.gs_tsdf_raycast_backward_poses(*args) == -2
    args = list(ok)
    args[24] = lib.gs_tsdf_raycast_backward_poses_ws_bytes(1, 4, 4, 4, 1, 2, 8, 8, 1) - 1
    assert lib.gs_tsdf_raycast_backward_poses(*args) == -2


def test_pose_python_error_contracts():
    t, w, c = torch.ones(1, 4, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4, 3)
    colors, depths, K, poses = make_sequence(1, 2, 8, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_integrate_backward_poses_raw(depths, K, poses, w, (0.0, 0.0, 0.0), 0.1, 0.4, 8.0, t, c)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_raycast_backward_poses_raw(t, w, c, (0.0, 0.0, 0.0), 0.1, K, poses, 8, 8, 1, 0.05, 1.0, torch.zeros(1, 2, 8, 8, dtype=torch.int32))
    with pytest.raises(TypeError, match="pose_gradients"):
        tk.kf(pose_gradients=1)
    assert tk.kf().pose_gradients is False and tk.kf(pose_gradients=True).pose_gradients is True


# ------------------------------------------------------------------ CPU: the formulas against float64 autograd
def test_integrate_pose_formulas_against_float64_autograd():
    sc = small_cpu_scene()
    poses = tilt(make_sequence(1, 3, 24, 32, seed=0)[3][0].numpy())
    K = make_intrinsics(24, 32)[0, 0].numpy()
    cent = ref_centres(sc["dims"], sc["v"], sc["origin"])
    proj = [tt.np_project(cent, poses[l], K, 24, 32) for l in range(3)]
    act, pix, z = (np.stack([p[k] for p in proj]) for k in range(3))
    rng = np.random.RandomState(3)
    n = sc["n"]
    f0, w0, c0 = rng.uniform(-1, 1, n), rng.randint(0, 3, n).astype(np.float64), rng.uniform(0, 255, (n, 3))
    _, _, _, rec = ref_integrate(act, pix, z, sc["depth"], sc["rgb"], f0, w0, c0, 0.15, 2.0)
    assert sum(int(r["lin"].sum()) for r in rec) > 50 and sum(int(r["sat"].sum()) for r in rec) > 0
    g_f = rng.randn(n)
    # the forward again with the pose as the variable: the voxel's depth z = sum_j R[j][2] (c_j - t_j) enters through sdf = d - z;
    # torch_integrate reads depth[l][pix[l]] - z[l], so it is handed d - z per voxel and the identity for the pixels
    P = torch.tensor(poses.astype(np.float64), requires_grad=True)
    cz = torch.from_numpy(cent.astype(np.float64))
    zt = [((cz - P[l, :3, 3]) * P[l, :3, 2]).sum(-1) for l in range(3)]
    d_eff = [torch.from_numpy(sc["depth"][l][pix[l]].astype(np.float64)) - zt[l] for l in range(3)]
    rgb_eff = [torch.from_numpy(sc["rgb"][l][pix[l]].astype(np.float64)) for l in range(3)]
    ident = [np.arange(n)] * 3
    out_f, _ = torch_integrate(rec, ident, np.zeros((3, n)), d_eff, rgb_eff, torch.tensor(f0), torch.tensor(c0), 0.15)
    (out_f * torch.from_numpy(g_f)).sum().backward()
    got = ref_integrate_pose_backward(rec, cent, poses, g_f, 0.15)
    want = P.grad.numpy()
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert (got[:, :3, 2] != 0).any(0).all() and (got[:, :3, 3] != 0).any(0).all()  # all six entries, none by accident
    assert not got[:, 3].any() and not got[:, :, :2].any() and not want[:, 3].any() and not want[:, :, :2].any()
    A = ref_integrate_pose_backward(rec, cent, poses, g_f, 0.15, absolute=True)
    assert (A >= np.abs(got) * (1 - 1e-12)).all()


def torch_cast_pose(vol, rec, K, Ho, Wo, stride, P, color):
    """Depth and rgb of the hit pixels in torch float64 with the pose P (4, 4) as the variable and the decisions of rec (ending
    sample, cells) as constants.  The positions are written as rec's own values plus what the pose moves them by, so that at P
    itself every sample is rec's, digit for digit: p(P) = p_rec + (t - t.detach()) + z (R - R.detach()) d."""
    dims, v = vol["dims"], float(F32(vol["v"]))
    hit = rec["hit"]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    D = lambda x: T(x[hit].astype(np.float64))
    dx, dy = (D(x) for x in cast_dirs(K, Ho, Wo, stride))
    d = torch.stack([dx, dy, torch.ones_like(dx)], -1)
    R, t = P[:3, :3], P[:3, 3]
    moved = lambda z: (t - t.detach()) + z[:, None] * (d @ (R - R.detach()).T)  # what the pose adds to a position at depth z
    tsdf = T(vol["tsdf"].reshape(-1).astype(np.float64))
    k, dz = D(rec["k"]), D(rec["dz"])
    z0 = T(((rec["k"][hit] - 1).astype(F32) * rec["dz"][hit]).astype(np.float64))
    z1 = T((rec["k"][hit].astype(F32) * rec["dz"][hit]).astype(np.float64))
    f0 = tr.trilerp_t(tsdf[T(tr.corner_ids(rec["i0"][hit], dims))], D(rec["a0"]) + moved(z0) / v)
    f1 = tr.trilerp_t(tsdf[T(tr.corner_ids(rec["i1"][hit], dims))], D(rec["a1"]) + moved(z1) / v)
    z = ((k - 1) + f0 / (f0 - f1)) * dz
    p = T(rec["t"].astype(np.float64)) + z[:, None] * D(rec["dw"]) + moved(z)
    a = (p - T(np.asarray(vol["origin"], F32).astype(np.float64))) / v - 0.5 - D(rec["ih"])
    ids = T(tr.corner_ids(rec["ih"][hit], dims))
    return z, torch.stack([tr.trilerp_t(color[:, ch][ids], a) for ch in range(3)], -1)


def test_cast_pose_formulas_against_float64_autograd():
    vol = host_volume(0)
    ref = reference(0, "rotated", STEPS[0])
    rec = ref["rec"]
    hit = rec["hit"]
    assert hit.sum() > 1000
    rng = np.random.RandomState(0)
    gd, gc = rng.randn(tr.H, tr.W), rng.randn(tr.H, tr.W, 3)
    P = torch.tensor(POSES["rotated"].astype(np.float64), requires_grad=True)
    cc = torch.from_numpy(vol["color"].reshape(-1, 3).astype(np.float64))
    z, rgb = torch_cast_pose(vol, rec, tr.make_K(), tr.H, tr.W, 1, P, cc)
    z_ref, rgb_ref = torch_cast(vol, rec, torch.from_numpy(vol["tsdf"].reshape(-1).astype(np.float64)), cc)  # the same forward
    assert (z - z_ref).abs().max() < 1e-12 and (rgb - rgb_ref).abs().max() < 1e-12
    assert np.abs(z.detach().numpy() - ref["depth"].reshape(-1)[hit]).max() < 1e-12
    ((z * torch.from_numpy(gd.reshape(-1)[hit])).sum() + (rgb * torch.from_numpy(gc.reshape(-1, 3)[hit])).sum()).backward()
    want = P.grad.numpy()
    got = ref_cast_pose_backward(vol, rec, tr.make_K(), tr.H, tr.W, 1, gd, gc)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert (got[:3] != 0).all() and not got[3].any() and not want[3].any()  # all twelve entries
    A = ref_cast_pose_backward(vol, rec, tr.make_K(), tr.H, tr.W, 1, gd, gc, absolute=True)
    assert (A >= np.abs(got) * (1 - 1e-12)).all()
    # the depth alone, into a volume without colours: the same formulas without w
    P0 = torch.tensor(POSES["rotated"].astype(np.float64), requires_grad=True)
    z, _ = torch_cast_pose(vol, rec, tr.make_K(), tr.H, tr.W, 1, P0, cc)
    (z * torch.from_numpy(gd.reshape(-1)[hit])).sum().backward()
    got0 = ref_cast_pose_backward(dict(vol, color=None), rec, tr.make_K(), tr.H, tr.W, 1, gd, None)
    assert np.abs(got0 - P0.grad.numpy()).max() <= 1e-10 * np.abs(got0).max() and np.abs(got0 - got).max() > 1e-3 * np.abs(got).max()


def test_closed_form_of_a_fronto_parallel_plane():
    """The plane z = 1 seen with the identity pose, one frame, a prior weight W everywhere, g_tsdf = 1 on the linear band: every
    such voxel sends gd = 1 / ((W + 1) trunc), so S0 = N_lin / ((W + 1) trunc) and S_j = gd sum_lin c_j; R[j][2] = (0, 0, 1)."""
    hh, ww, z_plane, v, trunc, Wp = 24, 32, 1.0, 0.05, 0.15, 1.0
    dims, origin = (6, 5, 12), (-0.15, -0.125, 0.6)
    cent = ref_centres(dims, v, origin)
    act, pix, z = tt.np_project(cent, np.eye(4), make_intrinsics(hh, ww)[0, 0].numpy(), hh, ww)
    depth = np.full((1, hh * ww), z_plane, F32)
    n = len(cent)
    _, _, _, rec = ref_integrate(act[None], pix[None], z[None], depth, None, np.ones(n), np.full(n, Wp), None, trunc, 8.0)
    lin = rec[0]["lin"]
    N_lin = int(lin.sum())
    assert 0 < N_lin < int(rec[0]["upd"].sum())  # some updated voxels are saturated: they send nothing
    got = ref_integrate_pose_backward(rec, cent, np.eye(4)[None], lin.astype(np.float64), trunc)
    t32 = float(F32(trunc))
    gd = 1.0 / ((Wp + 1.0) * t32)
    assert got[0, 0, 3] == 0.0 and got[0, 1, 3] == 0.0
    assert abs(got[0, 2, 3] - N_lin * gd) <= 1e-12 * N_lin * gd
    np.testing.assert_allclose(got[0, :3, 2], -gd * cent[lin].astype(np.float64).sum(0), rtol=1e-12, atol=1e-12)
    assert not got[0, 3].any() and not got[0, :, :2].any()


def cpu_integrate_records(L):
    """The integration scene with the CPU's decisions (np_project): per batch element rec; the upstream adjoint with the ties zeroed."""
    colors, depths, K, poses = integrate_scene(L)
    f0, w0, c0, g_f, _ = integrate_inputs(L)
    recs, g_f = [], g_f.copy()
    for b in range(I_B):
        cent = ref_centres(I_DIMS, tt.V, I_ORIGINS[b])
        proj = [tt.np_project(cent, poses[b, l].numpy(), K[b, 0].numpy(), I_H, I_W) for l in range(L)]
        act, pix, z = (np.stack([p[k] for p in proj]) for k in range(3))
        rec = ref_integrate(act, pix, z, depths[b].reshape(L, -1).numpy(), None, f0[b], w0[b], None, tt.TRUNC, 2.0)[3]
        g_f[b][np.any([r["tie"] for r in rec], 0)] = 0
        recs.append(rec)
    return recs, poses.numpy(), g_f


def test_float32_transcriptions_stay_within_what_the_bounds_were_built_from():
    worst_i = np.zeros(2)
    for L in (3, 33):
        recs, P, g_f = cpu_integrate_records(L)
        assert sum(int(r["lin"].sum()) for rec in recs for r in rec) > 200 * L // 3
        assert any((r["W"][r["upd"]] == 2).any() for rec in recs for r in rec)  # the cap acts
        w, want, A = integrate_deviation(recs, P, g_f)
        assert (want[:, :, :3, 2:] != 0).all(), "every camera updates voxels inside the band"
        worst_i = np.maximum(worst_i, w)
    print("integrate: float32 transcription against float64, in units of 2^-24 A: rotation column %.3g, translation column %.3g" % tuple(worst_i))
    assert (worst_i <= np.array(INTEGRATE_DEV)).all() and (worst_i >= 0.5 * np.array(INTEGRATE_DEV)).all(), worst_i
    worst_c = np.zeros(2)
    for step in STEPS:
        for stride in (1, 3):
            for color in (True, False):
                w, want, A = cast_deviation(step, stride, color)
                worst_c = np.maximum(worst_c, w)
                assert (want[0, :, :3] != 0).all() and not want[:, :, 3].any()
            for b in range(2):
                for name in C_NAMES[b]:
                    assert cast_records(b, name, step, stride)[2] <= 0.05
    print("cast: float32 transcription against float64, in units of 2^-24 A: rotation block %.3g, translation column %.3g" % tuple(worst_c))
    assert (worst_c <= np.array(CAST_DEV)).all() and (worst_c >= 0.5 * np.array(CAST_DEV)).all(), worst_c
    r = cast20(0, "identity", STEPS[0], 1)["rec"]
    assert (r["dw"][:, 0] == 0).sum() == C_H and (r["dw"][:, 1] == 0).sum() == C_W  # rays parallel to an axis
    assert (cast20(1, "inside", STEPS[0], 1)["k_end"] > 0).mean() < 0.05  # almost no hits


# ------------------------------------------------------------------ GPU: integration
def to_dev(*xs):
    return tuple(None if x is None else x.to(DEV) for x in xs)


def check_entries(got, want, A, bound, what):
    """|got - want| <= bound[kind] * 2^-24 * A per entry (kind 0: rotation entries, 1: the translation column); what no term
    touches (A = 0) is exactly zero."""
    assert np.isfinite(got).all(), what
    assert (got[A == 0] == 0).all(), what
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / (U * A)
    rot, tra = np.nanmax(r[..., :3, :3], initial=0.0), np.nanmax(r[..., :3, 3], initial=0.0)
    print(what, "largest error in units of 2^-24 A: rotation %.3g (bound %.3g), translation %.3g (bound %.3g)" % (rot, bound[0], tra, bound[1]))
    assert rot <= bound[0] and tra <= bound[1], what


@pytest.mark.gpu
@pytest.mark.parametrize("color", [True, False], ids=["color", "no_color"])
@pytest.mark.parametrize("L", [3, 33])
def test_integrate_pose_gradient_matches_the_float64_reference(L, color):
    """Measured on the MI355X, in units of 2^-24 A: 0.27 / 0.15 (L = 3) and 1.07 / 0.78 (L = 33) for the rotation column /
    translation column -- the transcription's figures; the bound is 4 x INTEGRATE_DEV = 4.4 / 3.2."""
    seq = to_dev(*integrate_scene(L))
    colors, depths, K, poses = seq
    f0, w0, c0, g_f, g_c = integrate_inputs(L)
    n = I_DIMS[0] * I_DIMS[1] * I_DIMS[2]
    ref, _ = tt.reference_state(I_DIMS, I_ORIGINS, seq, f0, w0, c0, maxw=2.0)  # the device's own pixels, float64 updates
    g_f = g_f.copy()
    for b in range(I_B):
        tie = np.any([r["tie"] for r in ref[b][3]], 0)
        assert tie.mean() <= 0.02
        g_f[b][tie] = 0
        g_c[b][tie] = 0
    shape = (I_B, I_DIMS[2], I_DIMS[1], I_DIMS[0])
    dev = lambda x, s: torch.from_numpy(x).reshape(s).to(DEV)
    origin = ops.tsdf_origin(I_ORIGINS, I_B, DEV)
    args = (depths, K, poses, dev(w0, shape), origin, tt.V, tt.TRUNC, 2.0, dev(g_f, shape), dev(g_c, shape + (3,)) if color else None)
    out = ops.tsdf_integrate_backward_poses_raw(*args)
    g_poses = out[4]
    assert g_poses.shape == (I_B, L, 4, 4)
    P = poses.cpu().numpy()
    want = np.stack([ref_integrate_pose_backward(ref[b][3], ref_centres(I_DIMS, tt.V, I_ORIGINS[b]), P[b], g_f[b], tt.TRUNC)
                     for b in range(I_B)])
    A = np.stack([ref_integrate_pose_backward(ref[b][3], ref_centres(I_DIMS, tt.V, I_ORIGINS[b]), P[b], g_f[b], tt.TRUNC, absolute=True)
                  for b in range(I_B)])
    assert (want[:, :, :3, 2:] != 0).all()
    check_entries(g_poses.cpu().numpy().astype(np.float64), want, A, 4 * np.array(INTEGRATE_DEV), "integrate L=%d" % L)
    # the other four outputs are the old entry point's, bit for bit
    old = ops.tsdf_integrate_backward_raw(*args)
    for a, b in zip(out[:4], old):
        assert (a is None and b is None) or torch.equal(a, b)
    assert (old[3] is None) == (not color)
    # the same bits from run to run, with the flag on and off; and without the outputs nobody asks for
    for flag in (True, False):
        torch.use_deterministic_algorithms(flag)
        try:
            again = ops.tsdf_integrate_backward_poses_raw(*args)
        finally:
            torch.use_deterministic_algorithms(False)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(again, out)), flag
    alone = ops.tsdf_integrate_backward_poses_raw(*args, want_state=False, want_frames=False)
    assert alone[:4] == (None, None, None, None) and torch.equal(alone[4], g_poses)
    frames_only = ops.tsdf_integrate_backward_poses_raw(*args, want_state=False)
    assert frames_only[0] is None and torch.equal(frames_only[2], out[2]) and torch.equal(frames_only[4], g_poses)
    assert color is False or torch.equal(frames_only[3], out[3])


# ------------------------------------------------------------------ GPU: ray cast
def cast_cameras():
    K = torch.from_numpy(make_K20()).view(1, 1, 4, 4).repeat(2, 1, 1, 1).to(DEV)
    poses = torch.from_numpy(np.stack([np.stack([POSES[n] for n in C_NAMES[b]]) for b in range(2)])).to(DEV)
    return K, poses


@pytest.mark.gpu
@pytest.mark.parametrize("color", [True, False], ids=["color", "no_color"])
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("stride", [1, 3])
def test_cast_pose_gradient_matches_the_float64_reference(stride, step, color):
    """Measured on the MI355X, in units of 2^-24 A: at most 2.6 (rotation block) and 1.3 (translation column) over the eight cases
    -- the transcription's figures; the bound is 4 x CAST_DEV = 10.8 / 5.4."""
    vol = tr.device_volume(color=color)
    K, poses = cast_cameras()
    Ho, Wo = -(-C_H // stride), -(-C_W // stride)
    fwd = ops.tsdf_raycast_raw(vol.tsdf, vol.weight, vol.color, vol.origin, tr.V, K, poses, C_H, C_W, stride, step)
    k_dev = fwd[3].cpu().numpy()
    tape = np.zeros((2, 2, Ho, Wo), np.int32)
    for b in range(2):
        for l, name in enumerate(C_NAMES[b]):
            rec, t, share = cast_records(b, name, step, stride)
            assert share <= 0.05
            good = ~cast20(b, name, step, stride)["tie"]
            assert np.array_equal(k_dev[b, l][good], t[good]), (b, name)  # the device's tape is the reference's off the ties
            tape[b, l] = np.where(good, k_dev[b, l], 0)
    gd, gc = cast_upstream(stride)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    args = (vol.tsdf, vol.weight, vol.color, vol.origin, tr.V, K, poses, C_H, C_W, stride, step, 1.0, dev(tape), dev(gd),
            dev(gc) if color else None)
    g_t, g_c, g_poses = ops.tsdf_raycast_backward_poses_raw(*args)
    _, want, A = cast_deviation(step, stride, color)
    got = g_poses.cpu().numpy()
    assert got.shape == (2, 2, 4, 4) and (tape[0] > 0).sum() > 200 // stride ** 2
    assert (tape[1, 0] > 0).mean() < 0.05 and np.isfinite(got).all()  # "inside": almost no hits, and no NaN from them
    for b in range(2):
        for l in range(2):
            if not (tape[b, l] > 0).any():
                assert not got[b, l].any()  # exact zeros
    check_entries(got.astype(np.float64), want, A, 4 * np.array(CAST_DEV), "cast stride=%d step=%g" % (stride, step))
    old = ops.tsdf_raycast_backward_raw(*args)
    assert torch.equal(g_t, old[0]) and ((g_c is None and old[1] is None) or torch.equal(g_c, old[1]))
    for flag in (True, False):
        torch.use_deterministic_algorithms(flag)
        try:
            again = ops.tsdf_raycast_backward_poses_raw(*args)
        finally:
            torch.use_deterministic_algorithms(False)
        assert torch.equal(again[2], g_poses) and torch.equal(again[0], g_t), flag
    alone = ops.tsdf_raycast_backward_poses_raw(*args, want_volume=False)
    assert alone[0] is None and alone[1] is None and torch.equal(alone[2], g_poses)


@pytest.mark.gpu
def test_a_cast_without_hits_gives_exact_zeros():
    vol = tr.device_volume(bs=(0,))
    K = torch.from_numpy(make_K20()).view(1, 1, 4, 4).to(DEV)
    away = torch.eye(4, device=DEV).view(1, 1, 4, 4).clone()
    away[0, 0, 2, 3] = 50.0  # behind the volume, looking away
    depth, _, rgb, k_end = ops.tsdf_raycast_raw(vol.tsdf, vol.weight, vol.color, vol.origin, tr.V, K, away, C_H, C_W, 1, STEPS[0])
    assert not k_end.any()
    g = ops.tsdf_raycast_backward_poses_raw(vol.tsdf, vol.weight, vol.color, vol.origin, tr.V, K, away, C_H, C_W, 1, STEPS[0], 1.0, k_end,
                                            torch.ones_like(depth), torch.ones_like(rgb))
    assert not g[2].any() and not g[0].any() and g[2].shape == (1, 1, 4, 4)


# ------------------------------------------------------------------ GPU: the autograd nodes
@pytest.mark.gpu
def test_integrate_node_hands_the_pose_gradient_on():
    L = 3
    colors, depths, K, poses = to_dev(*integrate_scene(L))
    f0, w0, c0, g_f, g_c = integrate_inputs(L)
    shape = (I_B, I_DIMS[2], I_DIMS[1], I_DIMS[0])
    dev = lambda x, s: torch.from_numpy(x).reshape(s).to(DEV)
    origin = ops.tsdf_origin(I_ORIGINS, I_B, DEV)
    up = [dev(g_f, shape), dev(g_c, shape + (3,))]

    def run(p):
        d, c = depths.clone().requires_grad_(True), colors.clone().requires_grad_(True)
        t, col = dev(f0, shape).requires_grad_(True), dev(c0, shape + (3,)).requires_grad_(True)
        out_t, out_w, out_c = ops.tsdf_integrate(d, c, K, p, t, dev(w0, shape), col, origin, tt.V, tt.TRUNC, 2.0)
        torch.autograd.backward([out_t, out_c], up)
        return (out_t.detach(), out_w, out_c.detach()), (t.grad, col.grad, d.grad, c.grad)

    p = poses.clone().requires_grad_(True)
    state, grads = run(p)
    raw = ops.tsdf_integrate_backward_poses_raw(depths, K, poses, dev(w0, shape), origin, tt.V, tt.TRUNC, 2.0, *up)
    assert p.grad is not None and torch.equal(p.grad, raw[4]) and bool(p.grad.any())  # (None on the parent commit)
    state0, grads0 = run(poses)            # poses that require no gradient: the old reverse pass
    state1, grads1 = run(poses.detach().clone())
    for a, b, c in zip(state + grads, state0 + grads0, state1 + grads1):
        assert torch.equal(a, b) and torch.equal(b, c)
    # the pose gradient alone: nothing else requires one
    p2 = poses.clone().requires_grad_(True)
    out_t, _, _ = ops.tsdf_integrate(depths, colors, K, p2, dev(f0, shape), dev(w0, shape), dev(c0, shape + (3,)), origin, tt.V, tt.TRUNC, 2.0)
    out_t.backward(up[0])
    want = ops.tsdf_integrate_backward_poses_raw(depths, K, poses, dev(w0, shape), origin, tt.V, tt.TRUNC, 2.0, up[0], None)[4]
    assert torch.equal(p2.grad, want)
    # TSDFVolume.integrate records the graph for poses alone
    vol = gs.TSDFVolume(I_DIMS, tt.V, origin=I_ORIGINS, trunc=tt.TRUNC, max_weight=2.0, device=DEV)
    p3 = poses.clone().requires_grad_(True)
    fused = vol.integrate(gs.RGBDImages(colors, depths, K, p3))
    assert fused.tsdf.requires_grad
    fused.tsdf.sum().backward()
    assert p3.grad is not None and bool(p3.grad.any())


@pytest.mark.gpu
def test_raycast_node_hands_the_pose_gradient_on_and_the_frames_stay_attached():
    vol = tr.device_volume()
    K, poses = cast_cameras()
    stride, step = 1, STEPS[0]
    gd, gc = cast_upstream(stride)
    gd, gc = torch.from_numpy(gd).to(DEV), torch.from_numpy(gc).to(DEV)

    def run(p):
        t, c = vol.tsdf.clone().requires_grad_(True), vol.color.clone().requires_grad_(True)
        depth, normal, rgb, k_end = ops.tsdf_raycast(t, vol.weight, c, vol.origin, tr.V, K, p, C_H, C_W, stride, step)
        torch.autograd.backward([depth, rgb], [gd, gc])
        return (depth.detach(), normal, rgb.detach(), k_end), (t.grad, c.grad)

    p = poses.clone().requires_grad_(True)
    outs, grads = run(p)
    raw = ops.tsdf_raycast_backward_poses_raw(vol.tsdf, vol.weight, vol.color, vol.origin, tr.V, K, poses, C_H, C_W, stride, step, 1.0,
                                              outs[3], gd, gc)
    assert p.grad is not None and torch.equal(p.grad, raw[2]) and bool(p.grad.any())  # (None on the parent commit)
    outs0, grads0 = run(poses)
    outs1, grads1 = run(poses.detach().clone())
    for a, b, c in zip(outs + grads, outs0 + grads0, outs1 + grads1):
        assert torch.equal(a, b) and torch.equal(b, c)
    # TSDFVolume.raycast: the returned frames carry the poses attached only when they require a gradient
    assert not vol.raycast(K, poses, C_H, C_W).poses.requires_grad
    p2 = poses[:, :1].clone().requires_grad_(True)
    frames = vol.raycast(K, p2, C_H, C_W)
    assert frames.poses.requires_grad and frames.depth_image.requires_grad
    with torch.no_grad():
        assert not vol.raycast(K, p2, C_H, C_W).poses.requires_grad
    # raycast_pointcloud's points carry the pose gradient through the depth and through the vertex map
    pc = vol.raycast_pointcloud(K, p2, C_H, C_W)
    pc.points_padded.sum().backward()
    both = p2.grad.clone()
    assert torch.isfinite(both).all() and bool(both[:, :, :3].any())
    p3 = poses[:, :1].clone().requires_grad_(True)
    vol.raycast(K, p3, C_H, C_W).depth_image.sum().backward()
    assert not torch.equal(both, p3.grad)


# ------------------------------------------------------------------ GPU: what it is for -- a pose refined against the volume
R_H, R_W, R_FRAME = 48, 64, 3
R_DT, R_DR = 0.01, np.deg2rad(0.3)


def refine_setup():
    """The 48 x 64 sequence of test_kinectfusion.py, the perturbed pose of frame 3 and the true one (host tensors)."""
    colors, depths, K, poses = make_sequence(1, tk.L, R_H, R_W, seed=0)
    true = poses[0, R_FRAME].double()
    xi0 = torch.tensor([R_DT * 0.6, -R_DT * 0.64, R_DT * 0.48, R_DR * 0.48, R_DR * 0.6, -R_DR * 0.64], dtype=torch.float64)  # 1 cm, 0.3 deg
    start = se3utils.se3_exp(xi0) @ true
    return colors, depths, K, poses, true, start


def pose_errors(P, true):
    """(translation [m], rotation [rad]) between two 4 x 4 poses."""
    P, true = P.detach().double().cpu(), true.double().cpu()
    dR = P[:3, :3] @ true[:3, :3].T
    return float((P[:3, 3] - true[:3, 3]).norm()), float(torch.acos(torch.clamp((torch.trace(dR) - 1) / 2, -1.0, 1.0)))


def refine(loss_and_grad, start, dtype, device, steps=15):
    """Plain gradient steps on xi with backtracking: P = se3_exp(xi) start; a step is halved until the loss falls; the next one
    starts from twice the accepted size.  No trial step is longer than the perturbation itself (|t g| <= 1 cm in xi): the loss
    is a sum over the hits, so a step that throws the camera off the volume would "lower" it to zero.
    -> (xi, the losses of the accepted steps)."""
    xi = torch.zeros(6, dtype=dtype, device=device)
    loss, g = loss_and_grad(xi)
    losses, t = [loss], 1.0
    for _ in range(steps):
        t = min(t, R_DT / float(g.norm()))
        for _ in range(60):
            cand = xi - t * g
            l2, g2 = loss_and_grad(cand)
            if l2 < loss:
                break
            t *= 0.5
        else:
            raise AssertionError("no step lowers the loss")
        xi, loss, g, t = cand, l2, g2, 2.0 * t
        losses.append(loss)
    return xi, losses


def refine_reference():
    """The loop with the float64 reference on the CPU (the integration: ref_integrate with np_project's pixels; the cast:
    ref_cast in float64; the pose adjoint: ref_cast_pose_backward) -> (final translation error, final rotation error, losses)."""
    colors, depths, K, poses, true, start = refine_setup()
    dims, v, trunc, origin = tk.DIMS, tk.V, tk.TRUNC, tk.ORIGINS[0]
    cent = ref_centres(dims, v, origin)
    Kn = K[0, 0].numpy()
    proj = [tt.np_project(cent, poses[0, l].numpy(), Kn, R_H, R_W) for l in range(tk.L)]
    act, pix, z = (np.stack([p[k] for p in proj]) for k in range(3))
    n = len(cent)
    f, w, _, _ = ref_integrate(act, pix, z, depths[0].reshape(tk.L, -1).numpy(), None, np.ones(n), np.zeros(n), None, trunc, 128.0)
    shape = (dims[2], dims[1], dims[0])
    vol = dict(tsdf=f.astype(F32).reshape(shape), weight=w.astype(F32).reshape(shape), color=None, origin=origin, v=v, dims=dims)
    obs = depths[0, R_FRAME, :, :, 0].double().numpy()

    def loss_and_grad(xi):
        xi = xi.detach().clone().requires_grad_(True)
        P = se3utils.se3_exp(xi) @ start
        r = ref_cast(vol, Kn, P.detach().float().numpy(), R_H, R_W, 1, trunc / 2)
        m = (r["depth"] > 0) & (obs > 0)
        diff = np.where(m, r["depth"] - obs, 0.0)
        gP = ref_cast_pose_backward(vol, r["rec"], Kn, R_H, R_W, 1, 2.0 * diff, None)
        P.backward(torch.from_numpy(gP))
        return float((diff ** 2).sum()), xi.grad.detach()

    xi, losses = refine(loss_and_grad, start, torch.float64, "cpu")
    return pose_errors(se3utils.se3_exp(xi) @ start, true) + (losses,)


def test_reference_refinement_reaches_the_recorded_errors():
    """The float64 loop on the CPU (about 30 casts of 48 x 64 pixels): 1 cm -> 1.7 mm, 0.3 degrees = 5.2e-3 rad -> 1.1e-3 rad."""
    t1, r1, losses = refine_reference()
    print("reference refinement: translation %.3g m, rotation %.3g rad, loss %.3g -> %.3g" % (t1, r1, losses[0], losses[-1]))
    assert len(losses) == 16 and all(b < a for a, b in zip(losses, losses[1:]))
    assert abs(t1 / REFINE_REF[0] - 1) <= 0.05 and abs(r1 / REFINE_REF[1] - 1) <= 0.05  # the recorded figures, to their digits


@pytest.mark.gpu
def test_a_perturbed_pose_is_refined_against_the_volume():
    """Frame 3's pose, off by 1 cm and 0.3 degrees, is pulled back by minimising sum_hit (cast depth - observed depth)^2 through
    the cast's pose gradient.  The device ends within twice the errors the same loop reaches with the float64 reference."""
    colors, depths, K, poses, true, start = refine_setup()
    c, d, Kd, Pd = to_dev(colors, depths, K, poses)
    vol = gs.TSDFVolume(tk.DIMS, tk.V, origin=[tk.ORIGINS[0]], trunc=tk.TRUNC, color=False, device=DEV).integrate(gs.RGBDImages(c, d, Kd, Pd))
    obs = d[:, R_FRAME:R_FRAME + 1, :, :, 0]
    start_d = start.float().to(DEV)

    def loss_and_grad(xi):
        xi = xi.detach().clone().requires_grad_(True)
        P = (se3utils.se3_exp(xi) @ start_d).view(1, 1, 4, 4)
        depth = ops.tsdf_raycast(vol.tsdf, vol.weight, None, vol.origin, tk.V, Kd, P, R_H, R_W, 1, tk.TRUNC / 2)[0]
        m = (depth > 0) & (obs > 0)
        loss = (torch.where(m, depth - obs, torch.zeros_like(depth)) ** 2).sum()
        loss.backward()
        return float(loss.detach()), xi.grad.detach()

    t0, r0 = pose_errors(start, true)
    assert abs(t0 - R_DT) < 1e-3 and abs(r0 - R_DR) < 1e-4
    xi, losses = refine(loss_and_grad, start, torch.float32, DEV)
    t1, r1 = pose_errors(se3utils.se3_exp(xi.double().cpu()) @ start, true)
    print("pose refinement: translation %.3g -> %.3g m (reference %.3g), rotation %.3g -> %.3g rad (reference %.3g), loss %.3g -> %.3g"
          % (t0, t1, REFINE_REF[0], r0, r1, REFINE_REF[1], losses[0], losses[-1]))
    assert len(losses) == 16 and all(b < a for a, b in zip(losses, losses[1:]))
    assert t1 < t0 and r1 < r0
    assert t1 <= 2 * REFINE_REF[0] and r1 <= 2 * REFINE_REF[1]


# ------------------------------------------------------------------ GPU: KinectFusion
@pytest.mark.gpu
def test_kinectfusion_default_is_the_old_graph_and_the_flag_closes_the_chain():
    base = tk.frames(1)
    L = 4

    def run(**kw):
        d = base.depth_image[:, :L].clone().requires_grad_(True)
        _, poses = tk.kf(1, **kw)(gs.RGBDImages(base.rgb_image[:, :L], d, base.intrinsics, base.poses[:, :L]))
        poses[:, -1].sum().backward()
        return poses.detach(), d.grad

    def by_hand():
        """The public pieces with the poses given to the volume detached: the graph as it was before the poses had gradients."""
        d = base.depth_image[:, :L].clone().requires_grad_(True)
        slam = tk.kf(1)
        vol = slam.new_volume(1)
        pose, out = base.poses[:, :1], []
        for s in range(L):
            rgb_s, d_s = base.rgb_image[:, s:s + 1], d[:, s:s + 1]
            if s > 0:
                target = vol.raycast_pointcloud(base.intrinsics, pose.detach(), tk.H, tk.W, stride=4, step=None, min_weight=1.0)
                source = tk.downsample_rgbdimages(gs.RGBDImages(rgb_s, d_s, base.intrinsics, pose), 4)
                T = slam.odomprov.provide(target, source)
                pose = tk.compose_transformations(T.squeeze(1), pose.squeeze(1)).unsqueeze(1)
            vol = vol.integrate(gs.RGBDImages(rgb_s, d_s, base.intrinsics, pose.detach()))
            out.append(pose[:, 0])
        poses = torch.stack(out, 1)
        poses[:, -1].sum().backward()
        return poses.detach(), d.grad

    torch.use_deterministic_algorithms(True)
    try:
        p0, g0 = run()
        ph, gh = by_hand()
        p1, g1 = run(pose_gradients=True)
        p2, g2 = run(pose_gradients=True)
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(p0, ph) and torch.equal(g0, gh)
    assert torch.equal(p1, p0) and torch.isfinite(g1).all() and not torch.equal(g1, g0)
    assert torch.equal(p1, p2) and torch.equal(g1, g2)
    with pytest.raises(NotImplementedError, match="gradients"):
        d = base.depth_image[:, :2].clone().requires_grad_(True)
        tk.kf(1, odom="rgbd", pose_gradients=True)(gs.RGBDImages(base.rgb_image[:, :2], d, base.intrinsics, base.poses[:, :2]))
