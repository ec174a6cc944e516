"""SDF odometry (csrc/sdf.hip; ops.sdf_*; gs.odometry.SDFOdometryProvider; KinectFusion(odom="sdf")).

The references live here, in numpy (the reference project has no counterpart): `ref_*` are the rule of include/gradslam_hip.h
vectorised over the pixels and written ONCE for a number type `dt`.  With dt = float64 they are the reference; with dt = float32
they are a transcription of the device's operations in the device's order (the library is built without contraction), which
measures what fp32 alone costs: ROWS_TRANSCRIPTION and T_TRANSCRIPTION below hold its largest deviations from float64, measured on
the CPU over every case of this file (test_float32_transcription_stays_within_its_recorded_deviation recomputes them), and the
device must agree with float64 within FOUR times those (the project's margin).  The sums are checked against
tests.helpers.exact_sum_f32 of the products formed in fp32 from the device's own rows.

Scene (host, float64, no files, no GPU): the volume is analytic -- tsdf = min(1, sdf / trunc) of a tilted plane with a sphere in
front of it (and a second sphere beside it: a plane and one sphere alone leave the rotation about the sphere's axis free), weight 1
except 0 more than trunc behind the surface and 0 in one unobserved slab (different per batch element); dims 24 x 20 x 16.  The
depth images are rendered from the TRUE cameras and have holes; the frames carry poses that are off by DELTAS (1.5 voxels and
0.5 degrees), so the true answer of the alignment is DELTAS[b].  B = 2 with different origins, slabs, holes and motions.

Pixels left out of the row comparison (fp32 and float64 may decide differently there), as float64 sees them: a cell coordinate g
within 1e-5 of an integer on any axis (the volume's border is the integers 0 and n - 1 of that coordinate); at most 5 % of the
pixels.  Every other decision reads stored fp32 values (depth, weights, corner values) and cannot differ.
"""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops
from tests.helpers import exact_sum_f32

DEV = "cuda:0"
U = 2.0 ** -24
NEW_SYMBOLS = {"gs_sdf_odometry_ws_size": 4, "gs_sdf_odometry": 25, "gs_sdf_rows": 23}
DAMP, TIE = 1e-8, 1e-5
DIMS, V, TRUNC = (24, 20, 16), 0.05, 0.15
F32 = lambda x: float(np.float32(x))
# (H, W, stride, levels, numiters finest first)
SIZES = {"48x64": (48, 64, 1, 3, (10, 5, 3)), "30x45": (30, 45, 1, 2, (8, 4)), "30x45s2": (30, 45, 2, 2, (8, 4)), "5x7": (5, 7, 1, 1, (6,))}
# the sums alone: more than 32 partial rows (49), and the first seam of reduce_partials (32 x 16 rows per round): 512 | 514 rows
MORE_SIZES = {"96x130": (96, 130, 1, 1, (1,)), "256x512": (256, 512, 1, 1, (1,)), "257x512": (257, 512, 1, 1, (1,))}
FOLD_ROWS = {"256x512": (512, 1), "257x512": (514, 2)}

# The float32 transcription's largest deviation from float64 (CPU, every case of this file; recomputed and asserted below).
#   rows: per group (J translation part, J rotation part, r), absolute, over the sizes, the batch elements and the three deltas
#   T:    per size (rotation entries, translation entries), absolute, after the whole loop and after the init run
ROWS_TRANSCRIPTION = (3.6e-6, 5.6e-6, 2.5e-7)
T_TRANSCRIPTION = {"48x64": (1.4e-7, 1.6e-7), "30x45": (1.7e-7, 1.5e-7), "30x45s2": (1.1e-7, 9.5e-8), "5x7": (1.2e-7, 1.3e-7)}
# "What it is for": the float64 reference's own error against the ground truth at 48 x 64 (translation m, rotation rad), the worse
# batch element: the discretisation of the volume (5 cm voxels, trilinear), not arithmetic.
RECOVER_REF_ERROR = (3.5e-3, 2.5e-3)


# ------------------------------------------------------------------ scene
def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def make_K(H, W):
    """(fx, fy, cx, cy) as the fp32 values the device gets: the image is a little wider than the volume."""
    return tuple(F32(k) for k in (1.1 * W, 1.1 * W, (W - 1) / 2.0, (H - 1) / 2.0))


PLANE_P0 = np.array([0.0, 0.0, 1.6])
PLANE_N = np.array([0.25, -0.15, -1.0]) / np.linalg.norm([0.25, -0.15, -1.0])
SPHERES = ((-0.25, 0.1, 1.42, 0.2), (0.28, -0.18, 1.45, 0.18))
ORIGINS = [(-0.6, -0.5, 1.1), (-0.58, -0.52, 1.12)]
SLABS = [(0, 9, 11), (1, 6, 8)]  # (axis, first, end): voxels first <= i_axis < end are unobserved
# the poses the frames CARRY (camera to world), per batch element
CARRIED = [make_pose(rot(0.010, -0.014, 0.008), (0.025, -0.012, 0.015)), make_pose(rot(-0.012, 0.009, -0.015), (-0.02, 0.018, -0.01))]
# the world-frame deltas to the true cameras: 1.5 voxels = 7.5 cm, 0.5 degrees
_w = np.deg2rad(0.5)
DELTAS = [make_pose(rot(*(_w * np.array([0.6, -0.64, 0.48]))), 1.5 * V * np.array([0.48, -0.6, 0.64])),
          make_pose(rot(*(_w * np.array([-0.48, 0.6, 0.64]))), 1.5 * V * np.array([-0.64, 0.48, -0.6]))]
TRUE = [DELTAS[b] @ CARRIED[b] for b in range(2)]


def scene_sdf(p):
    """Signed distance of the scene at p (..., 3), positive on the cameras' side: the smaller of the plane's and the spheres'."""
    out = (p - PLANE_P0) @ PLANE_N
    for (x, y, z, r) in SPHERES:
        out = np.minimum(out, np.linalg.norm(p - np.array([x, y, z]), axis=-1) - r)
    return out


def render(K, pose, H, W):
    """depth (H,W) float64 of the scene from the camera `pose` (camera-to-world): the nearest surface along the pixel's ray."""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)  # z-normalised: t is the camera depth
    dw, o = dc @ pose[:3, :3].T, pose[:3, 3]
    t = (PLANE_N @ (PLANE_P0 - o)) / (dw @ PLANE_N)
    for (x, y, z, r) in SPHERES:
        c = np.array([x, y, z])
        a, b, cc = (dw * dw).sum(-1), 2.0 * (dw @ (o - c)), ((o - c) ** 2).sum() - r * r
        disc = b * b - 4 * a * cc
        ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        t = np.where((ts > 0) & (ts < t), ts, t)
    return t


def punch(depth, b):
    """Holes: single pixels and a block, different per batch element (a 5 x 7 image: one pixel and a 1 x 2 block)."""
    H, W = depth.shape
    d = depth.copy()
    singles = ((0.25, 0.3), (0.6, 0.7), (0.8, 0.15)) if b == 0 else ((0.35, 0.55), (0.7, 0.2), (0.15, 0.85))
    for (fv, fu) in singles[: 3 if H >= 16 else 1]:
        d[int(fv * H), int(fu * W)] = 0.0
    v0, u0 = (int(0.5 * H), int(0.3 * W)) if b == 0 else (int(0.3 * H), int(0.6 * W))
    d[v0:v0 + (max(2, H // 8) if H >= 16 else 1), u0:u0 + max(2, W // 8)] = 0.0
    return d


@lru_cache(maxsize=None)
def volume(b):
    """Batch element b's volume as the fp32 arrays the device gets (x fastest), its origin and the slab's mask."""
    nx, ny, nz = DIMS
    o = np.array([F32(x) for x in ORIGINS[b]])
    idx = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"), -1)[..., ::-1]  # (nz, ny, nx, xyz)
    sdf = scene_sdf(o + (idx + 0.5) * F32(V))
    tsdf = np.minimum(1.0, sdf / F32(TRUNC)).astype(np.float32)
    axis, lo, hi = SLABS[b]
    slab = (idx[..., axis] >= lo) & (idx[..., axis] < hi)
    weight = np.where((sdf < -F32(TRUNC)) | slab, 0.0, 1.0).astype(np.float32)
    return dict(tsdf=tsdf, weight=weight, origin=o, slab=slab)


@lru_cache(maxsize=None)
def scene(name):
    """The frames of both batch elements as the fp32 arrays the device gets: depth (B,H,W); K; the carried poses P (B,4,4)."""
    H, W = {**SIZES, **MORE_SIZES}[name][:2]
    K = make_K(H, W)
    depth = np.stack([punch(render(K, TRUE[b], H, W), b) for b in range(2)]).astype(np.float32)
    return dict(depth=depth, K=K, P=np.stack(CARRIED).astype(np.float32), H=H, W=W)


def deltas(which):
    """The three (B,4,4) sets the rows are checked at: the true delta, the identity (1.5 voxels off), and a 15-degree turn about
    the volume's vertical axis that pushes one side of the image into clamped free space and the other behind the surface."""
    if which == "true":
        return np.stack(DELTAS).astype(np.float32)
    if which == "identity":
        return np.stack([np.eye(4)] * 2).astype(np.float32)
    out = []
    for b in range(2):
        c = np.array(ORIGINS[b]) + 0.5 * V * np.array(DIMS)
        R = rot(0.0, np.deg2rad(15.0) * (1 if b == 0 else -1), 0.0)
        out.append(make_pose(R, c - R @ c) @ DELTAS[b])
    return np.stack(out).astype(np.float32)


WHICH = ("true", "identity", "turned")


# ------------------------------------------------------------------ the rule, once, for a number type dt
def ref_rows(depth, K, P, D, vol, dt, stride=1, minw=1.0):
    """One linearisation of one batch element on the [::stride, ::stride] grid: (valid (Hs,Ws), rows (Hs,Ws,7), aux).  The fp32
    inputs (depth, K, P, D, the volume) are taken as they are and computed with in dt."""
    H, W = depth.shape
    nx, ny, nz = DIMS
    fx, fy, cx, cy = (dt(k) for k in K)
    P, D = P.astype(dt), D.astype(dt)
    d = depth[::stride, ::stride].astype(dt)
    h, w = np.meshgrid(np.arange(0, H, stride).astype(dt), np.arange(0, W, stride).astype(dt), indexing="ij")
    v, trunc = dt(np.float32(V)), dt(np.float32(TRUNC))
    o = vol["origin"].astype(dt)
    with np.errstate(all="ignore"):
        live = (d > 0) & np.isfinite(d)
        px, py = d * ((w - cx) / fx), d * ((h - cy) / fy)
        pw = [((P[i, 0] * px + P[i, 1] * py) + P[i, 2] * d) + P[i, 3] for i in range(3)]
        q = [((D[i, 0] * pw[0] + D[i, 1] * pw[1]) + D[i, 2] * pw[2]) + D[i, 3] for i in range(3)]
        g = [(q[k] - o[k]) / v - dt(0.5) for k in range(3)]
        fi = [np.floor(x) for x in g]
        inside = live
        for k, n in enumerate((nx, ny, nz)):
            inside = inside & (fi[k] >= 0) & (fi[k] + 1 <= n - 1)
        a = [g[k] - fi[k] for k in range(3)]
        ix, iy, iz = (np.where(inside, fi[k], 0).astype(np.int64) for k in range(3))
        corner = lambda A, c: A[iz + (c >> 2), iy + ((c >> 1) & 1), ix + (c & 1)]
        f = [corner(vol["tsdf"], c).astype(dt) for c in range(8)]
        wt = [corner(vol["weight"], c) for c in range(8)]
        seen = inside & np.all([x >= np.float32(minw) for x in wt], 0)
        near = np.all([corner(vol["tsdf"], c) < np.float32(1.0) for c in range(8)], 0)
        ok = seen & near
        lerp = lambda p_, q_, s: p_ + s * (q_ - p_)
        ax, ay, az = a
        fh = lerp(lerp(lerp(f[0], f[1], ax), lerp(f[2], f[3], ax), ay), lerp(lerp(f[4], f[5], ax), lerp(f[6], f[7], ax), ay), az)
        gx = lerp(lerp(f[1] - f[0], f[3] - f[2], ay), lerp(f[5] - f[4], f[7] - f[6], ay), az)
        gy = lerp(lerp(f[2] - f[0], f[3] - f[1], ax), lerp(f[6] - f[4], f[7] - f[5], ax), az)
        gz = lerp(lerp(f[4] - f[0], f[5] - f[1], ax), lerp(f[6] - f[2], f[7] - f[3], ax), ay)
        kappa = trunc / v
        r = trunc * fh
        n0, n1, n2 = kappa * gx, kappa * gy, kappa * gz
        cols = [n0, n1, n2, q[1] * n2 - q[2] * n1, q[2] * n0 - q[0] * n2, q[0] * n1 - q[1] * n0, r]
        rows = np.where(ok[..., None], np.stack(cols, -1), dt(0)).astype(dt)
        tie = live & np.any([np.abs(x - np.rint(x)) < TIE for x in g], 0)
        gate = np.where(~live, 1, np.where(~inside, 2, np.where(~seen, 3, np.where(~near, 4, 0))))
        in_slab = inside & np.any([corner(vol["slab"], c) for c in range(8)], 0)
    aux = dict(tie=tie, gate=gate, in_slab=in_slab, q=np.stack(q, -1), g=np.stack(g, -1), cell=(ix, iy, iz), f=f, live=live)
    return ok, rows, aux


def sums29(rows, ok, dt):
    """H upper triangle | g = MINUS the sum | err | cnt, the terms formed and summed in dt (numpy's pairwise sum)."""
    x = rows.reshape(-1, 7).astype(dt)
    J, r = x[:, :6], x[:, 6]
    out = [(J[:, m] * J[:, n]).sum(dtype=dt) for m in range(6) for n in range(m, 6)]
    out += [-(J[:, m] * r).sum(dtype=dt) for m in range(6)]
    out += [(r * r).sum(dtype=dt), dt(ok.sum())]
    return np.array(out, dtype=dt)


def se3_exp_np(xi, dt):
    """geometry.se3utils.se3_exp / the device's se3_exp_dev in dt (xi = [v; omega]; the small-angle branch uses V = I + w^)."""
    xi = xi.astype(dt)
    v, w = xi[:3], xi[3:]
    Wh = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=dt)
    th = np.sqrt((w * w).sum(dtype=dt))
    I3 = np.eye(3, dtype=dt)
    if th < 1e-6:
        R = I3 + Wh
        Vm = R
    else:
        s, c, W2 = np.sin(th), np.cos(th), Wh @ Wh
        A, Bc, C = s / th, (dt(1) - c) / (th * th), (th - s) / (th * th * th)
        R, Vm = (I3 + A * Wh) + Bc * W2, (I3 + Bc * Wh) + C * W2
    T = np.eye(4, dtype=dt)
    T[:3, :3], T[:3, 3] = R, Vm @ v
    return T


def ref_step(acc, T, dt, damp=DAMP):
    """-> (T', status).  The system is solved in float64 for either dt, like the device (damping added in dt)."""
    if acc[28] < 6:
        return T, 1
    Hm = np.zeros((6, 6), dtype=dt)
    q = 0
    for m in range(6):
        for n in range(m, 6):
            Hm[m, n] = Hm[n, m] = acc[q]
            q += 1
    A = Hm.copy()
    A[np.arange(6), np.arange(6)] = np.diag(Hm) + dt(np.float32(damp))
    with np.errstate(all="ignore"):
        try:
            xi = np.linalg.solve(A.astype(np.float64), acc[21:27].astype(np.float64)).astype(dt)
        except np.linalg.LinAlgError:
            return T, 2
        if not np.isfinite(xi).all():
            return T, 2
        dT = se3_exp_np(xi, dt)
        Tn = np.eye(4, dtype=dt)
        Tn[:3, :3] = dT[:3, :3] @ T[:3, :3]
        Tn[:3, 3] = dT[:3, :3] @ T[:3, 3] + dT[:3, 3]
    return (Tn, 0) if np.isfinite(Tn).all() else (T, 2)


def ref_odometry(depth, K, P, vol, stride, levels, numiters, dt, init=None):
    """One batch element, the whole loop -> (D, info (levels, 4), D after the coarse levels, the ties of each level's last
    linearisation as {level: (q, g)} for the count comparison)."""
    D = (np.eye(4) if init is None else init).astype(dt)
    info, D_coarse, last = np.zeros((levels, 4)), None, {}
    for l in range(levels - 1, -1, -1):
        if l == 0:
            D_coarse = D.copy()
        status = 0
        for it in range(numiters[l]):
            ok, rows, aux = ref_rows(depth, K, P, D, vol, dt, stride=stride << l)
            acc = sums29(rows, ok, dt)
            D, st = ref_step(acc, D, dt)
            status |= st
            info[l] = (acc[28], acc[27], status, it + 1)
            last[l] = aux
    return D, info, D_coarse, last


def t_deviation(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return float(np.abs(A[..., :3, :3] - B[..., :3, :3]).max()), float(np.abs(A[..., :3, 3] - B[..., :3, 3]).max())


GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7))  # J's translation part (the normal), its rotation part, r


@lru_cache(maxsize=None)
def rows_reference(name, which, b):
    s = scene(name)
    return ref_rows(s["depth"][b], s["K"], s["P"][b], deltas(which)[b], volume(b), np.float64, stride=SIZES[name][2])


def rows_transcription(name, which, b):
    s = scene(name)
    return ref_rows(s["depth"][b], s["K"], s["P"][b], deltas(which)[b], volume(b), np.float32, stride=SIZES[name][2])[:2]


def compare_rows(got_ok, got_rows, name, which, b, bound=None):
    """Flags equal and rows close on every pixel not left out -> (the per-group deviations, valid pixels compared).  `bound`:
    per-group absolute bounds to assert (None: only measure)."""
    ok, rows, aux = rows_reference(name, which, b)
    out = aux["tie"]
    assert out.mean() <= 0.05, (name, which, b, float(out.mean()))
    keep = ~out
    got_ok = np.asarray(got_ok).astype(bool)
    assert np.array_equal(got_ok[keep], ok[keep]), (name, which, b, "valid flags differ on %d pixels" % int((got_ok != ok)[keep].sum()))
    d = np.abs(got_rows.astype(np.float64) - rows)[keep]
    dev = [float(d[:, g].max()) for g in GROUPS]
    if bound is not None:
        for g in range(3):
            assert dev[g] <= bound[g], (name, which, b, "group", g, dev[g], bound[g])
    return dev, int(got_ok[keep].sum())


@lru_cache(maxsize=None)
def odometry_reference(name, b, dt_name="float64"):
    s = scene(name)
    _, _, stride, levels, numiters = SIZES[name]
    return ref_odometry(s["depth"][b], s["K"], s["P"][b], volume(b), stride, levels, numiters, getattr(np, dt_name))


def init_reference(name, b, dt):
    """The level-0 iterations alone, started from the float64 reference's D after the coarse levels."""
    s = scene(name)
    _, _, stride, levels, numiters = SIZES[name]
    counts = (numiters[0],) + (0,) * (levels - 1)
    init = odometry_reference(name, b)[2].astype(np.float32)
    return ref_odometry(s["depth"][b], s["K"], s["P"][b], volume(b), stride, levels, counts, dt, init=init)[0], init


def pose_error(T, Tt):
    """(translation error in metres, rotation error in radians) of T against Tt; the angle from the skew part of R Tt^T."""
    T, Tt = np.asarray(T, dtype=np.float64), np.asarray(Tt, dtype=np.float64)
    dR = T[:3, :3] @ Tt[:3, :3].T
    w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.linalg.norm(T[:3, 3] - Tt[:3, 3])), float(np.arcsin(min(1.0, np.linalg.norm(w))))


def measure_constants():
    """What the recorded constants were measured with (python -c "import tests.test_sdf_odometry as t; print(t.measure_constants())")."""
    rows = [0.0] * 3
    for name in SIZES:
        for which in WHICH:
            for b in range(2):
                ok, r = rows_transcription(name, which, b)
                dev, _ = compare_rows(ok, r, name, which, b)
                rows = [max(x, y) for x, y in zip(rows, dev)]
    Ts = {}
    for name in SIZES:
        dev = (0.0, 0.0)
        for b in range(2):
            d1 = t_deviation(odometry_reference(name, b, "float32")[0], odometry_reference(name, b)[0])
            want = init_reference(name, b, np.float64)[0]
            d2 = t_deviation(init_reference(name, b, np.float32)[0], want)
            dev = tuple(max(x) for x in zip(dev, d1, d2))
        Ts[name] = dev
    errs = [pose_error(odometry_reference("48x64", b)[0], DELTAS[b]) for b in range(2)]
    return rows, Ts, tuple(max(e[k] for e in errs) for k in range(2))


def count_slack(last, T_bound):
    """How many pixels the allowed deviation of D itself may move across a cell face at a linearisation `last` (a ref_rows aux):
    a D that is off by (rotation entries e_R, translation entries e_t) moves q by at most 3 e_R max|pw| + e_t per axis, that is
    g by that over the voxel size; pixels whose g is nearer to an integer than that (plus the tie width) may fall in another
    cell there, and the gates of that cell may decide differently."""
    move = (3 * T_bound[0] * float(np.abs(last["q"]).max() + 0.1) + T_bound[1]) / V + TIE
    g = last["g"]
    return int((last["live"] & (np.abs(g - np.rint(g)) < move).any(-1)).sum())


# ------------------------------------------------------------------ CPU: ABI, error contracts, the references themselves
def test_sdf_symbols_are_declared_and_load():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    sigs = nv.read_signatures(header)
    lib = nv.lib()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in sigs and name in nv.SIGNATURES and hasattr(lib, name), name
        assert len(sigs[name][1]) == nargs, (name, len(sigs[name][1]))
    assert sigs["gs_sdf_odometry_ws_size"][0] is nv.c_sz and sigs["gs_sdf_odometry"][0] is nv.c_i
    assert lib.gs_abi_version() == 3
    assert all(hasattr(ops, n) for n in ("sdf_odometry", "sdf_rows_raw"))
    assert gs.odometry.SDFOdometryProvider.__module__ == "gradslam_amd.odometry.sdf"


def test_sdf_c_entry_points_refuse_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    import ctypes

    lib = nv.lib()
    P = 4096
    inf, nan = float("inf"), float("nan")
    align = lambda n: -(-n // 256) * 256
    assert lib.gs_sdf_odometry_ws_size(2, 48, 64, 1) == align(64 * 2) + align(116 * 12 * 2)
    assert lib.gs_sdf_odometry_ws_size(2, 30, 45, 2) == align(64 * 2) + align(116 * 2 * 2)  # 15 x 23 = 345 pixels: 2 rows
    assert lib.gs_sdf_odometry_ws_size(1, 480, 640, 1) == 256 + align(116 * 1200)
    for bad in ((0, 48, 64, 1), (65536, 8, 8, 1), (1, 48, 64, 0), (1, 48, 64, -2), (1, 3, 64, 1), (1, 48, 64, 17), (1, 8192, 4096, 1), (1, 0, 64, 1)):
        assert lib.gs_sdf_odometry_ws_size(*bad) == 0, bad
    counts = (ctypes.c_int * 3)(2, 1, 1)
    #     d  B  H   W   K  P  init tsdf w  nx  ny  nz  o  v     trunc minw stride L counts damp  T  info ws bytes    stream
    ok = [P, 1, 48, 64, P, P, P, P, P, 24, 20, 16, P, 0.05, 0.15, 1.0, 1, 3, counts, 1e-8, P, P, P, 1 << 24, None]
    assert len(ok) == NEW_SYMBOLS["gs_sdf_odometry"]
    for pos in (0, 4, 5, 7, 8, 12, 18, 20, 21):  # (init may be NULL: the identity)
        args = list(ok)
        args[pos] = None
        assert lib.gs_sdf_odometry(*args) == -1, pos
    for pos, bad in ((1, 0), (1, 65536), (2, 0), (3, -1), (16, 0), (16, -1), (16, 5), (17, 0), (17, 9), (17, 5), (9, 0), (10, -3), (11, 0),
                     (13, 0.0), (13, -0.05), (13, nan), (13, inf), (14, 0.0), (14, -0.1), (14, nan), (14, inf), (15, nan),
                     (19, -1e-8), (19, nan), (19, inf), (18, (ctypes.c_int * 3)(2, -1, 1)), (18, (ctypes.c_int * 3)(2, 1, (1 << 20) + 1))):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_sdf_odometry(*args) == -1, (pos, bad)
    assert b"gs_sdf_odometry" in lib.gs_last_error()
    args = list(ok)
    args[2], args[3], args[17] = 8192, 4096, 1  # 2^25 pixels
    assert lib.gs_sdf_odometry(*args) == -1 and b"2^24" in lib.gs_last_error()
    args = list(ok)
    args[9], args[10], args[11] = 1024, 1024, 1024  # 2^30 voxels
    assert lib.gs_sdf_odometry(*args) == -1 and b"2^29" in lib.gs_last_error()
    args = list(ok)
    args[23] = lib.gs_sdf_odometry_ws_size(1, 48, 64, 1) - 1
    assert lib.gs_sdf_odometry(*args) == -2
    args = list(ok)
    args[22], args[23] = None, 0
    assert lib.gs_sdf_odometry(*args) == -2

    #     d  B  H   W   K  P  D  tsdf w  nx  ny  nz  o  v     trunc minw stride valid rows sums ws bytes    stream
    ok = [P, 1, 48, 64, P, P, P, P, P, 24, 20, 16, P, 0.05, 0.15, 1.0, 1, P, P, P, P, 1 << 24, None]
    assert len(ok) == NEW_SYMBOLS["gs_sdf_rows"]
    for pos in (0, 4, 5, 6, 7, 8, 12, 17, 18, 19):
        args = list(ok)
        args[pos] = None
        assert lib.gs_sdf_rows(*args) == -1, pos
    for pos, bad in ((1, 0), (2, 0), (2, 3), (3, 3), (3, -4), (16, 0), (16, 17), (9, -1), (13, 0.0), (13, nan), (14, inf), (14, -1.0), (15, nan)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_sdf_rows(*args) == -1, (pos, bad)
    assert b"gs_sdf_rows" in lib.gs_last_error()
    args = list(ok)
    args[21] = lib.gs_sdf_odometry_ws_size(1, 48, 64, 1) - 1
    assert lib.gs_sdf_rows(*args) == -2


def cpu_frames(B=1, H=8, W=8, channels_first=False, poses=True):
    rgb, d = torch.rand(B, 1, H, W, 3), torch.rand(B, 1, H, W, 1) + 0.5
    if channels_first:
        rgb, d = rgb.permute(0, 1, 4, 2, 3).contiguous(), d.permute(0, 1, 4, 2, 3).contiguous()
    eye = torch.eye(4).view(1, 1, 4, 4).repeat(B, 1, 1, 1)
    return gs.RGBDImages(rgb, d, eye.clone(), eye.clone() if poses else None, channels_first=channels_first)


def cpu_volume(B=1, dims=(6, 5, 4)):
    """A TSDFVolume whose state sits on the host (the constructor refuses that): what the error contracts are checked with."""
    vol = object.__new__(gs.TSDFVolume)
    nx, ny, nz = dims
    vol.__dict__.update(dims=dims, voxel_size=0.1, trunc=0.3, max_weight=128.0, device=torch.device("cpu"), _B=B,
                        origin=torch.zeros(B, 3), tsdf=torch.ones(B, nz, ny, nx), weight=torch.zeros(B, nz, ny, nx), color=None)
    return vol


def test_ops_error_contracts():
    fr, vol = cpu_frames(), cpu_volume()
    d, K, P = fr.depth_image[:, 0], fr.intrinsics, fr.poses[:, 0]
    state = (vol.tsdf, vol.weight, vol.origin, vol.voxel_size, vol.trunc)
    one = dict(levels=1, numiters=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sdf_odometry(d, K, P, *state, **one)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sdf_rows_raw(d, K, P, torch.eye(4).view(1, 4, 4), *state)
    with pytest.raises(TypeError, match="depth"):
        ops.sdf_odometry(None, K, P, *state, **one)
    with pytest.raises(TypeError, match="tsdf"):
        ops.sdf_odometry(d, K, P, None, *state[1:], **one)
    with pytest.raises(TypeError, match="D to be a tensor"):
        ops.sdf_rows_raw(d, K, P, None, *state)
    with pytest.raises(ValueError, match="depth should have shape"):
        ops.sdf_odometry(d[0, 0], K, P, *state, **one)
    with pytest.raises(ValueError, match="intrinsics"):
        ops.sdf_odometry(d, K[:, :, :2], P, *state, **one)
    with pytest.raises(ValueError, match="poses"):
        ops.sdf_odometry(d, K, torch.eye(4).repeat(2, 1, 1), *state, **one)
    with pytest.raises(ValueError, match="init"):
        ops.sdf_odometry(d, K, P, *state, init=torch.eye(3).view(1, 3, 3), **one)
    with pytest.raises(ValueError, match="batch size"):
        ops.sdf_odometry(d, K, P, vol.tsdf.repeat(2, 1, 1, 1), vol.weight.repeat(2, 1, 1, 1), *state[2:], **one)
    with pytest.raises(ValueError, match="weight"):
        ops.sdf_odometry(d, K, P, vol.tsdf, vol.weight[:, :2], *state[2:], **one)
    with pytest.raises(ValueError, match="smaller than 4 x 4"):
        ops.sdf_odometry(d, K, P, *state)  # 8 x 8 has no third grid of 4 x 4
    with pytest.raises(ValueError, match="smaller than 4 x 4"):
        ops.sdf_odometry(d, K, P, *state, stride=4, **one)
    for bad in (dict(damp=-1.0), dict(damp=float("inf")), dict(numiters=(1, 2)), dict(numiters=-1), dict(numiters=(1.0,)), dict(levels=0),
                dict(levels=9), dict(levels=True), dict(stride=0), dict(stride=1.0), dict(min_weight="x")):
        with pytest.raises(ValueError):
            ops.sdf_odometry(d, K, P, *state, **{**one, **bad})
    for bad in ((vol.tsdf, vol.weight, vol.origin, 0.0, vol.trunc), (vol.tsdf, vol.weight, vol.origin, vol.voxel_size, float("inf")),
                (vol.tsdf, vol.weight, (0.0, float("nan"), 0.0), vol.voxel_size, vol.trunc)):
        with pytest.raises(ValueError):
            ops.sdf_odometry(d, K, P, *bad, **one)
    # gradients are out of scope: refused, not cut silently -- depth, poses, init and the volume's tsdf
    g = lambda t: t.clone().requires_grad_(True)
    for args, kw in (((g(d), K, P, *state), {}), ((d, K, g(P), *state), {}), ((d, K, P, g(vol.tsdf), *state[1:]), {}),
                     ((d, K, P, *state), dict(init=g(P)))):
        with pytest.raises(NotImplementedError, match="gradients"):
            ops.sdf_odometry(*args, **one, **kw)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.sdf_odometry(*args, **one, **kw)


def test_provider_error_contracts():
    Prov = gs.odometry.SDFOdometryProvider
    p = Prov()
    assert (p.numiters, p.levels, p.stride, p.min_weight, p.damp) == ((10, 5, 3), 3, 1, 1.0, 1e-8)
    assert p.last_info is None and isinstance(p, gs.odometry.OdometryProvider)
    assert Prov(4, levels=2).numiters == (4, 4)
    for bad in (dict(numiters=(1, 2)), dict(numiters=(1, 2, -1)), dict(numiters=(1, 2, 3.0)), dict(levels=0), dict(levels=2.0), dict(stride=0),
                dict(stride=2.0)):
        with pytest.raises(ValueError):
            Prov(**bad)
    fr, vol = cpu_frames(), cpu_volume()
    with pytest.raises(TypeError, match="volume to be of type gradslam.TSDFVolume"):
        p.provide(fr, fr)
    with pytest.raises(TypeError, match="source_frames to be of type gradslam.RGBDImages"):
        p.provide(vol, fr.depth_image)
    with pytest.raises(TypeError, match="init"):
        p.provide(vol, fr, init=[1.0])
    with pytest.raises(ValueError, match="Batch size"):
        p.provide(vol, cpu_frames(B=2))
    two = gs.RGBDImages(torch.rand(1, 2, 8, 8, 3), torch.rand(1, 2, 8, 8, 1), torch.eye(4).view(1, 1, 4, 4), torch.eye(4).view(1, 1, 4, 4).repeat(1, 2, 1, 1))
    with pytest.raises(ValueError, match="Sequence length"):
        p.provide(vol, two)
    with pytest.raises(ValueError, match="must have poses"):
        p.provide(vol, cpu_frames(poses=False))
    with pytest.raises(ValueError, match="init"):
        p.provide(vol, fr, init=torch.eye(4).view(1, 1, 4, 4).repeat(2, 1, 1, 1))
    with pytest.raises(ValueError, match="smaller than 4 x 4"):
        p.provide(vol, fr)  # 8 x 8 has no third grid of 4 x 4
    small = Prov(2, levels=1)
    for cf in (False, True):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            small.provide(vol, cpu_frames(channels_first=cf))
    grad_d = gs.RGBDImages(fr.rgb_image, fr.depth_image.clone().requires_grad_(True), fr.intrinsics, fr.poses)
    grad_p = gs.RGBDImages(fr.rgb_image, fr.depth_image, fr.intrinsics, fr.poses.clone().requires_grad_(True))
    grad_v = cpu_volume()
    grad_v.tsdf = grad_v.tsdf.requires_grad_(True)
    for v_, f_, kw in ((vol, grad_d, {}), (vol, grad_p, {}), (grad_v, fr, {}), (vol, fr, dict(init=fr.poses.clone().requires_grad_(True)))):
        with pytest.raises(NotImplementedError, match="gradients"):
            small.provide(v_, f_, **kw)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            small.provide(v_, f_, **kw)


def test_kinectfusion_sdf_error_contracts():
    from gradslam_amd.slam import KinectFusion

    kw = dict(dims=(8, 8, 8), voxel_size=0.1, device="cuda:0")
    slam = KinectFusion(odom="sdf", numiters=(4, 2), levels=2, damp=1e-6, dsratio=2, min_weight=2.0, color=False, **kw)
    prov = slam.odomprov
    assert isinstance(prov, gs.odometry.SDFOdometryProvider)
    assert (prov.numiters, prov.levels, prov.damp, prov.stride, prov.min_weight) == ((4, 2), 2, 1e-6, 2, 2.0)
    assert KinectFusion(odom="sdf", **kw).odomprov.numiters == (20, 20, 20)  # the driver's default count, at every level
    assert KinectFusion(odom="sdf", **kw).odomprov.stride == 4               # the driver's default dsratio
    with pytest.raises(ValueError, match="not supported.*'sdf'$"):
        KinectFusion(odom="orb", **kw)
    with pytest.raises(ValueError, match="odom_gradients"):
        KinectFusion(odom="sdf", odom_gradients=True, **kw)
    with pytest.raises(ValueError):
        KinectFusion(odom="sdf", levels=0, **kw)
    with pytest.raises(ValueError, match="dsratio"):
        KinectFusion(odom="sdf", dsratio=0, **kw)
    for odom in ("gt", "icp", "gradicp", "rgbd"):  # as before
        assert not isinstance(KinectFusion(odom=odom, **kw).odomprov, gs.odometry.SDFOdometryProvider)
    # the driver's own checks come first, then the provider's: frames on the host
    fr, vol = cpu_frames(), cpu_volume()
    with pytest.raises(ValueError, match="should have poses"):
        KinectFusion(odom="sdf", levels=1, dsratio=1, **kw).step(vol, fr, cpu_frames(poses=False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KinectFusion(odom="sdf", levels=1, dsratio=1, **kw).step(vol, fr, cpu_frames())


def test_reference_jacobian_equals_central_differences_of_its_own_residual():
    """J of the float64 reference = d r / d xi at xi = 0 of r(exp(xi) q) = trunc * trilerp(the cell's 8 values, the cell's
    coordinates of exp(xi) q), the cell held fixed: central differences with h = 1e-5 (the interpolant is a cubic in q, so the
    difference quotient is exact up to h^2 times its third derivatives)."""
    s = scene("48x64")
    b, h = 0, 1e-5
    vol = volume(b)
    ok, rows, aux = ref_rows(s["depth"][b], s["K"], s["P"][b], deltas("identity")[b], vol, np.float64)
    vs, us = np.nonzero(ok)
    pick = np.arange(0, len(vs), max(1, len(vs) // 200))
    vs, us = vs[pick], us[pick]
    assert len(vs) >= 150
    q0 = aux["q"][vs, us]
    cell = np.stack([c[vs, us] for c in aux["cell"]], -1).astype(np.float64)
    f = [x[vs, us] for x in aux["f"]]
    o, v, trunc = vol["origin"].astype(np.float64), float(np.float32(V)), float(np.float32(TRUNC))

    def residual(q):
        a = (q - o) / v - 0.5 - cell
        wx, wy, wz = ((1 - a[:, k], a[:, k]) for k in range(3))
        return trunc * sum(f[c] * wx[c & 1] * wy[(c >> 1) & 1] * wz[c >> 2] for c in range(8))

    assert np.allclose(residual(q0), rows[vs, us, 6], rtol=0, atol=1e-14)
    J = np.zeros((len(vs), 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        Ep, Em = se3_exp_np(e, np.float64), se3_exp_np(-e, np.float64)
        J[:, k] = (residual(q0 @ Ep[:3, :3].T + Ep[:3, 3]) - residual(q0 @ Em[:3, :3].T + Em[:3, 3])) / (2 * h)
    got = rows[vs, us, :6]
    scale = max(1.0, float(np.abs(J).max()))
    assert np.abs(J - got).max() <= 1e-8 * scale, np.abs(J - got).max()
    assert np.abs(got[:, :3]).max() > 0.5 and np.abs(got[:, 3:]).max() > 0.5  # the check is not vacuous: |n| is about 1


def test_scene_has_what_the_tests_need():
    """Unequal dims, every gate removes pixels, the slab is hit, at most 5 % of the pixels are left out, enough stay valid."""
    assert len(set(DIMS)) == 3
    for b in range(2):
        vol = volume(b)
        assert vol["tsdf"].shape == DIMS[::-1] and vol["slab"].sum() > 0 and (vol["weight"] == 0).sum() > vol["slab"].sum()
        assert (vol["tsdf"] == 1).any() and (vol["tsdf"] < 0).any()
    assert not np.array_equal(volume(0)["weight"], volume(1)["weight"])
    for name in SIZES:
        s = scene(name)
        assert not np.array_equal(s["depth"][0] == 0, s["depth"][1] == 0)
        gates = {1: 0, 2: 0, 3: 0, 4: 0}
        slab = 0
        for which in WHICH:
            for b in range(2):
                ok, _, aux = rows_reference(name, which, b)
                assert aux["tie"].mean() <= 0.05, (name, which, b, float(aux["tie"].mean()))
                for k in gates:
                    gates[k] += int((aux["gate"] == k).sum())
                slab += int(((aux["gate"] == 3) & aux["in_slab"]).sum())
                if which == "true" and name != "5x7":
                    assert ok.mean() >= 0.3, (name, b, float(ok.mean()))
                if which == "true":
                    assert ok.sum() >= 6, (name, b, int(ok.sum()))
        print(name, "pixels removed by gate (depth, outside, weight, free space)", gates, "of them in the slab", slab)
        assert all(n >= 1 for n in gates.values()) and slab >= 1, (name, gates, slab)


def test_float32_transcription_stays_within_its_recorded_deviation():
    """The constants the GPU bounds are built from: recomputed here from the float32 transcription, never from the device."""
    rows, Ts, recover = measure_constants()
    print("rows transcription", rows, "T transcription", Ts, "reference's error against the truth", recover)
    for g in range(3):
        assert 0.5 * ROWS_TRANSCRIPTION[g] <= rows[g] <= ROWS_TRANSCRIPTION[g], (g, rows[g])  # recorded from this, not padded
    for name in SIZES:
        for k in range(2):
            assert 0.5 * T_TRANSCRIPTION[name][k] <= Ts[name][k] <= T_TRANSCRIPTION[name][k], (name, k, Ts[name][k])
    for k in range(2):
        assert 0.5 * RECOVER_REF_ERROR[k] <= recover[k] <= RECOVER_REF_ERROR[k], (k, recover[k])
    # the reference itself recovers 1.5 voxels / 0.5 degrees to a tenth of that translation and half of that angle
    assert recover[0] < 0.15 * V and recover[1] < np.deg2rad(0.25)


# ------------------------------------------------------------------ GPU
def dev_scene(name):
    s = scene(name)
    K = torch.eye(4).repeat(2, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = s["K"]
    vols = [volume(b) for b in range(2)]
    return dict(depth=torch.from_numpy(s["depth"]).to(DEV), K=K.to(DEV), P=torch.from_numpy(s["P"]).to(DEV),
                tsdf=torch.from_numpy(np.stack([v["tsdf"] for v in vols])).to(DEV),
                weight=torch.from_numpy(np.stack([v["weight"] for v in vols])).to(DEV),
                origin=torch.from_numpy(np.stack([v["origin"] for v in vols]).astype(np.float32)).to(DEV))


def dev_T(T):
    return torch.from_numpy(np.asarray(T, dtype=np.float32)).to(DEV)


def dev_rows(name, which):
    t = dev_scene(name)
    stride = {**SIZES, **MORE_SIZES}[name][2]
    return ops.sdf_rows_raw(t["depth"], t["K"], t["P"], dev_T(deltas(which)), t["tsdf"], t["weight"], t["origin"], V, TRUNC, stride=stride)


@pytest.mark.gpu
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", list(SIZES))
def test_rows_match_the_float64_reference(name, which):
    H, W, stride = SIZES[name][:3]
    valid, rows, _ = dev_rows(name, which)
    assert tuple(valid.shape) == (2, -(-H // stride), -(-W // stride)) and tuple(rows.shape) == tuple(valid.shape) + (7,)
    valid, rows = valid.cpu().numpy(), rows.cpu().numpy()
    assert not rows[valid == 0].any()
    bound = [4 * x for x in ROWS_TRANSCRIPTION]
    for b in range(2):
        dev, n = compare_rows(valid[b], rows[b], name, which, b)
        print(name, which, "b", b, "valid compared", n, "deviation per group", dev, "bound", bound)
        compare_rows(valid[b], rows[b], name, which, b, bound=bound)
        gate = rows_reference(name, which, b)[2]["gate"]
        print(name, which, "b", b, "reference's gates (depth, outside, weight, free space)", [int((gate == k).sum()) for k in (1, 2, 3, 4)])


def chain_length(npix):
    """The longest chain of fp32 additions a term passes through: 6 butterfly steps in its wave, the block's 4 waves in order,
    its group's rows (g, g + 32, ...) in order, the 32 groups in order."""
    nblocks = -(-npix // 256)
    return 6 + 4 + -(-nblocks // 32) + 32


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES) + list(MORE_SIZES))
def test_sums_are_the_fixed_order_sums_of_the_rows_and_repeat_bitwise(name):
    H, W, stride = {**SIZES, **MORE_SIZES}[name][:3]
    valid, rows, sums = dev_rows(name, "true")
    valid2, rows2, sums2 = dev_rows(name, "true")
    assert torch.equal(sums, sums2) and torch.equal(rows, rows2) and torch.equal(valid, valid2)
    npix = -(-H // stride) * -(-W // stride)
    k = chain_length(npix)
    assert k == {"48x64": 43, "30x45": 43, "30x45s2": 43, "5x7": 43, "96x130": 44, "256x512": 58, "257x512": 59}[name]
    if name in FOLD_ROWS:  # the partial rows sit on either side of a round of reduce_partials (32 groups x 16 loads)
        nrows, rounds = FOLD_ROWS[name]
        assert -(-npix // 256) == nrows and -(-nrows // (32 * 16)) == rounds
    valid, rows, sums = valid.cpu().numpy(), rows.cpu().numpy(), sums.cpu().numpy()
    for b in range(2):
        r = rows[b].reshape(-1, 7)
        J, res = r[:, :6], r[:, 6]
        terms = [J[:, m] * J[:, n] for m in range(6) for n in range(m, 6)] + [-(J[:, m] * res) for m in range(6)] + [res * res]
        worst = 0.0
        for q, term in enumerate(terms):
            assert term.dtype == np.float32
            # (at the fold's seam: the float64 sum -- its error of at most n 2^-53 sum |term| is nothing beside the bound, and
            # the exact fp32 sum would take tens of seconds of Python at 130 thousand rows)
            exact = float(term.sum(dtype=np.float64)) if name in FOLD_ROWS else float(exact_sum_f32(term))
            bound = k * U * float(np.abs(term.astype(np.float64)).sum())
            err = abs(float(sums[b, q]) - exact)
            worst = max(worst, err / bound if bound > 0 else 0.0)
            assert err <= bound, (name, b, q, err, bound)
        in_last = int(valid[b].reshape(-1)[(-(-npix // 256) - 1) // 512 * 512 * 256:].sum())
        print(name, "b", b, "k", k, "worst error / bound", worst, "cnt", float(sums[b, 28]), "valid pixels behind the last round's rows", in_last)
        assert sums[b, 28] == float(valid[b].sum()) and sums[b, 28] >= (6 if name == "5x7" else 50)
        assert in_last >= 1  # a round left out would show in the count


def run_device(name, numiters=None, init=None, zero_depth=None):
    _, _, stride, levels, counts = SIZES[name]
    t = dev_scene(name)
    depth = t["depth"]
    if zero_depth is not None:
        depth = depth.clone()
        depth[zero_depth] = 0.0
    return ops.sdf_odometry(depth, t["K"], t["P"], t["tsdf"], t["weight"], t["origin"], V, TRUNC, init=init,
                            numiters=numiters or counts, levels=levels, stride=stride)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES))
def test_whole_call_matches_the_float64_reference(name):
    T, info = run_device(name)
    T2, info2 = run_device(name)
    assert torch.equal(T, T2) and torch.equal(info, info2)  # bit-identical from run to run
    T, info = T.cpu().numpy(), info.cpu().numpy()
    bound = [4 * x for x in T_TRANSCRIPTION[name]]
    for b in range(2):
        want, winfo, _, last = odometry_reference(name, b)
        dev = t_deviation(T[b], want)
        slack = [count_slack(last[l], bound) for l in range(len(winfo))]
        print(name, "b", b, "T deviation (rot, trans)", dev, "bound", bound, "device info", info[b].tolist(), "reference", winfo.tolist(),
              "count slack", slack, "error against the truth", pose_error(T[b], DELTAS[b]), "reference's", pose_error(want, DELTAS[b]))
        assert np.array_equal(T[b][3], [0, 0, 0, 1])
        assert np.array_equal(info[b][:, 2:], winfo[:, 2:])  # status bits and iteration counts
        # the counts: the reference's, up to the pixels the allowed deviation of D itself can move across a cell face (count_slack)
        assert (np.abs(info[b][:, 0] - winfo[:, 0]) <= np.array(slack)).all(), (name, b, info[b][:, 0], winfo[:, 0], slack)
        assert dev[0] <= bound[0] and dev[1] <= bound[1], (name, b, dev, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES))
def test_init_is_honoured_and_equals_the_levels_one_after_another(name):
    _, _, stride, levels, counts = SIZES[name]
    wants, inits = zip(*(init_reference(name, b, np.float64) for b in range(2)))
    only = lambda l: tuple(counts[k] if k == l else 0 for k in range(levels))
    T, info = run_device(name, numiters=only(0), init=dev_T(np.stack(inits)))
    Tn, info = T.cpu().numpy(), info.cpu().numpy()
    bound = [4 * x for x in T_TRANSCRIPTION[name]]
    for b in range(2):
        dev = t_deviation(Tn[b], wants[b])
        print(name, "b", b, "T deviation from the init run's reference", dev, "bound", bound)
        assert dev[0] <= bound[0] and dev[1] <= bound[1], (name, b, dev, bound)
        assert not info[b][1:].any() and info[b][0, 3] == counts[0]  # levels without iterations: zeros
    # the whole call = its levels one after another, each from the one before: the same bits (T and every level's info row)
    T_all, info_all = run_device(name)
    T_run = None
    for l in range(levels - 1, -1, -1):
        T_run, info_l = run_device(name, numiters=only(l), init=T_run)
        assert torch.equal(info_l[:, l], info_all[:, l]), (name, l)
    assert torch.equal(T_run, T_all)
    # no iterations at all: the init comes back (and the identity without one)
    T0, info0 = run_device(name, numiters=(0,) * levels, init=dev_T(np.stack(inits)))
    assert torch.equal(T0, dev_T(np.stack(inits))) and not info0.any()
    assert torch.equal(run_device(name, numiters=(0,) * levels)[0], torch.eye(4, device=DEV).repeat(2, 1, 1))


@pytest.mark.gpu
def test_a_frame_without_valid_pixels_returns_its_init_and_sets_the_status_bit():
    name = "48x64"
    init = dev_T(np.stack([make_pose(rot(0.001, 0.002, -0.001), (0.003, -0.002, 0.001))] * 2))
    T_all, info_all = run_device(name, init=init)
    T, info = run_device(name, init=init, zero_depth=1)
    assert torch.equal(T[1], init[1])
    info = info.cpu().numpy()
    assert (info[1][:, 2] == 1).all() and (info[1][:, 0] == 0).all() and np.array_equal(info[1][:, 3], SIZES[name][4])
    assert torch.equal(T[0], T_all[0]) and torch.equal(torch.from_numpy(info[0]), info_all[0].cpu())  # the other element is unaffected
    assert (info[0][:, 2] == 0).all() and not torch.equal(T[0], init[0])


@pytest.mark.gpu
@pytest.mark.parametrize("channels_first", [False, True])
def test_a_pose_off_by_one_and_a_half_voxels_and_half_a_degree_is_recovered(channels_first):
    """What it is for, through the provider.  The device's error against the ground truth is at most the float64 reference's own
    (RECOVER_REF_ERROR: the volume's discretisation) plus the distance the device may keep from that reference (four times the
    transcription's deviation): the triangle inequality, nothing measured on the device.  Measured on the MI355X: 3.42 mm, 2.47e-3 rad
    (b = 0) and 1.12 mm, 0.98e-3 rad (b = 1) from 75 mm and 8.7e-3 rad; the float64 reference: the same to 1e-7."""
    name = "48x64"
    H, W, stride, levels, counts = SIZES[name]
    t = dev_scene(name)
    frames = gs.RGBDImages(torch.zeros(2, 1, H, W, 3, device=DEV), t["depth"].view(2, 1, H, W, 1), t["K"].view(2, 1, 4, 4), t["P"].view(2, 1, 4, 4))
    if channels_first:
        frames = frames.to_channels_first()
    vol = gs.TSDFVolume(DIMS, V, origin=t["origin"], trunc=TRUNC, color=False, device=DEV)
    vol.tsdf, vol.weight = t["tsdf"], t["weight"]
    prov = gs.odometry.SDFOdometryProvider(counts, levels, stride)
    T = prov.provide(vol, frames)
    assert T.shape == (2, 1, 4, 4) and not T.requires_grad and tuple(prov.last_info.shape) == (2, levels, 4) and prov.last_info.is_cuda
    assert torch.equal(T[:, 0], run_device(name)[0])
    allow = (RECOVER_REF_ERROR[0] + 2 * 4 * T_TRANSCRIPTION[name][1], RECOVER_REF_ERROR[1] + 3 * 4 * T_TRANSCRIPTION[name][0])
    for b in range(2):
        err, start = pose_error(T[b, 0].cpu().numpy(), DELTAS[b]), pose_error(np.eye(4), DELTAS[b])
        print("b", b, "error (m, rad)", err, "allowed", allow, "the float64 reference's", RECOVER_REF_ERROR, "before", start)
        assert start[0] >= 1.49 * V and start[1] >= np.deg2rad(0.49)
        assert err[0] <= allow[0] and err[1] <= allow[1], (b, err, allow)
    # the new pose is transform . carried pose: the true camera
    from gradslam_amd.geometry.geometryutils import compose_transformations
    pose = compose_transformations(T.squeeze(1), t["P"]).cpu().numpy()
    for b in range(2):
        assert pose_error(pose[b], TRUE[b])[0] <= 2 * allow[0] + 2 * allow[1]
    # from init = the answer it stays there
    T2 = prov.provide(vol, frames, init=T)
    for b in range(2):
        err = pose_error(T2[b, 0].cpu().numpy(), DELTAS[b])
        assert err[0] <= allow[0] and err[1] <= allow[1], (b, err, allow)


KF = dict(odom="sdf", dsratio=1, numiters=(10, 5, 3), levels=3, color=False)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_kinectfusion_forward_equals_steps_equals_the_hand_composition(B):
    from gradslam_amd.geometry.geometryutils import compose_transformations
    from tests import test_kinectfusion as tk

    fr = tk.frames(B)
    slam = tk.kf(B, **KF)
    volume_f, poses = slam(fr)
    assert poses.shape == (B, tk.L, 4, 4) and torch.equal(poses[:, 0], fr.poses[:, 0]) and torch.isfinite(poses).all()
    same = lambda a, b: torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and a.color is None and b.color is None
    vol_s, prev, got = slam.new_volume(B), None, []
    for s in range(tk.L):
        live = fr[:, s]
        vol_s, p = slam.step(vol_s, live, prev)
        prev = live
        got.append(p[:, 0])
    assert torch.equal(torch.stack(got, 1), poses) and same(vol_s, volume_f)
    vol_h = gs.TSDFVolume(tk.DIMS, tk.V, origin=tk.ORIGINS[:B], trunc=tk.TRUNC, color=False, device=DEV)
    pose = fr.poses[:, :1]
    for s in range(tk.L):
        live = gs.RGBDImages(fr.rgb_image[:, s:s + 1], fr.depth_image[:, s:s + 1], fr.intrinsics, pose)
        if s > 0:
            T = slam.odomprov.provide(vol_h, live)
            pose = compose_transformations(T.squeeze(1), pose.squeeze(1)).unsqueeze(1)
            live = gs.RGBDImages(fr.rgb_image[:, s:s + 1], fr.depth_image[:, s:s + 1], fr.intrinsics, pose)
        assert torch.equal(pose[:, 0], poses[:, s]), s
        vol_h = vol_h.integrate(live)
    assert same(vol_h, volume_f)
    assert (slam.odomprov.last_info[..., 2] == 0).all() and (slam.odomprov.last_info[..., 0] > 100).all()


@pytest.mark.gpu
def test_kinectfusion_trajectory_is_as_good_as_icp_tracking_up_to_the_grid():
    """The scene and the criterion of tests/test_kinectfusion.py: ATE <= max(2 ATE of the ICP-tracked run, voxel_size), on the same
    frames.  Measured on the MI355X: ATE 0.0023, 0.0022 m with odom="sdf", 0.0047, 0.0044 m with odom="icp"."""
    from gradslam_amd.metrics import absolute_trajectory_error
    from tests import test_kinectfusion as tk

    fr = tk.frames(2)
    _, poses = tk.kf(2, **KF)(fr)
    _, icp_poses = tk.kf(2, odom="icp")(fr)
    ate, ate_icp = absolute_trajectory_error(poses, fr.poses), absolute_trajectory_error(icp_poses, fr.poses)
    print("ATE KinectFusion(sdf)", ate.tolist(), "ATE KinectFusion(icp)", ate_icp.tolist())
    assert torch.isfinite(ate).all() and (ate <= torch.clamp(2 * ate_icp, min=tk.V)).all()
    assert not torch.equal(poses[:, 1:], fr.poses[:, :-1].expand_as(poses[:, 1:]))  # it moved: not the previous pose handed on


@pytest.mark.gpu
def test_kinectfusion_sdf_refusals_and_a_camera_that_sees_nothing():
    from gradslam_amd.slam import KinectFusion
    from tests import test_kinectfusion as tk

    fr = tk.frames(2)
    # batch element 1's volume is far from everything its camera sees: nothing raises, the pose stays, the status bit is set
    slam = KinectFusion(dims=tk.DIMS, voxel_size=tk.V, origin=[tk.ORIGINS[0], (50.0, 50.0, 50.0)], trunc=tk.TRUNC, device=DEV, **KF)
    _, poses = slam(fr)
    assert torch.isfinite(poses).all()
    assert torch.equal(poses[1, 1:], fr.poses[1, :1].expand_as(poses[1, 1:]))
    info = slam.odomprov.last_info.cpu().numpy()
    assert (info[1][:, 2] == 1).all() and (info[1][:, 0] == 0).all() and (info[0][:, 2] == 0).all()
    assert not torch.equal(poses[0, 1:], fr.poses[0, :1].expand_as(poses[0, 1:]))
    # a frame without depth: the same
    empty = gs.RGBDImages(fr.rgb_image, torch.zeros_like(fr.depth_image), fr.intrinsics, fr.poses)
    one = tk.kf(2, **KF)
    vol, _ = one.step(one.new_volume(2), fr[:, 0])
    _, p = one.step(vol, empty[:, 1], fr[:, 0])
    assert torch.equal(p, fr.poses[:, :1]) and (one.odomprov.last_info[..., 2] == 1).all()
    # gradients: refused, not cut
    with pytest.raises(ValueError, match="odom_gradients"):
        tk.kf(1, **{**KF, "odom_gradients": True})
    d = fr.depth_image.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gradients"):
        tk.kf(2, **KF)(gs.RGBDImages(fr.rgb_image, d, fr.intrinsics, fr.poses))
    p = fr.poses.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gradients"):
        tk.kf(2, **KF)(gs.RGBDImages(fr.rgb_image, fr.depth_image, fr.intrinsics, p))
