"""Dense RGB-D odometry (csrc/rgbd.hip; ops.rgbd_*; gs.odometry.RGBDOdometryProvider; KinectFusion(odom="rgbd")).

The references live here, in numpy (the reference project has no counterpart): `ref_*` are the rule of include/gradslam_hip.h
vectorised over the pixels and written ONCE for a number type `dt`.  With dt = float64 they are the reference; with dt = float32
they are a transcription of the device's operations in the device's order (the library is built without contraction), which
measures what fp32 alone costs: ROWS_TRANSCRIPTION and T_TRANSCRIPTION below hold its largest deviations from float64, measured on
the CPU over every case of this file (test_float32_transcription_stays_within_its_recorded_deviation recomputes them), and the
device must agree with float64 within FOUR times those.  The sums are checked against tests.helpers.exact_sum_f32 of the products
formed in fp32 from the device's own rows.

Scene (host, float64, no files): a tilted textured plane with a textured sphere in front of it (an occlusion edge for
depth_diff_max and for the pyramid's foreground rule), depth holes (single pixels and a block), two cameras a few centimetres
and about a degree apart; B = 2 with different holes and motions.

Pixels left out of the row comparison (fp32 and float64 may decide differently there), as float64 sees them: x or y within 1e-5
of an integer, q_z within 1e-5 of 0, |r_D| within 1e-5 of the threshold; at most 5 % of the pixels.  AT THE IDENTITY every
source pixel lands on its own integer coordinates (x = u whatever the depth), so that rule would leave out every pixel: there
the x / y ties are not left out but compared against float64 evaluated in each of the (up to four) cells that meet at the
integer -- the device must agree with one of them, flag and 14 floats -- which asks more, not less.
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
from gradslam_amd.odometry import RGBDOdometryProvider
from tests.helpers import exact_sum_f32

DEV = "cuda:0"
U = 2.0 ** -24
NEW_SYMBOLS = {"gs_rgbd_odometry_ws_bytes": 4, "gs_rgbd_odometry": 20, "gs_rgbd_rows": 18, "gs_rgbd_pyramid": 10}
LAM, DDM, DAMP, SCALE = 0.968, 0.07, 1e-8, 1.0 / 255.0
TIE, CUT = 1e-5, 1e-6
# (H, W, levels, numiters finest first)
SIZES = {"48x64": (48, 64, 3, (10, 5, 3)), "30x45": (30, 45, 2, (8, 4)), "5x7": (5, 7, 1, (6,))}
# the sums alone, where the fold of the partial rows takes more than one row per group (49 blocks > 32)
MORE_SIZES = {"96x130": (96, 130, 1, (1,)),
              # the seams of reduce_partials (32 x 16 rows per round): 512 | 514 rows = one | two rounds, 1024 | 1026 = two | three.
              # (257 / 513: the last round holds the image's bottom line only, which the motion may push out of the target;
              # 288 / 544 give it 32 image lines, and there the test asserts that it holds valid pixels)
              "256x512": (256, 512, 1, (1,)), "257x512": (257, 512, 1, (1,)), "288x512": (288, 512, 1, (1,)),
              "512x512": (512, 512, 1, (1,)), "513x512": (513, 512, 1, (1,)), "544x512": (544, 512, 1, (1,))}
# partial rows (blocks of 256 pixels) and rounds of reduce_partials at those sizes.  Worst error / bound on the MI355X (b = 0, 1):
# 256x512 0.032 0.043 | 257x512 0.045 0.044 | 288x512 0.044 0.036 | 512x512 0.065 0.050 | 513x512 0.029 0.052 | 544x512 0.022 0.055
FOLD_ROWS = {"256x512": (512, 1), "257x512": (514, 2), "288x512": (576, 2), "512x512": (1024, 2), "513x512": (1026, 3), "544x512": (1088, 3)}

# The float32 transcription's largest deviation from float64 (CPU, every case of this file; recomputed and asserted below).
#   rows: per group (J_I, r_I, J_D, r_D), absolute, over the sizes, the batch elements and the three transforms
#   T:    per size (rotation entries, translation entries), absolute, after the whole loop and after the init run
ROWS_TRANSCRIPTION = (3.3e-6, 9.0e-8, 8.7e-5, 1.2e-6)
T_TRANSCRIPTION = {"48x64": (4.7e-7, 3.0e-7), "30x45": (2.6e-7, 1.3e-7), "5x7": (1.45e-2, 3.8e-3)}
# "What it is for": the float64 reference's own error against the ground truth on the facing plane (translation m, rotation rad):
# discretisation, not arithmetic.
PLANE_REF_ERROR = (8.3e-5, 8.1e-5)


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
    """(fx, fy, cx, cy) as the fp32 values the device gets."""
    return tuple(float(np.float32(k)) for k in (0.82 * W, 0.82 * W, (W - 1) / 2.0, (H - 1) / 2.0))


PLANE_P0 = np.array([0.0, 0.0, 1.6])
PLANE_N = np.array([0.25, -0.15, -1.0]) / np.linalg.norm([0.25, -0.15, -1.0])
SPHERE = (-0.16, 0.09, 1.18, 0.23)
# source camera in target-camera coordinates = the true T, per batch element
MOTIONS = [make_pose(rot(0.010, -0.014, 0.008), (0.025, -0.012, 0.015)), make_pose(rot(-0.012, 0.009, -0.015), (-0.02, 0.018, -0.01))]


def texture(p):
    """Smooth, non-periodic: sums of sinusoids of world coordinates with incommensurate frequencies, per channel, in 0..255."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    out = []
    for ph in (0.0, 1.3, 2.9):
        s = (np.sin(3.1 * x + 1.7 * y + ph) + 0.8 * np.sin(5.3 * y - 2.3 * z + 2.0 * ph) + 0.6 * np.sin(7.7 * x - 4.1 * y + 3.3 * z + 0.5)
             + 0.5 * np.sin(2.1 * (x + y) * (1.0 + 0.3 * x) + ph))
        out.append(127.5 + 127.5 * s / 2.9)
    return np.stack(out, -1)


def render(K, pose, H, W, sphere=True, plane=(PLANE_P0, PLANE_N)):
    """(depth (H,W), rgb (H,W,3)) float64 of the scene from the camera `pose` (camera-to-world)."""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)  # z-normalised: t is the camera depth
    dw, o = dc @ pose[:3, :3].T, pose[:3, 3]
    p0, n = plane
    t = (n @ (p0 - o)) / (dw @ n)
    if sphere:
        c, r = np.array(SPHERE[:3]), SPHERE[3]
        a, b, cc = (dw * dw).sum(-1), 2.0 * (dw @ (o - c)), ((o - c) ** 2).sum() - r * r
        disc = b * b - 4 * a * cc
        ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        t = np.where((ts > 0) & (ts < t), ts, t)
    return t, texture(o + t[..., None] * dw)


def punch(depth, b):
    """Holes: single pixels and a block, different per batch element (a 5 x 7 image: one pixel and a 1 x 2 block -- a hole in
    the target takes the four cells around it with it)."""
    H, W = depth.shape
    d = depth.copy()
    singles = ((0.25, 0.3), (0.6, 0.7), (0.8, 0.15)) if b == 0 else ((0.35, 0.55), (0.7, 0.2), (0.15, 0.85))
    for (fv, fu) in singles[: 3 if H >= 16 else 1]:
        d[int(fv * H), int(fu * W)] = 0.0
    v0, u0 = (int(0.5 * H), int(0.12 * W)) if b == 0 else (int(0.1 * H), int(0.6 * W))
    d[v0:v0 + (max(2, H // 8) if H >= 16 else 1), u0:u0 + max(2, W // 8)] = 0.0
    return d


@lru_cache(maxsize=None)
def scene(name):
    """Both frames of both batch elements as the fp32 arrays the device gets: depth (B,H,W), rgb (B,H,W,3); K; true T (B,4,4)."""
    H, W = {**SIZES, **MORE_SIZES}[name][:2]
    K = make_K(H, W)
    out = {k: [] for k in ("td", "tc", "sd", "sc")}
    for b in range(2):
        td, tc = render(K, np.eye(4), H, W)
        sd, sc = render(K, MOTIONS[b], H, W)
        out["td"].append(punch(td, 1 - b))
        out["sd"].append(punch(sd, b))
        out["tc"].append(tc)
        out["sc"].append(sc)
    out = {k: np.stack(v).astype(np.float32) for k, v in out.items()}
    out.update(K=K, T=np.stack(MOTIONS), H=H, W=W)
    return out


def in_plane_shift(T, frac, K, W):
    """translate(t) . T with t in the plane (so the warped points stay on it) and long enough to move the image by frac * W."""
    t = np.cross(PLANE_N, [0.0, 1.0, 0.0])
    t = t / np.linalg.norm(t) * (frac * W * PLANE_P0[2] / K[0])
    return make_pose(np.eye(3), t) @ T


def transforms(name):
    """The three (B,4,4) sets the rows are checked at: the true T, the identity, a fifth of the pixels pushed outside."""
    s = scene(name)
    return {"true": s["T"], "identity": np.stack([np.eye(4)] * 2),
            "outside": np.stack([in_plane_shift(s["T"][0], 0.25, s["K"], s["W"]), in_plane_shift(s["T"][1], -0.125, s["K"], s["W"])])}


# ------------------------------------------------------------------ the rule, once, for a number type dt
def ref_level0(depth, rgb, dt, scale=SCALE):
    c = [dt(np.float32(x)) for x in (0.299, 0.587, 0.114)]
    rgb, d = rgb.astype(dt), depth.astype(dt)
    I = dt(np.float32(scale)) * ((c[0] * rgb[..., 0] + c[1] * rgb[..., 1]) + c[2] * rgb[..., 2])
    return I, np.where((d > 0) & np.isfinite(d), d, dt(0))


def ref_down(I, D, dt, ddm=DDM):
    """(H, W) -> (H // 2, W // 2); also the blocks in which a valid depth lies within CUT of the cut (float64's view)."""
    H2, W2 = I.shape[0] // 2, I.shape[1] // 2
    blk = lambda A: [A[0:2 * H2:2, 0:2 * W2:2], A[0:2 * H2:2, 1:2 * W2:2], A[1:2 * H2:2, 0:2 * W2:2], A[1:2 * H2:2, 1:2 * W2:2]]
    i, d = blk(I), blk(D)
    Io = (((i[0] + i[1]) + i[2]) + i[3]) * dt(0.25)
    dmin = np.full((H2, W2), np.inf, dtype=dt)
    for k in range(4):
        dmin = np.where((d[k] > 0) & (d[k] < dmin), d[k], dmin)
    s, n, near = np.zeros((H2, W2), dtype=dt), np.zeros((H2, W2), dtype=np.int64), np.zeros((H2, W2), dtype=bool)
    cut = dt(np.float32(ddm))
    with np.errstate(invalid="ignore"):
        for k in range(4):
            take = (d[k] > 0) & (d[k] - dmin <= cut)
            s = np.where(take, s + d[k], s)
            n += take
            near |= (d[k] > 0) & (np.abs((d[k] - dmin) - cut) < CUT)
        Do = np.where(n > 0, s / np.maximum(n, 1).astype(dt), dt(0))
    return Io, Do, near


def ref_pyramid(depth, rgb, levels, dt):
    """[(I, D)] per level, and the per-level masks of blocks near the cut."""
    pyr, nears = [ref_level0(depth, rgb, dt)], [None]
    for _ in range(1, levels):
        I, D, near = ref_down(pyr[-1][0], pyr[-1][1], dt)
        pyr.append((I, D))
        nears.append(near)
    return pyr, nears


def level_K(K, level, dt):
    fx, fy, cx, cy = (dt(k) for k in K)
    for _ in range(level):
        fx, fy = fx * dt(0.5), fy * dt(0.5)
        cx, cy = (cx + dt(0.5)) * dt(0.5) - dt(0.5), (cy + dt(0.5)) * dt(0.5) - dt(0.5)
    return fx, fy, cx, cy


def ref_rows(tI, tD, sI, sD, K, T, dt, lam=LAM, ddm=DDM, cell=None):
    """One linearisation of one batch element at one level: (valid (H,W), rows (H,W,14), aux).  K: the level's (fx, fy, cx, cy) in dt.
    cell = (sx, sy): pixels whose x (y) lies within TIE of an integer take the cell round(x) - sx (round(y) - sy)."""
    H, W = sD.shape
    fx, fy, cx, cy = K
    T = T.astype(dt)
    v, u = np.meshgrid(np.arange(H).astype(dt), np.arange(W).astype(dt), indexing="ij")
    one = dt(1)
    with np.errstate(all="ignore"):
        d = sD.astype(dt)
        ok = d > 0
        px, py = d * ((u - cx) / fx), d * ((v - cy) / fy)
        qx, qy, qz = (((T[i, 0] * px + T[i, 1] * py) + T[i, 2] * d) + T[i, 3] for i in range(3))
        ok = ok & (qz > 0)
        iz = one / qz
        x, y = (fx * qx) * iz + cx, (fy * qy) * iz + cy
        xf, yf = np.floor(x), np.floor(y)
        tie_x, tie_y = np.abs(x - np.rint(x)) < TIE, np.abs(y - np.rint(y)) < TIE
        if cell is not None:
            xf, yf = np.where(tie_x, np.rint(x) - cell[0], xf), np.where(tie_y, np.rint(y) - cell[1], yf)
        ok = ok & (xf >= 0) & (xf <= W - 2) & (yf >= 0) & (yf <= H - 2)
        i, j = np.where(ok, xf, 0).astype(np.int64), np.where(ok, yf, 0).astype(np.int64)
        a, b = x - xf, y - yf
        tI, tD = tI.astype(dt), tD.astype(dt)
        I00, I10, I01, I11 = tI[j, i], tI[j, i + 1], tI[j + 1, i], tI[j + 1, i + 1]
        D00, D10, D01, D11 = tD[j, i], tD[j, i + 1], tD[j + 1, i], tD[j + 1, i + 1]
        ok = ok & (D00 > 0) & (D10 > 0) & (D01 > 0) & (D11 > 0)

        def sample(F00, F10, F01, F11):
            X0, X1 = F10 - F00, F11 - F01
            top, bot = F00 + a * X0, F01 + a * X1
            return top + b * (bot - top), X0 + b * (X1 - X0), bot - top

        Ih, Ix, Iy = sample(I00, I10, I01, I11)
        Dh, Dx, Dy = sample(D00, D10, D01, D11)
        ri, rd = Ih - sI.astype(dt), Dh - qz
        cut = dt(np.float32(ddm))
        pre = ok
        ok = ok & (np.abs(rd) <= cut)
        lam32 = dt(np.float32(lam))
        wI, wD = np.sqrt(one - lam32), np.sqrt(lam32)
        gx, gy = fx * iz, fy * iz
        i0, i1 = Ix * gx, Iy * gy
        i2 = -((i0 * qx + i1 * qy) * iz)
        d0, d1 = Dx * gx, Dy * gy
        d2 = -((d0 * qx + d1 * qy) * iz) - one
        cols = [wI * i0, wI * i1, wI * i2, wI * (qy * i2 - qz * i1), wI * (qz * i0 - qx * i2), wI * (qx * i1 - qy * i0), wI * ri,
                wD * d0, wD * d1, wD * d2, wD * (qy * d2 - qz * d1), wD * (qz * d0 - qx * d2), wD * (qx * d1 - qy * d0), wD * rd]
        rows = np.where(ok[..., None], np.stack(cols, -1), dt(0)).astype(dt)
        live = (sD > 0)
        aux = dict(tie_xy=live & (qz > 0) & (tie_x | tie_y), tie_q=live & (np.abs(qz) < TIE),
                   tie_r=pre & (np.abs(np.abs(rd) - cut) < TIE), x=x, y=y, qz=qz, i=i, j=j, a=a, b=b, pre=pre)
    return ok, rows, aux


def sums29(rows, ok, dt):
    """H upper triangle | g = MINUS the sum | err | cnt, the terms formed and summed in dt (numpy's pairwise sum)."""
    r = rows.reshape(-1, 14).astype(dt)
    JI, rI, JD, rD = r[:, :6], r[:, 6], r[:, 7:13], r[:, 13]
    out = []
    for m in range(6):
        for n in range(m, 6):
            out.append((JI[:, m] * JI[:, n] + JD[:, m] * JD[:, n]).sum(dtype=dt))
    for m in range(6):
        out.append(-(JI[:, m] * rI + JD[:, m] * rD).sum(dtype=dt))
    out.append((rI * rI + rD * rD).sum(dtype=dt))
    out.append(dt(ok.sum()))
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
        V = R
    else:
        s, c, W2 = np.sin(th), np.cos(th), Wh @ Wh
        A, Bc, C = s / th, (dt(1) - c) / (th * th), (th - s) / (th * th * th)
        R, V = (I3 + A * Wh) + Bc * W2, (I3 + Bc * Wh) + C * W2
    T = np.eye(4, dtype=dt)
    T[:3, :3], T[:3, 3] = R, V @ v
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


def ref_odometry(td, tc, sd, sc, K, levels, numiters, dt, init=None):
    """One batch element, the whole loop -> (T, info (levels, 4), T after the coarse levels)."""
    tp, _ = ref_pyramid(td, tc, levels, dt)
    sp, _ = ref_pyramid(sd, sc, levels, dt)
    T = (np.eye(4) if init is None else init).astype(dt)
    info, T_coarse = np.zeros((levels, 4)), None
    for l in range(levels - 1, -1, -1):
        if l == 0:
            T_coarse = T.copy()
        Kl, status = level_K(K, l, dt), 0
        for it in range(numiters[l]):
            ok, rows, _ = ref_rows(tp[l][0], tp[l][1], sp[l][0], sp[l][1], Kl, T, dt)
            acc = sums29(rows, ok, dt)
            T, st = ref_step(acc, T, dt)
            status |= st
            info[l] = (acc[28], acc[27], status, it + 1)
    return T, info, T_coarse


def left_out(aux):
    return aux["tie_xy"] | aux["tie_q"] | aux["tie_r"]


def t_deviation(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return float(np.abs(A[..., :3, :3] - B[..., :3, :3]).max()), float(np.abs(A[..., :3, 3] - B[..., :3, 3]).max())


GROUPS = (slice(0, 6), slice(6, 7), slice(7, 13), slice(13, 14))  # J_I, r_I, J_D, r_D


def group_dev(a, b, mask):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))[mask]
    return [float(d[:, g].max()) if d.size else 0.0 for g in GROUPS]


@lru_cache(maxsize=None)
def rows_reference(name, which, b):
    """float64 rows of batch element b at level 0 (and, at the identity, in each of the four cells)."""
    s = scene(name)
    T = transforms(name)[which][b]
    tI, tD = ref_level0(s["td"][b], s["tc"][b], np.float64)
    sI, sD = ref_level0(s["sd"][b], s["sc"][b], np.float64)
    K = level_K(s["K"], 0, np.float64)
    cells = [None] if which != "identity" else [(sx, sy) for sx in (0, 1) for sy in (0, 1)]
    return [ref_rows(tI, tD, sI, sD, K, T, np.float64, cell=c) for c in cells]


def rows_transcription(name, which, b):
    s = scene(name)
    T = transforms(name)[which][b].astype(np.float32)
    tI, tD = ref_level0(s["td"][b], s["tc"][b], np.float32)
    sI, sD = ref_level0(s["sd"][b], s["sc"][b], np.float32)
    return ref_rows(tI, tD, sI, sD, level_K(s["K"], 0, np.float32), T, np.float32)[:2]


def compare_rows(got_ok, got_rows, name, which, b, bound=None):
    """Flags equal and rows close on every pixel not left out -> the per-group deviations.  At the identity a pixel passes if
    it agrees with one of the cells.  `bound`: per-group absolute bounds to assert (None: only measure)."""
    refs = rows_reference(name, which, b)
    aux = refs[0][2]
    out = aux["tie_q"] | aux["tie_r"] if which == "identity" else left_out(aux)
    for r in refs[1:]:
        out = out | r[2]["tie_q"] | r[2]["tie_r"]
    assert out.mean() <= 0.05, (name, which, b, float(out.mean()))
    keep = ~out
    got_ok = np.asarray(got_ok).astype(bool)
    best = np.full(got_ok.shape + (4,), np.inf)
    flags = np.zeros(got_ok.shape, dtype=bool)
    for ok, rows, _ in refs:
        same = ok == got_ok
        d = np.abs(got_rows.astype(np.float64) - rows)
        dev = np.stack([d[..., g].max(-1) for g in GROUPS], -1)
        better = same & (dev.max(-1) < best.max(-1))
        best = np.where(better[..., None], dev, best)
        flags |= same
    assert flags[keep].all(), (name, which, b, "valid flags differ on %d pixels" % int((~flags[keep]).sum()))
    dev = [float(best[..., g][keep].max()) for g in range(4)]
    if bound is not None:
        for g in range(4):
            assert dev[g] <= bound[g], (name, which, b, "group", g, dev[g], bound[g])
    return dev, int(got_ok[keep].sum())


@lru_cache(maxsize=None)
def odometry_reference(name, b, dt_name="float64"):
    s = scene(name)
    _, _, levels, numiters = SIZES[name]
    return ref_odometry(s["td"][b], s["tc"][b], s["sd"][b], s["sc"][b], s["K"], levels, numiters, getattr(np, dt_name))


def init_reference(name, b, dt):
    """The level-0 iterations alone, started from the float64 reference's T after the coarse levels."""
    s = scene(name)
    _, _, levels, numiters = SIZES[name]
    counts = (numiters[0],) + (0,) * (levels - 1)
    init = odometry_reference(name, b)[2]
    return ref_odometry(s["td"][b], s["tc"][b], s["sd"][b], s["sc"][b], s["K"], levels, counts, dt, init=init.astype(np.float32))[0], init


# the facing plane: what the colour is for
PLANE = (np.array([0.0, 0.0, 1.5]), np.array([0.0, 0.0, -1.0]))
PLANE_T = make_pose(rot(0.0, 0.0, np.deg2rad(0.5)), (0.016, 0.012, 0.0))  # ~2 cm in the plane, 0.5 degrees about the normal


@lru_cache(maxsize=None)
def plane_scene():
    H, W = 48, 64
    K = make_K(H, W)
    td, tc = render(K, np.eye(4), H, W, sphere=False, plane=PLANE)
    sd, sc = render(K, PLANE_T, H, W, sphere=False, plane=PLANE)
    return dict(td=td.astype(np.float32), tc=tc.astype(np.float32), sd=sd.astype(np.float32), sc=sc.astype(np.float32), K=K, H=H, W=W)


def pose_error(T, Tt):
    """(translation error in metres, rotation error in radians) of T against Tt.  The angle from the skew part of R Tt^T (its
    sine): well conditioned at small angles, where the arc cosine of the trace turns an fp32 matrix's 1e-7 into 4e-4."""
    T, Tt = np.asarray(T, dtype=np.float64), np.asarray(Tt, dtype=np.float64)
    dR = T[:3, :3] @ Tt[:3, :3].T
    w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.linalg.norm(T[:3, 3] - Tt[:3, 3])), float(np.arcsin(min(1.0, np.linalg.norm(w))))


def measure_constants():
    """What the recorded constants were measured with (python -c "import tests.test_rgbd_odometry as t; print(t.measure_constants())")."""
    rows = [0.0] * 4
    for name in SIZES:
        for which in ("true", "identity", "outside"):
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
    p = plane_scene()
    T = ref_odometry(p["td"], p["tc"], p["sd"], p["sc"], p["K"], 3, (10, 5, 3), np.float64)[0]
    return rows, Ts, pose_error(T, PLANE_T)


# ------------------------------------------------------------------ CPU: ABI, error contracts, the references themselves
def test_rgbd_symbols_load_and_are_declared():
    lib = nv.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
        assert name + "(" in header, name
        decl = header[header.index(name + "("):]
        assert decl[: decl.index(";")].count(",") + 1 == nargs, name
    assert lib.gs_abi_version() == 3
    assert all(hasattr(ops, n) for n in ("rgbd_odometry", "rgbd_rows_raw", "rgbd_pyramid_raw"))
    assert gs.odometry.RGBDOdometryProvider.__module__ == "gradslam_amd.odometry.rgbd"


def test_rgbd_c_entry_points_refuse_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    import ctypes

    lib = nv.lib()
    P = 4096
    inf, nan = float("inf"), float("nan")
    align = lambda n: -(-n // 256) * 256
    pix = 48 * 64 + 24 * 32 + 12 * 16
    assert lib.gs_rgbd_odometry_ws_bytes(2, 48, 64, 3) == align(64 * 2) + align(116 * 12 * 2) + 2 * align(8 * pix * 2)
    for bad in ((0, 48, 64, 3), (1, 48, 64, 0), (1, 48, 64, 5), (1, 48, 64, 9), (1, 3, 64, 1), (1, 5, 7, 2), (1, 8192, 4096, 1), (65536, 8, 8, 1)):
        assert lib.gs_rgbd_odometry_ws_bytes(*bad) == 0, bad
    counts = (ctypes.c_int * 3)(2, 1, 1)
    #     td tc sd sc B  H   W   K  init L  counts  lam  ddm   damp  scale T  info ws  bytes    stream
    ok = [P, P, P, P, 1, 48, 64, P, P, 3, counts, 0.9, 0.07, 1e-8, 1.0, P, P, P, 1 << 24, None]
    for pos in (0, 1, 2, 3, 7, 10, 15, 16):  # (init may be NULL: the identity)
        args = list(ok)
        args[pos] = None
        assert lib.gs_rgbd_odometry(*args) == -1, pos
    for pos, bad in ((4, 0), (4, 65536), (5, 0), (6, -1), (5, 15), (6, 15), (9, 0), (9, 9), (9, 5), (11, -0.01), (11, 1.01), (11, nan), (11, inf),
                     (12, 0.0), (12, -0.07), (12, nan), (12, inf), (13, -1e-8), (13, nan), (13, inf), (14, nan), (14, inf),
                     (10, (ctypes.c_int * 3)(2, -1, 1)), (10, (ctypes.c_int * 3)(2, 1, -5))):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_rgbd_odometry(*args) == -1, (pos, bad)
    assert b"gs_rgbd_odometry" in lib.gs_last_error()
    args = list(ok)
    args[5], args[6], args[9] = 8192, 4096, 1  # 2^25 pixels
    assert lib.gs_rgbd_odometry(*args) == -1 and b"2^24" in lib.gs_last_error()
    args = list(ok)
    args[18] = lib.gs_rgbd_odometry_ws_bytes(1, 48, 64, 3) - 1
    assert lib.gs_rgbd_odometry(*args) == -2
    args = list(ok)
    args[17], args[18] = None, 0
    assert lib.gs_rgbd_odometry(*args) == -2

    #     td tc sd sc B  H   W   K  T  lam  ddm   scale valid rows sums ws bytes    stream
    ok = [P, P, P, P, 1, 48, 64, P, P, 0.9, 0.07, 1.0, P, P, P, P, 1 << 24, None]
    for pos in (0, 1, 2, 3, 7, 8, 12, 13, 14):
        args = list(ok)
        args[pos] = None
        assert lib.gs_rgbd_rows(*args) == -1, pos
    for pos, bad in ((4, 0), (5, 0), (5, 3), (6, 3), (6, -4), (9, -0.5), (9, 2.0), (9, nan), (10, 0.0), (10, nan), (10, inf), (11, nan)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_rgbd_rows(*args) == -1, (pos, bad)
    assert b"gs_rgbd_rows" in lib.gs_last_error()
    args = list(ok)
    args[16] = lib.gs_rgbd_odometry_ws_bytes(1, 48, 64, 1) - 1
    assert lib.gs_rgbd_rows(*args) == -2

    #     d  rgb B  H   W   L  ddm   scale out stream
    ok = [P, P, 1, 48, 64, 3, 0.07, 1.0, P, None]
    for pos in (0, 1, 8):
        args = list(ok)
        args[pos] = None
        assert lib.gs_rgbd_pyramid(*args) == -1, pos
    for pos, bad in ((2, 0), (3, 0), (4, -1), (5, 0), (5, 5), (5, 9), (6, 0.0), (6, -1.0), (6, nan), (6, inf), (7, nan), (7, inf)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_rgbd_pyramid(*args) == -1, (pos, bad)
    assert b"gs_rgbd_pyramid" in lib.gs_last_error()


def cpu_frames(B=1, H=8, W=8, channels_first=False, **kw):
    rgb, d = torch.rand(B, 1, H, W, 3), torch.rand(B, 1, H, W, 1) + 0.5
    if channels_first:
        rgb, d = rgb.permute(0, 1, 4, 2, 3).contiguous(), d.permute(0, 1, 4, 2, 3).contiguous()
    return gs.RGBDImages(rgb, d, torch.eye(4).view(1, 1, 4, 4).repeat(B, 1, 1, 1), channels_first=channels_first, **kw)


def test_provider_error_contracts():
    Prov = RGBDOdometryProvider
    assert gs.odometry.RGBDOdometryProvider is Prov
    p = Prov()
    assert (p.numiters, p.levels, p.lambda_geo, p.depth_diff_max, p.damp, p.rgb_scale) == ((10, 5, 3), 3, 0.968, 0.07, 1e-8, 1 / 255)
    assert p.last_info is None and isinstance(p, gs.odometry.OdometryProvider)
    assert Prov(4, levels=2).numiters == (4, 4)
    for bad in (dict(numiters=(1, 2)), dict(numiters=(1, 2, -1)), dict(numiters=(1, 2, 3.0)), dict(levels=0), dict(levels=2.0)):
        with pytest.raises(ValueError):
            Prov(**bad)
    fr = cpu_frames()
    with pytest.raises(TypeError, match="target_frames to be of type gradslam.RGBDImages"):
        p.provide(fr.depth_image, fr)
    with pytest.raises(TypeError, match="source_frames to be of type gradslam.RGBDImages"):
        p.provide(fr, None)
    with pytest.raises(TypeError, match="init"):
        p.provide(fr, fr, init=[1.0])
    with pytest.raises(ValueError, match="Batch size"):
        p.provide(fr, cpu_frames(B=2))
    two = gs.RGBDImages(torch.rand(1, 2, 8, 8, 3), torch.rand(1, 2, 8, 8, 1), torch.eye(4).view(1, 1, 4, 4))
    with pytest.raises(ValueError, match="Sequence length"):
        p.provide(fr, two)
    with pytest.raises(ValueError, match="Image size"):
        p.provide(fr, cpu_frames(H=16))
    with pytest.raises(ValueError, match="init"):
        p.provide(fr, fr, init=torch.eye(4).view(1, 1, 4, 4).repeat(2, 1, 1, 1))
    other_K = gs.RGBDImages(fr.rgb_image, fr.depth_image, 2 * fr.intrinsics)
    with pytest.raises(ValueError, match="Intrinsics"):
        p.provide(fr, other_K)
    with pytest.raises(ValueError, match="smaller than 4 x 4"):
        p.provide(fr, fr)  # 8 x 8 has no third level of 4 x 4
    small = Prov(2, levels=1)
    for cf in (False, True):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            small.provide(cpu_frames(channels_first=cf), cpu_frames(channels_first=cf))
    # gradients are out of scope: refused, not cut silently
    grad = gs.RGBDImages(fr.rgb_image, fr.depth_image.clone().requires_grad_(True), fr.intrinsics)
    with pytest.raises(NotImplementedError, match="gradients"):
        small.provide(fr, grad)
    with pytest.raises(NotImplementedError, match="gradients"):
        small.provide(grad, fr)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        small.provide(fr, grad)
    d, c, K = fr.depth_image[:, 0], fr.rgb_image[:, 0], fr.intrinsics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgbd_odometry(d, c, d, c, K, levels=1, numiters=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgbd_rows_raw(d, c, d, c, K, torch.eye(4).view(1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgbd_pyramid_raw(d, c, 1)
    for bad in (dict(lambda_geo=1.5), dict(depth_diff_max=0.0), dict(damp=-1.0), dict(numiters=(1, 2)), dict(rgb_scale=float("inf"))):
        with pytest.raises(ValueError):
            ops.rgbd_odometry(d, c, d, c, K, **{**dict(levels=1, numiters=1), **bad})
    with pytest.raises(ValueError, match="same batch size and image size"):
        ops.rgbd_odometry(d, c, d[:, :4], c[:, :4], K, levels=1, numiters=1)


def test_kinectfusion_rgbd_error_contracts():
    from gradslam_amd.slam import KinectFusion

    kw = dict(dims=(8, 8, 8), voxel_size=0.1, device="cuda:0")
    slam = KinectFusion(odom="rgbd", numiters=(4, 2), levels=2, lambda_geo=0.9, damp=1e-6, **kw)
    prov = slam.odomprov
    assert isinstance(prov, gs.odometry.RGBDOdometryProvider)
    assert (prov.numiters, prov.levels, prov.lambda_geo, prov.damp) == ((4, 2), 2, 0.9, 1e-6)
    assert KinectFusion(odom="rgbd", **kw).odomprov.numiters == (20, 20, 20)  # the driver's default count, at every level
    with pytest.raises(ValueError, match="color=True"):
        KinectFusion(odom="rgbd", color=False, **kw)
    with pytest.raises(ValueError, match="not supported.*'rgbd'"):
        KinectFusion(odom="orb", **kw)
    with pytest.raises(ValueError):
        KinectFusion(odom="rgbd", levels=0, **kw)
    for odom in ("gt", "icp", "gradicp"):  # as before: the new arguments are not theirs
        other = KinectFusion(odom=odom, **kw)
        assert not isinstance(other.odomprov, gs.odometry.RGBDOdometryProvider)


def test_reference_jacobians_equal_float64_autograd_of_its_own_residuals():
    """J_I, J_D of the float64 reference = d r_I / d xi, d r_D / d xi at xi = 0 by torch autograd of the reference's residuals
    (q = exp(xi) q0, projection, the bilinear interpolants in the cell the reference chose), the decisions held constant."""
    s = scene("48x64")
    b = 0
    tI, tD = ref_level0(s["td"][b], s["tc"][b], np.float64)
    sI, sD = ref_level0(s["sd"][b], s["sc"][b], np.float64)
    K = level_K(s["K"], 0, np.float64)
    T = s["T"][b]
    ok, rows, aux = ref_rows(tI, tD, sI, sD, K, T, np.float64)
    vs, us = np.nonzero(ok)
    pick = np.arange(0, len(vs), max(1, len(vs) // 150))
    vs, us = vs[pick], us[pick]
    assert len(vs) >= 100
    fx, fy, cx, cy = K
    d = sD[vs, us]
    p0 = np.stack([d * ((us - cx) / fx), d * ((vs - cy) / fy), d], -1)
    q0 = torch.from_numpy(p0 @ T[:3, :3].T + T[:3, 3])
    i, j = aux["i"][vs, us], aux["j"][vs, us]
    cI = [torch.from_numpy(tI[j + dj, i + di]) for dj, di in ((0, 0), (0, 1), (1, 0), (1, 1))]  # 00, 10, 01, 11 (x offset first)
    cD = [torch.from_numpy(tD[j + dj, i + di]) for dj, di in ((0, 0), (0, 1), (1, 0), (1, 1))]
    Is = torch.from_numpy(sI[vs, us])
    wI, wD = np.sqrt(1 - float(np.float32(LAM))), np.sqrt(float(np.float32(LAM)))

    def residuals(xi):
        E = se3utils.se3_exp(xi)
        q = q0 @ E[:3, :3].T + E[:3, 3]
        a = fx * q[:, 0] / q[:, 2] + cx - torch.from_numpy(i.astype(np.float64))
        bb = fy * q[:, 1] / q[:, 2] + cy - torch.from_numpy(j.astype(np.float64))
        bil = lambda c: (1 - bb) * ((1 - a) * c[0] + a * c[1]) + bb * ((1 - a) * c[2] + a * c[3])
        return torch.cat([wI * (bil(cI) - Is), wD * (bil(cD) - q[:, 2])])

    xi0 = torch.zeros(6, dtype=torch.float64)
    r = residuals(xi0).numpy()
    J = torch.autograd.functional.jacobian(residuals, xi0).numpy()
    n = len(vs)
    got = rows[vs, us]
    assert np.allclose(r[:n], got[:, 6], rtol=0, atol=1e-12) and np.allclose(r[n:], got[:, 13], rtol=0, atol=1e-12)
    scale = max(1.0, float(np.abs(J).max()))
    assert np.abs(J[:n] - got[:, :6]).max() <= 1e-10 * scale and np.abs(J[n:] - got[:, 7:13]).max() <= 1e-10 * scale
    assert np.abs(J[:n]).max() > 1e-3 and np.abs(J[n:, 3:]).max() > 1e-1  # the check is not vacuous


def test_pyramid_reference_on_a_hand_written_example():
    """4 x 4 with a hole and a depth step: the mean of the valid depths within depth_diff_max of the block's smallest."""
    D = np.array([[1.0, 1.02, 2.0, 2.0],
                  [1.0, 0.0, 1.0, 2.0],
                  [0.0, 0.0, 3.0, 3.05],
                  [0.0, 0.0, 3.2, 0.0]])
    I = np.arange(16, dtype=np.float64).reshape(4, 4)
    Io, Do, near = ref_down(I, D, np.float64)
    assert np.array_equal(Io, [[2.5, 4.5], [10.5, 12.5]])
    assert np.allclose(Do, [[3.02 / 3, 1.0], [0.0, 6.05 / 2]], rtol=1e-15, atol=0) and not near.any()
    # foreground and background are never averaged: 1.0 and 2.0 in one block give 1.0; 3.2 is beyond 3.0 + 0.07
    K1 = level_K((100.0, 100.0, 31.5, 23.5), 1, np.float64)
    assert K1 == (50.0, 50.0, 15.5, 11.5)
    pyr, _ = ref_pyramid(np.ones((5, 7)), np.full((5, 7, 3), 255.0), 2, np.float64)
    assert pyr[1][0].shape == (2, 3) and np.allclose(pyr[0][0], 1.0, atol=1e-6)  # odd sizes: the floor; luma weights sum to 1


def test_scene_has_what_the_tests_need():
    """An occlusion edge, holes, an outside fifth, and no pyramid block near the cut (so fp32 and float64 agree on validity)."""
    for name, (H, W, levels, _) in SIZES.items():
        s = scene(name)
        for b in range(2):
            assert (s["td"][b] == 0).sum() >= 3 and (s["sd"][b] == 0).sum() >= 3
            assert not np.array_equal(s["td"][0] == 0, s["td"][1] == 0)
            for d, c in ((s["td"][b], s["tc"][b]), (s["sd"][b], s["sc"][b])):
                assert c.min() >= 0 and c.max() <= 255
                _, nears = ref_pyramid(d, c, levels, np.float64)
                assert not any(n.any() for n in nears[1:]), (name, b)
        if name == "48x64":
            step = np.abs(np.diff(s["sd"][0], axis=1))
            assert (step > DDM).sum() >= 10  # the sphere's rim
            for b in range(2):
                aux = rows_reference(name, "outside", b)[0][2]
                x, y, live = aux["x"], aux["y"], s["sd"][b] > 0
                outside = live & ((x < 0) | (x > W - 1) | (y < 0) | (y > H - 1))
                assert 0.15 <= outside.sum() / live.sum() <= 0.25, outside.sum() / live.sum()  # a fifth


def test_float32_transcription_stays_within_its_recorded_deviation():
    """The constants the GPU bounds are built from: recomputed here from the float32 transcription, never from the device."""
    rows, Ts, plane = measure_constants()
    print("rows transcription", rows, "T transcription", Ts, "plane reference error", plane)
    for g in range(4):
        assert rows[g] <= ROWS_TRANSCRIPTION[g], (g, rows[g])
        assert rows[g] >= 0.5 * ROWS_TRANSCRIPTION[g], (g, rows[g])  # recorded from this, not padded
    for name in SIZES:
        for k in range(2):
            assert 0.5 * T_TRANSCRIPTION[name][k] <= Ts[name][k] <= T_TRANSCRIPTION[name][k], (name, k, Ts[name][k])
    for k in range(2):
        assert 0.5 * PLANE_REF_ERROR[k] <= plane[k] <= PLANE_REF_ERROR[k], (k, plane[k])
    assert plane[0] < 0.004 and plane[1] < np.deg2rad(0.1)  # the reference itself recovers 2 cm / 0.5 degrees to a fraction


# ------------------------------------------------------------------ GPU
def dev_scene(name):
    s = scene(name)
    t = {k: torch.from_numpy(s[k]).to(DEV) for k in ("td", "tc", "sd", "sc")}
    K = torch.eye(4).repeat(2, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = s["K"]
    t["K"] = K.to(DEV)
    return t


def dev_T(T):
    return torch.from_numpy(np.asarray(T, dtype=np.float32)).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES))
def test_pyramid_matches_the_float64_reference(name):
    """Bounds from the operation chain, relative (all terms are positive): intensity at level 0 passes one product, two additions
    and the scale = 4 roundings, every level adds 3 additions (the quarter is exact); depth passes at most 3 rounded additions
    (the first adds to 0) and one division per level."""
    H, W, levels, _ = SIZES[name]
    s, t = scene(name), dev_scene(name)
    for frame in (("td", "tc"), ("sd", "sc")):
        pyr = ops.rgbd_pyramid_raw(t[frame[0]], t[frame[1]], levels)
        assert [tuple(p.shape) for p in pyr] == [(2, H >> l, W >> l, 2) for l in range(levels)]
        for b in range(2):
            ref, nears = ref_pyramid(s[frame[0]][b], s[frame[1]][b], levels, np.float64)
            for l in range(levels):
                got = pyr[l][b].cpu().numpy().astype(np.float64)
                I, D = ref[l]
                skip = np.zeros(D.shape, dtype=bool) if nears[l] is None else nears[l]
                assert not skip.any()
                assert np.array_equal(got[..., 1] > 0, D > 0), (name, frame, b, l)
                eI, eD = np.abs(got[..., 0] - I), np.abs(got[..., 1] - D)
                print(name, frame[0], b, "level", l, "intensity err / u", float((eI / np.abs(I)).max() / U), "depth err / u",
                      float((eD[D > 0] / D[D > 0]).max() / U))
                assert (eI <= (4 + 3 * l) * U * 1.00001 * np.abs(I)).all(), (name, frame, b, l)
                assert (eD <= 4 * l * U * 1.00001 * D).all(), (name, frame, b, l)
        if name == "48x64":  # the foreground rule acted: a coarse pixel on the sphere's rim holds the sphere's depth, not a mixture
            d0 = s["sd"][0]
            blocks = d0[: H // 2 * 2, : W // 2 * 2].reshape(H // 2, 2, W // 2, 2).transpose(0, 2, 1, 3).reshape(H // 2, W // 2, 4)
            rim = (blocks.min(-1) > 0) & (blocks.max(-1) - blocks.min(-1) > DDM)
            assert rim.sum() >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["true", "identity", "outside"])
@pytest.mark.parametrize("name", list(SIZES))
def test_rows_match_the_float64_reference(name, which):
    t = dev_scene(name)
    valid, rows, _ = ops.rgbd_rows_raw(t["td"], t["tc"], t["sd"], t["sc"], t["K"], dev_T(transforms(name)[which]))
    valid, rows = valid.cpu().numpy(), rows.cpu().numpy()
    assert not rows[valid == 0].any()
    for b in range(2):
        dev, n = compare_rows(valid[b], rows[b], name, which, b)
        print(name, which, "b", b, "valid compared", n, "deviation per group", dev, "bound", [4 * x for x in ROWS_TRANSCRIPTION])
        compare_rows(valid[b], rows[b], name, which, b, bound=[4 * x for x in ROWS_TRANSCRIPTION])
        if name != "5x7":
            assert n >= 0.3 * valid[b].size


def chain_length(H, W):
    """The longest chain of fp32 additions a term passes through: 6 butterfly steps in its wave, the block's 4 waves in order,
    its group's rows (g, g + 32, ...) in order, the 32 groups in order."""
    nblocks = -(-H * W // 256)
    return 6 + 4 + -(-nblocks // 32) + 32


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES) + list(MORE_SIZES))
def test_sums_are_the_fixed_order_sums_of_the_rows_and_repeat_bitwise(name):
    H, W = {**SIZES, **MORE_SIZES}[name][:2]
    t = dev_scene(name)
    T = dev_T(transforms(name)["true"])
    valid, rows, sums = ops.rgbd_rows_raw(t["td"], t["tc"], t["sd"], t["sc"], t["K"], T)
    valid2, rows2, sums2 = ops.rgbd_rows_raw(t["td"], t["tc"], t["sd"], t["sc"], t["K"], T)
    assert torch.equal(sums, sums2) and torch.equal(rows, rows2) and torch.equal(valid, valid2)
    k = chain_length(H, W)
    assert k == {"48x64": 43, "30x45": 43, "5x7": 43, "96x130": 44, "256x512": 58, "257x512": 59, "288x512": 60, "512x512": 74,
                 "513x512": 75, "544x512": 76}[name]
    if name in FOLD_ROWS:  # the partial rows sit on either side of a round of reduce_partials (32 groups x 16 loads)
        nrows, rounds = FOLD_ROWS[name]
        assert -(-H * W // 256) == nrows and -(-nrows // (32 * 16)) == rounds
    valid, rows, sums = valid.cpu().numpy(), rows.cpu().numpy(), sums.cpu().numpy()
    for b in range(2):
        r = rows[b].reshape(-1, 14)
        JI, rI, JD, rD = r[:, :6], r[:, 6], r[:, 7:13], r[:, 13]
        terms = [JI[:, m] * JI[:, n] + JD[:, m] * JD[:, n] for m in range(6) for n in range(m, 6)]
        terms += [-(JI[:, m] * rI + JD[:, m] * rD) for m in range(6)]
        terms.append(rI * rI + rD * rD)
        worst = 0.0
        for q, term in enumerate(terms):
            assert term.dtype == np.float32
            # (at the fold's seams: the float64 sum -- its error of at most n 2^-53 sum |term| is nothing beside the bound,
            # and the exact fp32 sum would take tens of seconds of Python at a quarter of a million rows)
            exact = float(term.sum(dtype=np.float64)) if name in FOLD_ROWS else float(exact_sum_f32(term))
            bound = k * U * float(np.abs(term.astype(np.float64)).sum())
            err = abs(float(sums[b, q]) - exact)
            worst = max(worst, err / bound if bound > 0 else 0.0)
            assert err <= bound, (name, b, q, err, bound)
        print(name, "b", b, "k", k, "worst error / bound", worst)
        assert sums[b, 28] == float(valid[b].sum()) and sums[b, 28] > (6 if name == "5x7" else 1000)
        if name in FOLD_ROWS:  # what the last round alone carries: a round left out would show in the count
            in_last = int(valid[b].reshape(-1)[(FOLD_ROWS[name][0] - 1) // 512 * 512 * 256:].sum())
            print(name, "b", b, "valid pixels behind the last round's rows", in_last)
            assert in_last > 1000 or name in ("257x512", "513x512")


def run_device(name, numiters=None, init=None, zero_source=None):
    _, _, levels, counts = SIZES[name]
    t = dev_scene(name)
    sd = t["sd"]
    if zero_source is not None:
        sd = sd.clone()
        sd[zero_source] = 0.0
    return ops.rgbd_odometry(t["td"], t["tc"], sd, t["sc"], t["K"], init=init, numiters=numiters or counts, levels=levels)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES))
def test_whole_call_matches_the_float64_reference(name):
    _, _, levels, counts = SIZES[name]
    T, info = run_device(name)
    T2, info2 = run_device(name)
    assert torch.equal(T, T2) and torch.equal(info, info2)  # bit-identical from run to run
    T, info = T.cpu().numpy(), info.cpu().numpy()
    bound = [4 * x for x in T_TRANSCRIPTION[name]]
    for b in range(2):
        want, winfo, _ = odometry_reference(name, b)
        dev = t_deviation(T[b], want)
        print(name, "b", b, "T deviation (rot, trans)", dev, "bound", bound, "device info", info[b].tolist(), "reference", winfo.tolist(),
              "error against the truth", pose_error(T[b], scene(name)["T"][b]), "reference's", pose_error(want, scene(name)["T"][b]))
        assert np.array_equal(T[b][3], [0, 0, 0, 1])
        assert np.array_equal(info[b][:, 2:], winfo[:, 2:])  # status bits and iteration counts
        assert (np.abs(info[b][:, 0] - winfo[:, 0]) <= max(3, 0.01 * winfo[:, 0].max())).all()  # a handful of pixels may flip
        assert dev[0] <= bound[0] and dev[1] <= bound[1], (name, b, dev, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES))
def test_init_is_honoured(name):
    _, _, levels, counts = SIZES[name]
    wants, inits = zip(*(init_reference(name, b, np.float64) for b in range(2)))
    T, info = run_device(name, numiters=(counts[0],) + (0,) * (levels - 1), init=dev_T(np.stack(inits)))
    T, info = T.cpu().numpy(), info.cpu().numpy()
    bound = [4 * x for x in T_TRANSCRIPTION[name]]
    for b in range(2):
        dev = t_deviation(T[b], wants[b])
        print(name, "b", b, "T deviation from the init run's reference", dev, "bound", bound)
        assert dev[0] <= bound[0] and dev[1] <= bound[1], (name, b, dev, bound)
        assert not info[b][1:].any() and info[b][0, 3] == counts[0]  # levels without iterations: zeros
    # no iterations at all: the init comes back
    T0, _ = run_device(name, numiters=(0,) * levels, init=dev_T(np.stack(inits)))
    assert torch.equal(T0, dev_T(np.stack(inits)))


@pytest.mark.gpu
def test_a_source_without_valid_depth_returns_its_init_and_sets_the_status_bit():
    name = "48x64"
    init = dev_T(np.stack([make_pose(rot(0.001, 0.002, -0.001), (0.003, -0.002, 0.001))] * 2))
    T_all, info_all = run_device(name, init=init)
    T, info = run_device(name, init=init, zero_source=1)
    assert torch.equal(T[1], init[1])
    info = info.cpu().numpy()
    assert (info[1][:, 2] == 1).all() and (info[1][:, 0] == 0).all() and np.array_equal(info[1][:, 3], SIZES[name][3])
    assert torch.equal(T[0], T_all[0]) and torch.equal(torch.from_numpy(info[0]), info_all[0].cpu())  # the other element is unaffected
    assert (info[0][:, 2] == 0).all() and not torch.equal(T[0], init[0])


def plane_frames():
    p = plane_scene()
    K = torch.eye(4).view(1, 1, 4, 4).clone()
    K[0, 0, 0, 0], K[0, 0, 1, 1], K[0, 0, 0, 2], K[0, 0, 1, 2] = p["K"]
    mk = lambda d, c: gs.RGBDImages(torch.from_numpy(c).view(1, 1, 48, 64, 3).to(DEV), torch.from_numpy(d).view(1, 1, 48, 64, 1).to(DEV),
                                    K.to(DEV), torch.eye(4).view(1, 1, 4, 4).to(DEV))
    return mk(p["td"], p["tc"]), mk(p["sd"], p["sc"])


@pytest.mark.gpu
@pytest.mark.parametrize("channels_first", [False, True])
def test_the_colour_recovers_the_motion_in_the_plane_that_icp_cannot_see(channels_first):
    """A textured plane facing the camera, moved 2 cm in the plane and 0.5 degrees about its normal: point-to-plane ICP leaves
    exactly these three degrees of freedom to the damping.  Measured on the MI355X: RGB-D 7.5e-5 m, 7.4e-5 rad (the float64 reference: 7.5e-5 m,
    7.4e-5 rad); ICP 0.02 m, 8.7e-3 rad -- it stays at the identity."""
    from gradslam_amd.structures.utils import pointclouds_from_rgbdimages

    target, source = plane_frames()
    clouds = [pointclouds_from_rgbdimages(f, global_coordinates=False) for f in (target, source)]
    if channels_first:
        target, source = target.to_channels_first(), source.to_channels_first()
    prov = gs.odometry.RGBDOdometryProvider()
    T = prov.provide(target, source)
    assert T.shape == (1, 1, 4, 4) and not T.requires_grad and tuple(prov.last_info.shape) == (1, 3, 4) and prov.last_info.is_cuda
    err = pose_error(T[0, 0].cpu().numpy(), PLANE_T)
    T_icp = gs.odometry.ICPOdometryProvider(numiters=20).provide(clouds[0], clouds[1])
    err_icp = pose_error(T_icp[0, 0].cpu().numpy(), PLANE_T)
    print("RGB-D error (m, rad)", err, "float64 reference's", PLANE_REF_ERROR, "ICP's", err_icp, "info", prov.last_info.cpu().tolist())
    assert err[0] <= 2 * PLANE_REF_ERROR[0] and err[1] <= 2 * PLANE_REF_ERROR[1]
    assert err_icp[0] > err[0] and err_icp[1] > err[1]
    # the same through init = the answer: it stays there (to the same bound)
    T2 = prov.provide(target, source, init=T)
    err2 = pose_error(T2[0, 0].cpu().numpy(), PLANE_T)
    assert err2[0] <= 2 * PLANE_REF_ERROR[0] and err2[1] <= 2 * PLANE_REF_ERROR[1]


@pytest.mark.gpu
def test_kinectfusion_tracks_with_rgbd_and_icp_is_what_it_was():
    """The scene and the bound of tests/test_kinectfusion.py (odom="icp" against the ground truth: ATE <= max(2 ATE_icpslam,
    voxel_size)).  Measured on the MI355X: ATE 0.0136 m with odom="rgbd" (the sequence's colours are
    independent noise per frame, so the photometric term only disturbs here), ICPSLAM 0.0304 m."""
    from gradslam_amd.geometry.geometryutils import compose_transformations
    from gradslam_amd.metrics import absolute_trajectory_error
    from gradslam_amd.odometry.icputils import downsample_rgbdimages
    from gradslam_amd.slam import ICPSLAM
    from tests import test_kinectfusion as tk

    fr = tk.frames(1)
    slam = tk.kf(1, odom="rgbd", numiters=(10, 5, 3))
    volume, poses = slam(fr)
    poses_again = tk.kf(1, odom="rgbd", numiters=(10, 5, 3))(fr)[1]
    assert poses.shape == (1, tk.L, 4, 4) and torch.isfinite(poses).all() and torch.equal(poses, poses_again)
    assert torch.equal(poses[:, 0], fr.poses[:, 0]) and int((volume.weight > 0).sum()) > 1000
    assert (slam.odomprov.last_info[..., 2] == 0).all() and (slam.odomprov.last_info[..., 0] > 100).all()
    _, ref_poses = ICPSLAM(odom="icp", dsratio=4, device=DEV)(fr)
    ate, ate_icpslam = absolute_trajectory_error(poses, fr.poses), absolute_trajectory_error(ref_poses, fr.poses)
    print("ATE KinectFusion(rgbd)", ate.tolist(), "ATE ICPSLAM", ate_icpslam.tolist())
    assert (ate <= torch.clamp(2 * ate_icpslam, min=tk.V)).all()
    assert not torch.equal(poses[:, 1:], fr.poses[:, :-1].expand_as(poses[:, 1:]))  # it moved
    # odom="icp" is what it was: the driver against the hand composition of the public pieces, a path this change does not touch
    icp = tk.kf(1)
    _, icp_poses = icp(fr)
    vol_h = gs.TSDFVolume(tk.DIMS, tk.V, origin=tk.ORIGINS[:1], trunc=tk.TRUNC, device=DEV)
    pose = fr.poses[:, :1]
    for s in range(tk.L):
        live = gs.RGBDImages(fr.rgb_image[:, s:s + 1], fr.depth_image[:, s:s + 1], fr.intrinsics, pose)
        if s > 0:
            target = vol_h.raycast_pointcloud(fr.intrinsics, pose, tk.H, tk.W, stride=4, step=None, min_weight=1.0)
            T = icp.odomprov.provide(target, downsample_rgbdimages(live, 4))
            pose = compose_transformations(T.squeeze(1), pose.squeeze(1)).unsqueeze(1)
            live = gs.RGBDImages(fr.rgb_image[:, s:s + 1], fr.depth_image[:, s:s + 1], fr.intrinsics, pose)
        assert torch.equal(pose[:, 0], icp_poses[:, s]), s
        vol_h = vol_h.integrate(live)
    # under autograd with inputs that require gradients the rgbd driver refuses instead of cutting the graph
    d = fr.depth_image.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gradients"):
        tk.kf(1, odom="rgbd", numiters=2)(gs.RGBDImages(fr.rgb_image, d, fr.intrinsics, fr.poses))
