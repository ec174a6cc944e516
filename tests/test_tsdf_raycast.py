"""TSDF ray casting (gs_tsdf_raycast and its reverse pass, ops.tsdf_raycast*, TSDFVolume.raycast / raycast_pointcloud).

The references are written here in numpy and torch, not taken from the code under test:
* ref_cast: the rule of include/gradslam_hip.h vectorised over the pixels.  Rays, dz and z_k = (float)k * dz are numpy float32
  in the order the rule states them; positions, samples, the march and the hit are float64 (the reference) or float32 (the
  transcription that measures what fp32 alone costs).  A pixel is left out when, on its ray up to the ending sample or at p*,
  an observed |f| is below 1e-5 or a grid coordinate lies within 1e-5 of an integer: there fp32 and float64 may decide
  differently.  At most 5 % of an image may be left out.
* the scene is hand-made on the host: tsdf = clip(d / trunc, -1, 1), d the smaller of a tilted plane's and a sphere's signed
  distance; weight 1 where d > -trunc and x < 0.8, else 0 (tsdf 1 there), less single voxels at the surface (they drop hits at
  p*); smooth colours.  Four cameras: slightly rotated in front of the sphere; the identity with integer cx, cy (rays parallel
  to the axes); inside the sphere (rays that start at f < 0); outside the box.  A ray that grazes the sphere has
  f_prev - f << 1 and turns one rounding of f into many of z*: sphere and cameras were placed, on the CPU, so that the float32
  transcription stays within 6.6e-7 m of the float64 reference (TRANSCRIPTION, asserted below) -- the 5.0e-7 m of the issue's
  scene within a third -- and the device's bound of 2e-6 m keeps the factor it was built with.
* reverse pass: the explicit formulas of the header in float64 (ref_cast_backward), checked against torch float64 autograd of
  the reference with the decisions held constant.  Run on absolute values they give A, the sum of the absolute terms of every
  element; the device's sums are exact, what differs is each term, and the bound is 32 * 2^-24 * A.  Like the forward reference,
  which is evaluated at the same fp32 rays, dz and z_k, the formulas are evaluated at the same fp32 samples: the fractions
  a = g - i, the values f_prev, f and the hit's cell come from the float32 transcription of the rule (whose forward the device
  reproduces digit for digit) and are promoted.  A fraction is a difference of numbers of size |g| ~ 40 and carries an absolute
  error of about 40 * 2^-24 between fp32 and float64, so a corner weight 1 - a near 0 has no relative accuracy across the two:
  with the float64 samples instead, the float32 transcription itself, no device involved, misses 32 * 2^-24 * A by a factor
  of 4e4 (test_reverse_formulas_... asserts that this is so).
"""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops
from gradslam_amd.metrics import chamfer_distance
from gradslam_amd.structures.utils import pointclouds_from_rgbdimages
from gradslam_amd.synthetic import make_sequence
from tests.helpers import exact_sum_f32

DEV = "cuda:0"
U = 2.0 ** -24
F32 = np.float32
NEW_SYMBOLS = {"gs_tsdf_raycast": 24, "gs_tsdf_raycast_backward_ws_bytes": 5, "gs_tsdf_raycast_backward": 25}

# the common scene (test_tsdf.py's volume)
DIMS, V, TRUNC = (42, 22, 56), 0.05, 0.15
ORIGINS = [(-1.0, -0.55, -0.2), (-0.95, -0.5, -0.15)]
H, W = 48, 64
TIE = 1e-5
SPHERE = (0.084, -0.017, 1.141, 0.412)
STEPS = (TRUNC / 2, V)
# the largest deviation of the float32 transcription from the float64 reference over the cameras, both origins and both steps
# (depth [m], normal, colour; measured on the CPU, asserted by test_float32_transcription_...); the device gets four times that
TRANSCRIPTION = (6.6e-7, 5.9e-7, 4.7e-7)
DEPTH_BOUND = 2e-6  # the issue's
NORMAL_BOUND, COLOR_BOUND = 4 * TRANSCRIPTION[1], 4 * TRANSCRIPTION[2]


# ------------------------------------------------------------------ the scene and the references
def make_K():
    K = np.eye(4, dtype=F32); K[0, 0] = K[1, 1] = 60.0; K[0, 2] = 32.0; K[1, 2] = 24.0
    return K

def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx

def make_pose(R, t):
    P = np.eye(4); P[:3, :3] = R; P[:3, 3] = t
    return P.astype(F32)

POSES = {
    "rotated": make_pose(rot(0.0, -0.049, 0.028), (0.099, -0.054, 0.13)),
    "identity": make_pose(np.eye(3), (0.0, 0.0, 0.0)),
    "inside": make_pose(rot(0.0, 0.3, 0.0), (0.084, -0.017, 1.141)),
    "outside": make_pose(rot(0.038, 0.418, -0.042), (-1.302, 0.122, -0.438)),
}

def make_volume(origin, dims=DIMS, v=V, trunc=TRUNC):
    """(tsdf, weight (nz, ny, nx), color (nz, ny, nx, 3)) float32 of one batch element."""
    sc = SPHERE
    nx, ny, nz = dims
    o = np.asarray(origin, F32)
    ax = [(o[k] + (np.arange(n, dtype=F32) + F32(0.5)) * F32(v)).astype(np.float64) for k, n in enumerate(dims)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    n = np.array([0.1, 0.05, -1.0]); n /= np.linalg.norm(n)
    plane = n[0] * x + n[1] * y + n[2] * (z - 2.0)
    sphere = np.sqrt((x - sc[0]) ** 2 + (y - sc[1]) ** 2 + (z - sc[2]) ** 2) - sc[3]
    d = np.minimum(plane, sphere)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    hole = (np.abs(d) < v) & ((7 * ix + 13 * iy + 5 * iz) % 61 == 0)  # single unobserved voxels at the surface: they drop hits at p*
    obs = (d > -trunc) & (x < 0.8) & ~hole
    tsdf = np.where(obs, np.clip(d / trunc, -1, 1), 1.0).astype(F32)
    weight = obs.astype(F32)
    color = np.stack([0.5 + 0.4 * np.sin(2 * x + 1), 0.5 + 0.4 * np.cos(3 * y - z), 0.3 + 0.2 * np.sin(x + 2 * y + 3 * z)], -1).astype(F32)
    return tsdf, weight, color

def ref_rays(K, P, height, width, stride, step):
    """The ray rule in numpy float32, in the order written: -> t (3,), dw (Ho,Wo,3), dz (Ho,Wo), all float32."""
    K, P = np.asarray(K, F32), np.asarray(P, F32)
    w = np.arange(0, width, stride).astype(F32)[None, :]
    h = np.arange(0, height, stride).astype(F32)[:, None]
    dx = np.broadcast_to((w - K[0, 2]) / K[0, 0], (h.shape[0], w.shape[1]))
    dy = np.broadcast_to((h - K[1, 2]) / K[1, 1], (h.shape[0], w.shape[1]))
    dw = np.stack([(P[i, 0] * dx + P[i, 1] * dy) + P[i, 2] for i in range(3)], -1)
    dz = F32(step) / np.sqrt((dx * dx + dy * dy) + F32(1))
    assert dw.dtype == F32 and dz.dtype == F32
    return P[:3, 3].copy(), dw, dz

def lerp(p, q, s):
    return p + s * (q - p)

def trilerp(c, a):
    """c (..., 8) corner values, corner = x + 2 y + 4 z; a (..., 3)."""
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    c00, c10 = lerp(c[..., 0], c[..., 1], ax), lerp(c[..., 2], c[..., 3], ax)
    c01, c11 = lerp(c[..., 4], c[..., 5], ax), lerp(c[..., 6], c[..., 7], ax)
    return lerp(lerp(c00, c10, ay), lerp(c01, c11, ay), az)

def trigrad(c, a):
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    gx = lerp(lerp(c[..., 1] - c[..., 0], c[..., 3] - c[..., 2], ay), lerp(c[..., 5] - c[..., 4], c[..., 7] - c[..., 6], ay), az)
    gy = lerp(lerp(c[..., 2] - c[..., 0], c[..., 3] - c[..., 1], ax), lerp(c[..., 6] - c[..., 4], c[..., 7] - c[..., 5], ax), az)
    gz = lerp(lerp(c[..., 4] - c[..., 0], c[..., 5] - c[..., 1], ax), lerp(c[..., 6] - c[..., 2], c[..., 7] - c[..., 3], ax), ay)
    return np.stack([gx, gy, gz], -1)

def corner_ids(i, dims):
    """i (..., 3) int cell -> (..., 8) flat voxel ids."""
    nx, ny, nz = dims
    j = (i[..., 2] * ny + i[..., 1]) * nx + i[..., 0]
    off = np.array([(c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nx * ny for c in range(8)])
    return j[..., None] + off

def ref_sample(vol, p, minw, dt):
    """One sample per row of p (n, 3) in dtype dt -> dict(obs, f, i, a, ids, tie)."""
    tsdf, weight, origin, v, dims = vol["tsdf"], vol["weight"], vol["origin"], vol["v"], vol["dims"]
    o = np.asarray(origin, F32).astype(dt)
    g = (p - o) / dt(F32(v)) - dt(0.5)
    fi = np.floor(g)
    nmax = np.array(dims, dtype=dt) - dt(1)
    with np.errstate(invalid="ignore"):
        inside = np.all((fi >= 0) & (fi + 1 <= nmax), -1)
        tie = np.any(np.abs(g - np.rint(g)) < TIE, -1)
    i = np.where(inside[:, None], fi, 0).astype(np.int64)
    a = (g - fi).astype(dt)
    ids = np.where(inside[:, None], corner_ids(i, dims), 0)  # (outside: no voxel is read)
    w8 = weight.reshape(-1)[ids]
    obs = inside & np.all(w8 >= minw, -1)
    f = trilerp(tsdf.reshape(-1)[ids].astype(dt), a)
    assert f.dtype == dt
    return dict(obs=obs, f=f, i=i, a=a, ids=ids, tie=tie)

def ref_cast(vol, K, P, height, width, stride, step, near=0.0, far=np.inf, minw=1.0, dt=np.float64, kmax=None):
    """The rule, vectorised over the pixels, in dtype dt (float64: the reference; float32: the transcription).  Rays, dz and
    z_k are fp32 in both.  -> dict of (Ho, Wo) arrays: k_end, depth, normal, rgb, branch (0 never ends, 1 ends without a hit,
    2 dropped at p*, 3 hit), tie, and the per-pixel records of the reverse pass."""
    t, dw, dz = ref_rays(K, P, height, width, stride, step)
    Ho, Wo = dz.shape
    n = Ho * Wo
    dw, dz = dw.reshape(n, 3), dz.reshape(n)
    tD, dwD = t.astype(dt), dw.astype(dt)
    if kmax is None:
        o = np.asarray(vol["origin"], np.float64)
        corners = np.array([[o[a] + (c >> a & 1) * vol["dims"][a] * vol["v"] for a in range(3)] for c in range(8)])
        reach = np.max(np.linalg.norm(corners - t.astype(np.float64), axis=1))
        kmax = int(reach / step) + 3
    done = np.zeros(n, bool); prev_ok = np.zeros(n, bool); tie = np.zeros(n, bool)
    f_prev = np.zeros(n, dt); branch = np.zeros(n, np.int64); k_end = np.zeros(n, np.int64)
    rec = dict(f0=np.zeros(n, dt), f1=np.zeros(n, dt), i0=np.zeros((n, 3), np.int64), i1=np.zeros((n, 3), np.int64),
               a0=np.zeros((n, 3), dt), a1=np.zeros((n, 3), dt))
    prev_i, prev_a = np.zeros((n, 3), np.int64), np.zeros((n, 3), dt)
    for k in range(1, kmax + 1):
        zk = (F32(k) * dz)
        assert zk.dtype == F32
        on = ~done & (zk >= F32(near)) & (zk <= F32(far))
        s = ref_sample(vol, tD + zk.astype(dt)[:, None] * dwD, minw, dt)
        obs = on & s["obs"]
        tie |= on & (s["tie"] | (s["obs"] & (np.abs(s["f"]) < TIE)))
        end = obs & (s["f"] < 0)
        hit = end & prev_ok
        branch[end] = 1
        branch[hit] = 3
        k_end[hit] = k
        for name, val in (("f0", f_prev), ("f1", s["f"]), ("i0", prev_i), ("i1", s["i"]), ("a0", prev_a), ("a1", s["a"])):
            rec[name][hit] = val[hit]
        done |= end
        prev_ok = obs & (s["f"] >= 0)
        f_prev = np.where(prev_ok, s["f"], 0).astype(dt)
        prev_i, prev_a = s["i"], s["a"]
    hit = branch == 3
    with np.errstate(all="ignore"):
        sfrac = np.where(hit, rec["f0"] / (rec["f0"] - rec["f1"]), 0).astype(dt)
    if dt == np.float32:
        zs = ((k_end - 1).astype(F32) + sfrac) * dz
    else:
        zs = ((k_end - 1).astype(dt) + sfrac) * dz.astype(dt)
    ps = tD + zs[:, None] * dwD
    s = ref_sample(vol, ps, minw, dt)
    tie |= hit & (s["tie"])
    c8 = vol["tsdf"].reshape(-1)[s["ids"]].astype(dt)
    g = trigrad(c8, s["a"])
    nn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    ok = hit & s["obs"] & (nn > 0)
    branch[hit & ~ok] = 2
    k_end[~ok] = 0
    with np.errstate(all="ignore"):
        normal = np.where(ok[:, None], g / nn[:, None], 0)
    depth = np.where(ok, zs, 0)
    rgb = None
    if vol.get("color") is not None:
        col = vol["color"].reshape(-1, 3)
        rgb = np.stack([np.where(ok, trilerp(col[:, ch][s["ids"]].astype(dt), s["a"]), 0) for ch in range(3)], -1)
    rec.update(ih=s["i"], ah=s["a"], dz=dz, dw=dw, t=t, hit=ok.copy(), k=k_end.copy())
    sh = lambda x: x.reshape((Ho, Wo) + x.shape[1:])
    return dict(k_end=sh(k_end), depth=sh(depth), normal=sh(normal), rgb=None if rgb is None else sh(rgb), branch=sh(branch), tie=sh(tie),
                rec=rec)


def corner_w(a):
    """(n, 8) trilinear weights (wx wy) wz of the fractions a (n, 3)."""
    out = []
    for c in range(8):
        wx = a[:, 0] if c & 1 else 1 - a[:, 0]
        wy = a[:, 1] if c & 2 else 1 - a[:, 1]
        wz = a[:, 2] if c & 4 else 1 - a[:, 2]
        out.append((wx * wy) * wz)
    return np.stack(out, -1)


def ref_cast_backward(vol, rec, g_depth, g_rgb, absolute=False):
    """The explicit reverse formulas in float64 at the records rec of the hit pixels (the samples' cells, fractions and values,
    promoted) -> (g_tsdf (nvox,), g_color (nvox, 3) or None).  absolute=True: run on absolute values, A: per element the sum of
    its absolute terms (g_z as |g_depth| + sum_ch |its colour term|)."""
    dims, v = vol["dims"], float(F32(vol["v"]))
    nvox = dims[0] * dims[1] * dims[2]
    hit = rec["hit"]
    D = lambda x: x[hit].astype(np.float64)
    P = np.abs if absolute else (lambda x: x)
    f0, f1, dz, dw, a0, a1, ah = D(rec["f0"]), D(rec["f1"]), D(rec["dz"]), D(rec["dw"]), D(rec["a0"]), D(rec["a1"]), D(rec["ah"])
    ids0, ids1, idsh = corner_ids(rec["i0"][hit], dims), corner_ids(rec["i1"][hit], dims), corner_ids(rec["ih"][hit], dims)
    gz = P(g_depth.reshape(-1)[hit].astype(np.float64))
    den2 = (f0 - f1) ** 2
    g_tsdf, g_color = np.zeros(nvox), None
    if vol.get("color") is not None and g_rgb is not None:
        grgb = g_rgb.reshape(-1, 3)[hit].astype(np.float64)
        col = vol["color"].reshape(-1, 3).astype(np.float64)
        g_color = np.zeros((nvox, 3))
        wh = corner_w(ah)
        for ch in range(3):
            gz = gz + P(grgb[:, ch] * ((trigrad(col[:, ch][idsh], ah) * dw).sum(-1) / v))
            np.add.at(g_color[:, ch], idsh, P(grgb[:, ch][:, None] * wh))
    np.add.at(g_tsdf, ids0, P((gz * dz * (-f1) / den2)[:, None] * corner_w(a0)))
    np.add.at(g_tsdf, ids1, P((gz * dz * f0 / den2)[:, None] * corner_w(a1)))
    return g_tsdf, g_color


def trilerp_t(c, a):
    l = lambda p, q, s: p + s * (q - p)
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    return l(l(l(c[:, 0], c[:, 1], ax), l(c[:, 2], c[:, 3], ax), ay), l(l(c[:, 4], c[:, 5], ax), l(c[:, 6], c[:, 7], ax), ay), az)


def torch_cast(vol, rec, tsdf, color):
    """Depth and rgb of the hit pixels in torch float64 with the decisions of rec (cells, ending sample) as constants."""
    dims, v = vol["dims"], float(F32(vol["v"]))
    hit = rec["hit"]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    D = lambda x: T(x[hit].astype(np.float64))
    f0 = trilerp_t(tsdf[T(corner_ids(rec["i0"][hit], dims))], D(rec["a0"]))
    f1 = trilerp_t(tsdf[T(corner_ids(rec["i1"][hit], dims))], D(rec["a1"]))
    z = ((D(rec["k"]) - 1) + f0 / (f0 - f1)) * D(rec["dz"])
    p = T(rec["t"].astype(np.float64)) + z[:, None] * D(rec["dw"])
    a = (p - T(np.asarray(vol["origin"], F32).astype(np.float64))) / v - 0.5 - D(rec["ih"])
    ids = T(corner_ids(rec["ih"][hit], dims))
    return z, torch.stack([trilerp_t(color[:, ch][ids], a) for ch in range(3)], -1)


@lru_cache(maxsize=None)
def host_volume(b, weights=1):
    """One batch element of the common scene as the reference's dict; weights = 2: the weight is 2 where y < 0."""
    tsdf, weight, color = make_volume(ORIGINS[b])
    if weights == 2:
        nz, ny, nx = tsdf.shape
        y = ORIGINS[b][1] + (np.arange(ny) + 0.5) * V
        weight = weight * np.where(y < 0, 2, 1)[None, :, None].astype(F32)
    return dict(tsdf=tsdf, weight=weight, color=color, origin=ORIGINS[b], v=V, dims=DIMS)


@lru_cache(maxsize=None)
def reference(b, pose, step, stride=1, near=0.0, far=np.inf, minw=1.0, weights=1, dt=np.float64):
    """Computed once, shared by the tests, never written to."""
    return ref_cast(host_volume(b, weights), make_K(), POSES[pose], H, W, stride, step, near, far, minw, dt)


def compare(dev, ref, what, cap=0.05):
    """dev = (depth, normal, rgb or None, k_end) numpy images of the device, ref = ref_cast's dict: the ending sample and the hit
    mask are equal and depth, normal and colour lie within their bounds wherever the reference does not tie.
    -> the three largest deviations."""
    depth, normal, rgb, k_end = dev
    good = ~ref["tie"]
    assert (~good).mean() <= cap, (what, int((~good).sum()))
    assert np.array_equal(k_end[good], ref["k_end"][good]), (what, int((k_end != ref["k_end"])[good].sum()))
    miss = k_end == 0
    assert (depth[miss] == 0).all() and (normal[miss] == 0).all() and (rgb is None or (rgb[miss] == 0).all()), what
    hit = good & ~miss
    dev3 = [0.0, 0.0, 0.0]
    if hit.any():
        dev3[0] = float(np.abs(depth - ref["depth"])[hit].max())
        dev3[1] = float(np.abs(normal - ref["normal"])[hit].max())
        if rgb is not None:
            dev3[2] = float(np.abs(rgb - ref["rgb"])[hit].max())
    print(what, "hits", int(hit.sum()), "left out", int((~good).sum()), "deviation: depth %.3g normal %.3g colour %.3g" % tuple(dev3))
    assert dev3[0] <= DEPTH_BOUND and dev3[1] <= NORMAL_BOUND and dev3[2] <= COLOR_BOUND, (what, dev3)
    return dev3


# ------------------------------------------------------------------ CPU: ABI, error contracts, the references themselves
def test_raycast_symbols_load_and_are_declared():
    lib = nv.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
        assert name + "(" in header, name
        decl = header[header.index(name + "("):]
        assert decl[: decl.index(";")].count(",") + 1 == nargs, name
    assert lib.gs_abi_version() == 3
    assert hasattr(ops, "_TsdfRaycastFn") and hasattr(gs.TSDFVolume, "raycast") and hasattr(gs.TSDFVolume, "raycast_pointcloud")


def test_raycast_c_entry_points_refuse_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    lib = nv.lib()
    P = 4096
    inf, nan = float("inf"), float("nan")
    #     tsdf w col B  nx ny nz v    o  K  P  L  H  W  s  step  near far  minw depth nrm rgb kend stream
    ok = [P, P, P, 1, 4, 4, 4, 0.1, P, P, P, 2, 8, 8, 1, 0.05, 0.0, inf, 1.0, P, P, P, P, None]
    for pos in (0, 1, 8, 9, 10, 19, 20, 22, 2, 21):  # (the last two: colours go together)
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_raycast(*args) == -1, pos
    for pos, bad in ((3, 0), (3, 65536), (4, 0), (5, -1), (6, 0), (4, 1 << 30), (7, 0.0), (7, nan), (7, inf), (11, 0), (11, 65536), (12, 0),
                     (13, -2), (14, 0), (14, -1), (15, 0.0), (15, -0.05), (15, nan), (15, inf), (16, nan), (16, -0.5), (17, nan), (18, nan),
                     (15, 12 * 0.1 / (1 << 20) * 0.999)):  # (nx + ny + nz) v / step just above 2^20
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_raycast(*args) == -1, (pos, bad)
    assert b"gs_tsdf_raycast" in lib.gs_last_error()
    args = list(ok)
    args[15] = 1e-7
    assert lib.gs_tsdf_raycast(*args) == -1 and b"2^20" in lib.gs_last_error()
    args = list(ok)
    args[12], args[13] = 1, (1 << 31) - 1  # H W fits int32, the 16 x 16 tiles do not fit a launch
    assert lib.gs_tsdf_raycast(*args) == -1 and b"tiles" in lib.gs_last_error()

    n = 2 * 42 * 22 * 56
    assert lib.gs_tsdf_raycast_backward_ws_bytes(2, 42, 22, 56, 1) == 256 + 4 * n + 64 * n  # 16 B per voxel and channel (+ flags)
    assert lib.gs_tsdf_raycast_backward_ws_bytes(2, 42, 22, 56, 0) == 256 + 4 * n + 16 * n
    assert lib.gs_tsdf_raycast_backward_ws_bytes(0, 4, 4, 4, 1) == 0 and lib.gs_tsdf_raycast_backward_ws_bytes(1, 1024, 1024, 513, 0) == 0
    #     tsdf w col B  nx ny nz v    o  K  P  L  H  W  s  step  minw kend gd grgb gt gc ws  bytes    stream
    ok = [P, P, P, 1, 4, 4, 4, 0.1, P, P, P, 2, 8, 8, 1, 0.05, 1.0, P, P, P, P, P, P, 1 << 20, None]
    for pos in (0, 1, 8, 9, 10, 17, 20, 2, 21):
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_raycast_backward(*args) == -1, pos
    for pos, bad in ((3, 0), (4, 0), (7, -1.0), (11, 0), (12, 0), (14, 0), (15, 0.0), (15, nan), (15, inf), (15, 1e-7), (16, nan)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_raycast_backward(*args) == -1, (pos, bad)
    args = list(ok)
    args[22], args[23] = None, 0
    assert lib.gs_tsdf_raycast_backward(*args) == -2
    args = list(ok)
    args[23] = lib.gs_tsdf_raycast_backward_ws_bytes(1, 4, 4, 4, 1) - 1
    assert lib.gs_tsdf_raycast_backward(*args) == -2
    assert b"gs_tsdf_raycast_backward" in lib.gs_last_error()


def test_raycast_python_error_contracts():
    T = gs.structures.TSDFVolume
    with pytest.raises(ValueError, match="no CPU fallback"):
        T((4, 4, 4), 0.1, device="cpu")
    # a volume that is not on a device: the checks of types and batch sizes come first, then the ops refuse its tensors
    vol = object.__new__(T)
    vol._B, vol.dims, vol.voxel_size, vol.trunc = 2, (4, 4, 4), 0.1, 0.4
    vol.tsdf, vol.weight, vol.color = torch.ones(2, 4, 4, 4), torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4, 4, 3)
    vol.origin = torch.zeros(2, 3)
    K, poses = torch.eye(4).expand(2, 1, 4, 4).contiguous(), torch.eye(4).expand(2, 3, 4, 4).contiguous()
    for fn in (vol.raycast, vol.raycast_pointcloud):
        with pytest.raises(TypeError, match="tensor"):
            fn([1.0], poses[:, :1], 8, 8)
        with pytest.raises(TypeError, match="tensor"):
            fn(K, None, 8, 8)
        with pytest.raises(ValueError, match="Batch size"):
            fn(K, poses[:1, :1], 8, 8)
        with pytest.raises(ValueError, match="Batch size"):
            fn(K[:1], poses[:, :1], 8, 8)
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(K, poses[:, :1], 8, 8)
    with pytest.raises(ValueError, match="L = 1"):
        vol.raycast_pointcloud(K, poses, 8, 8)
    t, w, c, o = vol.tsdf, vol.weight, vol.color, (0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_raycast_raw(t, w, c, o, 0.1, K, poses, 8, 8, 1, 0.05)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_raycast(t, w, c, o, 0.1, K, poses, 8, 8, 1, 0.05)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_raycast_backward_raw(t, w, c, o, 0.1, K, poses, 8, 8, 1, 0.05, 1.0, torch.zeros(2, 3, 8, 8, dtype=torch.int32))


def test_reference_on_a_fronto_parallel_plane_gives_the_closed_form():
    """tsdf = clip((z0 - z) / trunc): the interpolant of a linear function is the function, so every hit lies at depth z0 with
    the normal (0, 0, -1), whatever the pixel, the step and the stride."""
    dims, v, trunc, z0 = (24, 20, 30), 0.05, 0.15, 0.8125
    origin = (-0.6, -0.5, 0.0)
    z = origin[2] + (np.arange(dims[2]) + 0.5) * v
    tsdf = np.broadcast_to(np.clip((z0 - z) / trunc, -1, 1)[:, None, None], dims[::-1]).astype(np.float64)
    vol = dict(tsdf=tsdf, weight=np.ones(dims[::-1], F32), color=None, origin=origin, v=v, dims=dims)
    for step, stride in ((trunc / 2, 1), (v, 3)):
        r = ref_cast(vol, make_K(), np.eye(4, dtype=F32), H, W, stride, step)
        hit = r["k_end"] > 0
        assert hit.sum() > 0.3 * hit.size and (r["branch"][~hit] == 0).all()  # the others leave the box by its sides
        assert np.abs(r["depth"][hit] - z0).max() < 1e-6  # (tsdf's float64 values of a float32 voxel size: 1e-7 of rounding)
        assert np.abs(r["normal"][hit] - np.array([0.0, 0.0, -1.0])).max() < 1e-6


def test_reverse_formulas_against_float64_autograd():
    vol = host_volume(0)
    rec = reference(0, "rotated", STEPS[0])["rec"]
    assert rec["hit"].sum() > 1000
    rng = np.random.RandomState(0)
    gd, gc = rng.randn(H, W), rng.randn(H, W, 3)
    g_t, g_c = ref_cast_backward(vol, rec, gd, gc)
    tt = torch.from_numpy(vol["tsdf"].reshape(-1).astype(np.float64)).requires_grad_(True)
    cc = torch.from_numpy(vol["color"].reshape(-1, 3).astype(np.float64)).requires_grad_(True)
    z, rgb = torch_cast(vol, rec, tt, cc)
    ref = reference(0, "rotated", STEPS[0])
    assert np.abs(z.detach().numpy() - ref["depth"].reshape(-1)[rec["hit"]]).max() < 1e-12
    assert np.abs(rgb.detach().numpy() - ref["rgb"].reshape(-1, 3)[rec["hit"]]).max() < 1e-12
    hit = rec["hit"]
    ((z * torch.from_numpy(gd.reshape(-1)[hit])).sum() + (rgb * torch.from_numpy(gc.reshape(-1, 3)[hit])).sum()).backward()
    assert np.abs(g_t).max() > 0.1 and np.abs(g_c).max() > 0.1
    assert np.abs(tt.grad.numpy() - g_t).max() < 1e-12 * np.abs(g_t).max()
    assert np.abs(cc.grad.numpy() - g_c).max() < 1e-12 * np.abs(g_c).max()
    A_t, A_c = ref_cast_backward(vol, rec, gd, gc, absolute=True)
    assert (A_t >= np.abs(g_t)).all() and (A_c >= np.abs(g_c)).all()
    # why the device is compared at the float32 samples: between the float64 and the float32 samples of the same pixels the
    # formulas differ by far more than 32 * 2^-24 * A, with no device involved
    r32 = reference(0, "rotated", STEPS[0], dt=np.float32)
    same = rec["hit"] & r32["rec"]["hit"] & (rec["k"] == r32["rec"]["k"]) & ~ref["tie"].reshape(-1)
    rec32, rec64 = dict(r32["rec"], hit=same), dict(rec, hit=same)
    t32, c32 = ref_cast_backward(vol, rec32, gd, gc)
    t64, c64 = ref_cast_backward(vol, rec64, gd, gc)
    A_t, A_c = ref_cast_backward(vol, rec64, gd, gc, absolute=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        p_t, p_c = np.nanmax(np.abs(t32 - t64) / (U * A_t)), np.nanmax(np.abs(c32 - c64) / (U * A_c))
    print("float64 samples against float32 samples, in units of 2^-24 A: g_tsdf %.3g g_color %.3g" % (p_t, p_c))
    assert p_t > 32 and p_c > 32


def test_float32_transcription_populates_every_branch_and_stays_within_what_the_bounds_were_built_from():
    worst = np.zeros(3)
    for b in range(2):
        for step in STEPS:
            branches = np.zeros(4, np.int64)
            for pose in POSES:
                r64, r32 = reference(b, pose, step), reference(b, pose, step, dt=np.float32)
                branches += np.bincount(r64["branch"].ravel(), minlength=4)
                good = ~r64["tie"]
                assert (~good).mean() <= 0.05
                assert np.array_equal(r64["k_end"][good], r32["k_end"][good]), (b, pose, step)
                hit = good & (r64["k_end"] > 0)
                if hit.any():
                    worst = np.maximum(worst, [np.abs(r64[k] - r32[k])[hit].max() for k in ("depth", "normal", "rgb")])
            # never ends, ends without a hit, dropped at p*, hit
            assert branches[0] > 100 and branches[1] > 100 and branches[2] >= 5 and branches[3] > 1000, (b, step, branches)
    print("float32 transcription against float64: depth %.3g m, normal %.3g, colour %.3g" % tuple(worst))
    assert (worst <= np.array(TRANSCRIPTION)).all(), worst
    r = reference(0, "identity", STEPS[0])["rec"]
    assert (r["dw"][:, 0] == 0).sum() == H and (r["dw"][:, 1] == 0).sum() == W  # the centre column and row: rays parallel to an axis
    assert (reference(0, "inside", STEPS[0])["branch"] == 1).mean() > 0.9  # rays that start at f < 0


# ------------------------------------------------------------------ GPU: helpers
def device_volume(bs=(0, 1), weights=1, color=True):
    """The common scene's batch elements bs as a TSDFVolume whose state is the hand-made one."""
    vol = gs.TSDFVolume(DIMS, V, origin=[ORIGINS[b] for b in bs], trunc=TRUNC, color=color, device=DEV)
    hv = [host_volume(b, weights) for b in bs]
    vol.tsdf = torch.from_numpy(np.stack([h["tsdf"] for h in hv])).to(DEV)
    vol.weight = torch.from_numpy(np.stack([h["weight"] for h in hv])).to(DEV)
    if color:
        vol.color = torch.from_numpy(np.stack([h["color"] for h in hv])).to(DEV)
    return vol


def cameras(B, names):
    K = torch.from_numpy(make_K()).view(1, 1, 4, 4).repeat(B, 1, 1, 1).to(DEV)
    poses = torch.from_numpy(np.stack([POSES[n] for n in names])).view(1, len(names), 4, 4).repeat(B, 1, 1, 1).to(DEV)
    return K, poses


def raw(vol, K, poses, **kw):
    kw.setdefault("stride", 1)
    kw.setdefault("step", STEPS[0])
    return ops.tsdf_raycast_raw(vol.tsdf, vol.weight, vol.color, vol.origin, V, K, poses, H, W, **kw)


def images(out, b, l):
    return tuple(None if x is None else x[b, l].cpu().numpy() for x in out)


# ------------------------------------------------------------------ GPU 1: the forward against the float64 reference
@pytest.mark.gpu
@pytest.mark.parametrize("step", STEPS)
def test_cast_matches_the_float64_reference(step):
    """Both batch elements and the four cameras in one call.  Measured on the MI355X (largest deviation over the 16 images of
    the two steps): depth 6.5e-07 m, normal 5.9e-07, colour 4.7e-07 (the float32 transcription's figures, digit for digit); 0 to 24 of
    3072 pixels left out per image."""
    names = list(POSES)
    vol = device_volume()
    K, poses = cameras(2, names)
    out = raw(vol, K, poses, step=step)
    assert out[0].shape == (2, 4, H, W) and out[1].shape == (2, 4, H, W, 3) and out[2].shape == (2, 4, H, W, 3)
    assert out[3].shape == (2, 4, H, W) and out[3].dtype == torch.int32
    worst = np.zeros(3)
    for b in range(2):
        for l, name in enumerate(names):
            worst = np.maximum(worst, compare(images(out, b, l), reference(b, name, step), "b=%d %s step=%g" % (b, name, step)))
    print("step", step, "largest deviations", worst)


# ------------------------------------------------------------------ GPU 2: strides, min_weight, near / far, batches, no colours
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 4, 5])
def test_cast_on_the_strided_grid(stride):
    """48 and 64 are no multiples of 5; stride 4 gives 12 x 16 pixels, less than one 16 x 16 block in height."""
    vol = device_volume(bs=(0,))
    K, poses = cameras(1, ["rotated", "outside"])
    out = raw(vol, K, poses, stride=stride)
    Ho, Wo = -(-H // stride), -(-W // stride)
    assert out[0].shape == (1, 2, Ho, Wo)
    for l, name in enumerate(("rotated", "outside")):
        ref = reference(0, name, STEPS[0], stride=stride)
        compare(images(out, 0, l), ref, "stride %d %s" % (stride, name))
        full = reference(0, name, STEPS[0])
        assert np.array_equal(ref["k_end"], full["k_end"][::stride, ::stride])  # the [::s, ::s] grid of downsample_rgbdimages


@pytest.mark.gpu
@pytest.mark.parametrize("minw", [1.0, 2.0])
def test_cast_with_min_weight(minw):
    vol = device_volume(bs=(0,), weights=2)
    K, poses = cameras(1, ["rotated"])
    out = raw(vol, K, poses, min_weight=minw)
    ref = reference(0, "rotated", STEPS[0], minw=minw, weights=2)
    compare(images(out, 0, 0), ref, "min_weight %g" % minw)
    n1 = int((reference(0, "rotated", STEPS[0], minw=1.0, weights=2)["k_end"] > 0).sum())
    assert (minw == 1.0) == (int((ref["k_end"] > 0).sum()) == n1) and int((ref["k_end"] > 0).sum()) > 300  # 2 sees the half with y < 0


@pytest.mark.gpu
def test_cast_between_near_and_far():
    """near behind the sphere's front: its rays start inside or behind it; far in front of the plane: the rays that pass the
    sphere never end."""
    vol = device_volume(bs=(0,))
    K, poses = cameras(1, ["identity"])
    full = reference(0, "identity", STEPS[0])
    for near, far in ((1.0, np.inf), (0.0, 1.5), (0.9, 1.2)):
        ref = reference(0, "identity", STEPS[0], near=near, far=far)
        compare(images(raw(vol, K, poses, near=near, far=far), 0, 0), ref, "near %g far %g" % (near, far))
        hit = ref["k_end"] > 0
        assert 50 < hit.sum() < (full["k_end"] > 0).sum() - 50
        assert (ref["depth"][hit] >= near).all() and (ref["depth"][hit] <= far).all()


@pytest.mark.gpu
def test_batches_and_frames_in_one_call_equal_single_calls_bitwise():
    vol = device_volume()
    K, poses = cameras(2, ["rotated", "outside"])
    poses[1, :, :3, 3] += 0.01  # four different cameras
    out = raw(vol, K, poses)
    for b in range(2):
        one = device_volume(bs=(b,))
        for l in range(2):
            single = raw(one, K[b:b + 1], poses[b:b + 1, l:l + 1].contiguous())
            for x, y in zip(out, single):
                assert torch.equal(x[b, l], y[0, 0]), (b, l)
    assert not torch.equal(out[0][0, 0], out[0][1, 0])


@pytest.mark.gpu
def test_volume_without_colours():
    vol = device_volume(bs=(0,), color=False)
    K, poses = cameras(1, ["rotated"])
    out = raw(vol, K, poses)
    assert out[2] is None
    compare(images(out, 0, 0), reference(0, "rotated", STEPS[0]), "no colours")
    frames, normals = vol.raycast(K, poses, H, W, step=STEPS[0], return_normals=True)
    assert torch.equal(frames.depth_image[..., 0], out[0]) and torch.equal(normals, out[1])
    assert frames.rgb_image.shape == (1, 1, H, W, 3) and not frames.rgb_image.any()
    pc = vol.raycast_pointcloud(K, poses, H, W)
    assert pc.has_normals and not pc.has_colors and pc.num_points_per_pointcloud.tolist() == [int((out[3] > 0).sum())]


# ------------------------------------------------------------------ GPU 3: tiny volumes
def tiny_host_volume(dims):
    """A tilted plane through a volume of half-metre voxels in front of the identity camera, as the reference's dict."""
    v, trunc = 0.5, 1.0
    origin = (-0.5 * dims[0] * v + 0.013, -0.5 * dims[1] * v - 0.021, 1.0)
    nx, ny, nz = dims
    ax = [origin[k] + (np.arange(n) + 0.5) * v for k, n in enumerate(dims)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    tsdf = np.clip((origin[2] + 0.55 * nz * v + 0.2 * x - 0.1 * y - z) / trunc, -1, 1).astype(F32)
    color = np.stack([0.5 + 0.3 * x, 0.5 - 0.3 * y, 0.1 * z], -1).astype(F32)
    return dict(tsdf=tsdf, weight=np.ones_like(tsdf), color=color, origin=origin, v=v, dims=dims)


def tiny_volume(dims):
    """-> (the reference's dict, the TSDFVolume that holds the same state)."""
    hv = tiny_host_volume(dims)
    vol = gs.TSDFVolume(dims, hv["v"], origin=[hv["origin"]], trunc=1.0, device=DEV)
    vol.tsdf, vol.weight, vol.color = (torch.from_numpy(hv[k][None].copy()).to(DEV) for k in ("tsdf", "weight", "color"))
    return hv, vol


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 2, 2), (1, 1, 1), (5, 1, 1)])
def test_tiny_volumes(dims):
    """One cell, two cells, none: with a single voxel along an axis no position has 8 corners, every pixel is a miss and no
    voxel is read (the tensors hold exactly the volume: the first read beyond it is outside the allocation's data)."""
    hv, vol = tiny_volume(dims)
    v = hv["v"]
    K, poses = cameras(1, ["identity"])
    out = ops.tsdf_raycast_raw(vol.tsdf, vol.weight, vol.color, vol.origin, v, K, poses, H, W, 1, 0.25)
    ref = ref_cast(hv, make_K(), POSES["identity"], H, W, 1, 0.25)
    compare(images(out, 0, 0), ref, "dims %s" % (dims,))
    hits = int((ref["k_end"] > 0).sum())
    assert (hits > 20) if min(dims) > 1 else (hits == 0 and not out[3].any() and not out[0].any())
    g_t, g_c = ops.tsdf_raycast_backward_raw(vol.tsdf, vol.weight, vol.color, vol.origin, v, K, poses, H, W, 1, 0.25, 1.0, out[3],
                                             torch.ones_like(out[0]), torch.ones_like(out[2]))
    assert torch.isfinite(g_t).all() and torch.isfinite(g_c).all() and bool(g_t.any()) == (hits > 0)


# ------------------------------------------------------------------ GPU 4: consistency with the rest of the library
@lru_cache(maxsize=None)
def wall():
    colors, depths, K, poses = (t.to(DEV) for t in make_sequence(1, 4, H, W, seed=0))
    vol = gs.TSDFVolume(DIMS, V, origin=[ORIGINS[0]], trunc=TRUNC, device=DEV).integrate(gs.RGBDImages(colors, depths, K, poses))
    return vol, colors, depths, K, poses


@pytest.mark.gpu
def test_cast_of_an_integrated_wall_agrees_with_the_frames():
    vol, colors, depths, K, poses = wall()
    frames, normals = vol.raycast(K, poses[:, :1], H, W, return_normals=True)
    cast, given = frames.depth_image[0, 0, :, :, 0].cpu().numpy(), depths[0, 0, :, :, 0].cpu().numpy()
    both = (cast > 0) & (given > 0)
    # not at a depth edge: the 3 x 3 neighbourhood is valid and within v of the pixel
    pad = np.pad(given, 1, mode="edge")
    nb = np.stack([pad[1 + dy: 1 + dy + H, 1 + dx: 1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    smooth = (nb > 0).all(0) & (np.abs(nb - given).max(0) < V)
    sel = both & smooth
    print("pixels compared", int(sel.sum()), "of", H * W, "largest |cast - input|", float(np.abs(cast - given)[sel].max()))
    assert sel.sum() > 500  # (the volume holds 60 % of the image's rows; 5 % of the pixels are dropped, with them their neighbourhoods)
    assert np.abs(cast - given)[sel].max() <= V
    # the normals look at the camera
    _, dw, _ = ref_rays(K[0, 0].cpu().numpy(), poses[0, 0].cpu().numpy(), H, W, 1, TRUNC / 2)
    n = normals[0, 0].cpu().numpy()
    assert ((n * -dw).sum(-1)[cast > 0] > 0).all()
    assert np.allclose(np.linalg.norm(n[cast > 0], axis=-1), 1.0, atol=1e-5)
    assert (frames.rgb_image[0, 0].cpu().numpy()[cast > 0].max(-1) > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 4])
def test_raycast_pointcloud_is_the_vertex_map_at_the_hits(stride):
    vol, colors, depths, K, poses = wall()
    frames, normals = vol.raycast(K, poses[:, :1], H, W, stride=stride, return_normals=True)
    pc = vol.raycast_pointcloud(K, poses[:, :1], H, W, stride=stride)
    hit = (frames.depth_image[0, 0, :, :, 0] > 0)
    assert pc.num_points_per_pointcloud.tolist() == [int(hit.sum())] and int(hit.sum()) > 50
    gv = frames.global_vertex_map[0, 0][hit].cpu().numpy()
    p = pc.points_list[0].cpu().numpy()
    assert (np.abs(p - gv) <= 4 * np.spacing(np.abs(gv))).all()  # pixel order, 4 ulp of the coordinates
    assert torch.equal(pc.normals_list[0], normals[0, 0][hit]) and torch.equal(pc.colors_list[0], frames.rgb_image[0, 0][hit])
    # the points are t + z* dw of the full-resolution pixels (i s, j s): the strided intrinsics describe the same rays
    t, dw, _ = ref_rays(K[0, 0].cpu().numpy(), poses[0, 0].cpu().numpy(), H, W, stride, TRUNC / 2)
    z = frames.depth_image[0, 0, :, :, 0].cpu().numpy().astype(np.float64)
    want = (t.astype(np.float64) + z[..., None] * dw.astype(np.float64))[hit.cpu().numpy()]
    assert np.abs(p - want).max() < 2e-6
    Ks = frames.intrinsics[0, 0].cpu().numpy()
    assert np.allclose([Ks[0, 0], Ks[1, 1], Ks[0, 2], Ks[1, 2]], np.array([K[0, 0, 0, 0].item(), K[0, 0, 1, 1].item(), K[0, 0, 0, 2].item(),
                                                                         K[0, 0, 1, 2].item()]) / stride)


# ------------------------------------------------------------------ GPU 5: the reverse pass
def gradient_records(b, name, stride):
    """The float32 transcription's records of one image with the tying pixels taken out, and the tape that goes with them."""
    r64, r32 = reference(b, name, STEPS[0], stride=stride), reference(b, name, STEPS[0], stride=stride, dt=np.float32)
    good = ~r64["tie"]
    assert np.array_equal(r64["k_end"][good], r32["k_end"][good])
    rec = dict(r32["rec"], hit=r32["rec"]["hit"] & good.reshape(-1))
    return rec, np.where(good, r32["k_end"], 0)


def check_gradient(got, want, A, what):
    """|got - want| <= 32 * 2^-24 * A per element; what no term touches (A = 0) receives exactly nothing."""
    assert (got[A == 0] == 0).all(), what
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / (U * A)
    print(what, "largest error in units of 2^-24 A: %.3g (elements with terms: %d, largest |g| %.3g)" % (np.nanmax(r), (A > 0).sum(),
                                                                                                      np.abs(want).max()))
    assert np.nanmax(r) <= 32, what


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 4])
def test_cast_gradients_match_the_explicit_formulas_and_repeat_bitwise(stride):
    """The tape is the reference's with the tying pixels taken out (the forward tests pin the device's tape to it).  Measured on
    the MI355X: the largest |device - float64| / (2^-24 A) is 4.5 for g_tsdf (4.9 with g_depth alone) and 2.6 for g_color (the bound: 32)."""
    names = ["rotated", "outside"]
    vol = device_volume()
    K, poses = cameras(2, names)
    recs = [[gradient_records(b, n, stride) for n in names] for b in range(2)]
    tape = np.stack([np.stack([t for _, t in row]) for row in recs]).astype(np.int32)
    Ho, Wo = tape.shape[2:]
    rng = np.random.RandomState(3)
    gd, gc = rng.randn(2, 2, Ho, Wo).astype(F32), rng.randn(2, 2, Ho, Wo, 3).astype(F32)
    assert (tape > 0).sum() > 5000 // stride ** 2
    dev = lambda x: torch.from_numpy(x).to(DEV)
    args = (vol.tsdf, vol.weight, vol.color, vol.origin, V, K, poses, H, W, stride, STEPS[0], 1.0, dev(tape), dev(gd), dev(gc))
    g_t, g_c = ops.tsdf_raycast_backward_raw(*args)
    again = ops.tsdf_raycast_backward_raw(*args)
    assert torch.equal(g_t, again[0]) and torch.equal(g_c, again[1])
    assert g_t.shape == vol.tsdf.shape and g_c.shape == vol.color.shape
    # g_depth alone, into a volume without colours: the same formulas
    g_t0, none = ops.tsdf_raycast_backward_raw(vol.tsdf, vol.weight, None, vol.origin, V, K, poses, H, W, stride, STEPS[0], 1.0, dev(tape),
                                               dev(gd), None)
    assert none is None
    for b in range(2):
        hv, bare = host_volume(b), dict(host_volume(b), color=None)
        want_t, want_c, A_t, A_c, want_0, A_0 = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
        for l in range(2):
            rec = recs[b][l][0]
            t, c = ref_cast_backward(hv, rec, gd[b, l], gc[b, l])
            a_t, a_c = ref_cast_backward(hv, rec, gd[b, l], gc[b, l], absolute=True)
            want_t, want_c, A_t, A_c = want_t + t, want_c + c, A_t + a_t, A_c + a_c
            want_0, A_0 = want_0 + ref_cast_backward(bare, rec, gd[b, l], None)[0], A_0 + ref_cast_backward(bare, rec, gd[b, l], None, True)[0]
        assert (A_t > 0).sum() > 1000 // stride ** 2 and (A_t == 0).sum() > 30000  # misses, and most of the volume, receive nothing
        flat = lambda x, c: x[b].cpu().numpy().reshape((-1,) + c).astype(np.float64)
        check_gradient(flat(g_t, ()), want_t, A_t, "b %d stride %d g_tsdf" % (b, stride))
        check_gradient(flat(g_c, (3,)), want_c, A_c, "b %d stride %d g_color" % (b, stride))
        check_gradient(flat(g_t0, ()), want_0, A_0, "b %d stride %d g_tsdf of g_depth alone" % (b, stride))


def cast_terms_f32(hv, rec, p, gd, gc):
    """The terms of hit pixel p in float32 in the kernel's order: -> [(voxel, channel (0: tsdf, 1..3: colour), term)]."""
    dims, v = hv["dims"], F32(hv["v"])
    f0, f1, dz, dw = F32(rec["f0"][p]), F32(rec["f1"][p]), F32(rec["dz"][p]), rec["dw"][p].astype(F32)
    a0, a1, ah = (rec[k][p: p + 1].astype(F32) for k in ("a0", "a1", "ah"))
    ids0, ids1, idsh = (corner_ids(rec[k][p], dims) for k in ("i0", "i1", "ih"))
    col = hv["color"].reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        gz = F32(gd)
        for ch in range(3):
            g = trigrad(col[:, ch][idsh][None], ah)[0]
            gz = gz + F32(gc[ch]) * (((g[0] * dw[0] + g[1] * dw[1]) + g[2] * dw[2]) / v)
        den = f0 - f1
        den2, gs_ = den * den, gz * dz
        t0, t1 = gs_ * ((-f1) / den2), gs_ * (f0 / den2)
        w0, w1, wh = corner_w(a0)[0], corner_w(a1)[0], corner_w(ah)[0]
        out = [(int(ids0[c]), 0, t0 * w0[c]) for c in range(8)] + [(int(ids1[c]), 0, t1 * w1[c]) for c in range(8)]
        out += [(int(idsh[c]), 1 + ch, F32(gc[ch]) * wh[c]) for c in range(8) for ch in range(3)]
    assert all(t.dtype == F32 for _, _, t in out)
    return out


@pytest.mark.gpu
def test_cast_reverse_with_non_finite_upstream_entries():
    """g_depth = +inf at one hit pixel and g_rgb = NaN (one channel) at another, on the 12 x 16 grid of the stride-4 camera over
    a (5, 4, 3) volume.  A voxel sum that receives a non-finite term holds what a float sum of its terms gives (the terms formed
    in float32 in the kernel's order: inf times a zero weight is NaN); every other element of g_tsdf and g_color holds the bits of
    the same call with the two entries set to zero."""
    dims, stride, step = (5, 4, 3), 4, 0.25
    hv, vol = tiny_volume(dims)
    K, poses = cameras(1, ["identity"])
    r64 = ref_cast(hv, make_K(), POSES["identity"], H, W, stride, step)
    r32 = ref_cast(hv, make_K(), POSES["identity"], H, W, stride, step, dt=np.float32)
    good = ~r64["tie"] & (r64["k_end"] > 0)
    assert np.array_equal(r64["k_end"][good], r32["k_end"][good])
    tape = np.where(good, r32["k_end"], 0).astype(np.int32)
    Ho, Wo = tape.shape
    assert (Ho, Wo) == (12, 16)
    hits = np.nonzero(tape.reshape(-1))[0]
    assert len(hits) > 20
    p_inf, p_nan = int(hits[0]), int(hits[-1])
    rng = np.random.RandomState(6)
    gd, gc = rng.randn(Ho * Wo).astype(F32), rng.randn(Ho * Wo, 3).astype(F32)
    gd_bad, gc_bad, gd_zero, gc_zero = gd.copy(), gc.copy(), gd.copy(), gc.copy()
    gd_bad[p_inf], gc_bad[p_nan, 1], gd_zero[p_inf], gc_zero[p_nan, 1] = np.inf, np.nan, 0.0, 0.0
    dev = lambda x, s: torch.from_numpy(x).reshape(s).to(DEV)
    run = lambda d, c: ops.tsdf_raycast_backward_raw(vol.tsdf, vol.weight, vol.color, vol.origin, hv["v"], K, poses, H, W, stride, step, 1.0,
                                                     dev(tape, (1, 1, Ho, Wo)), dev(d, (1, 1, Ho, Wo)), dev(c, (1, 1, Ho, Wo, 3)))
    got, want = run(gd_bad, gc_bad), run(gd_zero, gc_zero)
    nvox = dims[0] * dims[1] * dims[2]
    flat = lambda x: np.concatenate([x[0].reshape(nvox, 1).cpu().numpy(), x[1].reshape(nvox, 3).cpu().numpy()], 1)  # (voxel, channel)
    g, z = flat(got), flat(want)
    terms = {}
    for p in (p_inf, p_nan):
        for j, ch, t in cast_terms_f32(hv, r32["rec"], p, gd_bad[p], gc_bad[p]):
            if not np.isfinite(t):
                terms.setdefault((j, ch), []).append(t)
    hit = np.zeros((nvox, 4), bool)
    for (j, ch), ts in terms.items():
        hit[j, ch] = True
        w, h = exact_sum_f32(ts), g[j, ch]
        assert (np.isnan(w) and np.isnan(h)) or w.view(np.uint32) == h.view(np.uint32), (j, ch, w, h)
    assert 0 < hit.sum() <= 2 * 16 + 8 and np.isposinf(g[hit]).any() and np.isnan(g[hit]).any()
    assert np.array_equal(g.view(np.uint32)[~hit], z.view(np.uint32)[~hit]) and (z != 0).sum() > 50


@pytest.mark.gpu
def test_autograd_node_reaches_tsdf_and_color():
    vol = device_volume(bs=(0,))
    K, poses = cameras(1, ["rotated"])
    vol.tsdf.requires_grad_(True)
    vol.color.requires_grad_(True)
    frames = vol.raycast(K, poses, H, W, stride=2)
    w_d = torch.linspace(0.5, 1.5, (H // 2) * (W // 2), device=DEV).view(1, 1, H // 2, W // 2, 1)
    ((frames.depth_image * w_d).sum() + 0.5 * frames.rgb_image.sum()).backward()
    depth, normal, rgb, k_end = ops.tsdf_raycast_raw(vol.tsdf.detach(), vol.weight, vol.color.detach(), vol.origin, V, K, poses, H, W, 2,
                                                     STEPS[0])
    assert torch.equal(frames.depth_image[..., 0], depth) and torch.equal(frames.rgb_image, rgb)
    g_t, g_c = ops.tsdf_raycast_backward_raw(vol.tsdf.detach(), vol.weight, vol.color.detach(), vol.origin, V, K, poses, H, W, 2, STEPS[0],
                                             1.0, k_end, w_d[..., 0].contiguous(), torch.full_like(rgb, 0.5))
    assert torch.equal(vol.tsdf.grad, g_t) and torch.equal(vol.color.grad, g_c) and int((g_t != 0).sum()) > 500


# ------------------------------------------------------------------ GPU 6: end to end
@pytest.mark.gpu
def test_end_to_end_chamfer_loss_reaches_depth_and_rgb_through_the_cast():
    """chamfer_distance differentiates the points only: it reaches the depth images through integrate and the cast's depth;
    the rgb images are reached through the cast's colours, by a colour term.  chamfer_distance's own reverse pass adds with
    float atomics unless torch.use_deterministic_algorithms is on, so the bits are compared under the flag."""
    colors, depths, K, poses = (t.to(DEV) for t in make_sequence(1, 3, H, W, seed=0))
    target = pointclouds_from_rgbdimages(gs.RGBDImages(colors[:, :1], depths[:, :1], K, poses[:, :1]))

    def run():
        d, c = depths.clone().requires_grad_(True), colors.clone().requires_grad_(True)
        vol = gs.TSDFVolume(DIMS, V, origin=[ORIGINS[0]], trunc=TRUNC, device=DEV).integrate(gs.RGBDImages(c, d, K, poses))
        pc = vol.raycast_pointcloud(K, poses[:, :1], H, W, stride=2)
        loss = chamfer_distance(pc, target)
        (loss + 1e-3 * pc.colors_padded.mean()).backward()
        return loss.detach(), d.grad, c.grad

    torch.use_deterministic_algorithms(True)
    try:
        a, b = run(), run()
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.isfinite(a[0]) and 0.0 < float(a[0]) < 0.05
    for g in a[1:]:
        assert g is not None and torch.isfinite(g).all() and int((g != 0).sum()) > 100
    assert all(torch.equal(x, y) for x, y in zip(a, b))
