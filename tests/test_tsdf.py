"""TSDF volumes (gs_tsdf_integrate / gs_tsdf_extract and their reverse passes, ops.tsdf_*, gs.structures.TSDFVolume).

The references are written here in numpy and torch, not taken from the code under test:
* voxel centres: o + (i + 0.5) * v in numpy float32, the kernels' rule bit for bit;
* integration: the per-frame running average in float64 (ref_integrate); on the GPU the pixel of a voxel comes from
  ops.project_active_raw on those centres (the projection body the integration calls, pinned by its own tests), z and the
  update are float64.  Voxels with a (voxel, frame) pair closer than 1e-5 to a threshold (sdf = -trunc: skip or update;
  sdf = +trunc: gradient or none) are left out: there fp32 and float64 may decide differently;
* extraction: numpy float32 with the operations in the order the header states them (ref_extract): bitwise for the edge ids, the
  points and the colours;
* reverse passes: the explicit formulas of the issue in float64 (ref_integrate_backward, ref_extract_backward), themselves checked
  against torch float64 autograd of the forward references on the CPU.  Run on absolute values they give A, the sum of the
  absolute terms of every element: the device's sums are exact, each term carries about 10 roundings, the bound is 32 * 2^-24 * A.
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
from gradslam_amd.synthetic import make_intrinsics, make_sequence
from tests.helpers import exact_sum_f32

DEV = "cuda:0"
U = 2.0 ** -24
NEW_SYMBOLS = {"gs_tsdf_integrate": 22, "gs_tsdf_integrate_backward_ws_bytes": 4, "gs_tsdf_integrate_backward": 24,
               "gs_tsdf_extract_ws_bytes": 4, "gs_tsdf_extract": 19, "gs_tsdf_extract_backward": 15}

# the common scene
DIMS, V, TRUNC, MAXW = (42, 22, 56), 0.05, 0.15, 2.0
ORIGINS = [(-1.0, -0.55, -0.2), (-0.95, -0.5, -0.15)]
H, W = 48, 64
TIE = 1e-5
SENT_T, SENT_C = 0.75, 7.0  # state of the untouched voxels in the sentinel runs (tsdf is not the fresh 1.0)


# ------------------------------------------------------------------ the references
def ref_centres(dims, v, origin):
    """(nvox, 3) float32, x fastest: c_k = o_k + ((float)i_k + 0.5f) * v, one rounded product and one rounded sum."""
    nx, ny, nz = dims
    o = np.asarray(origin, dtype=np.float32)
    ax = [o[k] + (np.arange(n, dtype=np.float32) + np.float32(0.5)) * np.float32(v) for k, n in enumerate((nx, ny, nz))]
    assert all(a.dtype == np.float32 for a in ax)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3)


def np_project(cent, pose, K, height, width):
    """find_active_map_points' rule in numpy float32 (the CPU tests' stand-in for the device's projection; on the GPU the pixels
    come from ops.project_active_raw): -> (active (n,), pix (n,), z (n,))."""
    pose, K = np.asarray(pose, np.float32), np.asarray(K, np.float32)
    R, t = pose[:3, :3], pose[:3, 3]
    pc = (cent @ R + (-(R.T @ t))).astype(np.float32)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    with np.errstate(all="ignore"):
        qx, qy, qz = K[0, 0] * x + K[0, 2] * z, K[1, 1] * y + K[1, 2] * z, z
        zs = np.where(qz != 0, qz, np.float32(1))
        u, vv = qx / zs, qy / zs
        act = (u > -1e-3) & (u < np.float32(width - 0.999)) & (vv > -1e-3) & (vv < np.float32(height - 0.999)) & (z > 0)
        w = np.clip(np.rint(u), 0, width - 1).astype(np.int64)
        h = np.clip(np.rint(vv), 0, height - 1).astype(np.int64)
    return act, np.where(act, h * width + w, 0), z


def ref_integrate(act, pix, z, depth, rgb, f, w, col, trunc, maxw):
    """One batch element in float64.  act, pix, z: (L, n); depth (L, HW); rgb (L, HW, 3) or None; f, w (n,), col (n, 3) or None.
    -> (f, w, col, rec): rec[l] holds the constants of frame l: upd (the voxel is updated), lin (and sdf < trunc), W (the weight
    before the frame), tie (a threshold closer than TIE)."""
    f, w = f.astype(np.float64).copy(), w.astype(np.float64).copy()
    col = None if col is None else col.astype(np.float64).copy()
    trunc = float(np.float32(trunc))
    rec = []
    for l in range(act.shape[0]):
        d = depth[l][pix[l]].astype(np.float64)
        sdf = d - z[l].astype(np.float64)
        seen = act[l] & (d > 0)
        upd = seen & ~(sdf < -trunc)
        t = np.minimum(1.0, sdf / trunc)
        rec.append(dict(upd=upd, lin=upd & (sdf < trunc), W=w.copy(), seen=seen, sat=upd & ~(sdf < trunc), occ=seen & ~upd,
                        tie=seen & ((np.abs(sdf + trunc) < TIE) | (np.abs(sdf - trunc) < TIE)),
                        tie_skip=seen & (np.abs(sdf + trunc) < TIE)))
        f = np.where(upd, (w * f + t) / (w + 1.0), f)
        if col is not None:
            c = rgb[l][pix[l]].astype(np.float64)
            col = np.where(upd[:, None], (w[:, None] * col + c) / (w[:, None] + 1.0), col)
        w = np.where(upd, np.minimum(w + 1.0, float(maxw)), w)
    return f, w, col, rec


def ref_integrate_backward(rec, pix, g_f, g_col, trunc, npix):
    """The explicit reverse formulas in float64: -> (g_f_in, g_col_in, g_depth (L, npix), g_rgb (L, npix, 3))."""
    trunc = float(np.float32(trunc))
    L = len(rec)
    g = g_f.astype(np.float64).copy()
    gc = None if g_col is None else g_col.astype(np.float64).copy()
    g_depth, g_rgb = np.zeros((L, npix)), np.zeros((L, npix, 3))
    for l in reversed(range(L)):
        upd, lin, Wb = rec[l]["upd"], rec[l]["lin"], rec[l]["W"]
        den = Wb + 1.0
        keep = Wb / den
        np.add.at(g_depth[l], pix[l][lin], (g / den / trunc)[lin])
        g = np.where(upd, g * keep, g)
        if gc is not None:
            np.add.at(g_rgb[l], pix[l][upd], (gc / den[:, None])[upd])
            gc = np.where(upd[:, None], gc * keep[:, None], gc)
    return g, gc, g_depth, g_rgb


def torch_integrate(rec, pix, z, depth, rgb, f, col, trunc):
    """The forward reference again in torch float64 with the decisions of `rec` as constants, for autograd."""
    trunc = float(np.float32(trunc))
    for l in range(len(rec)):
        upd, lin, Wb = (torch.from_numpy(rec[l][k]) for k in ("upd", "lin", "W"))
        p = torch.from_numpy(pix[l])
        sdf = depth[l][p] - torch.from_numpy(z[l].astype(np.float64))
        t = torch.where(lin, sdf / trunc, torch.ones_like(sdf))
        f = torch.where(upd, (Wb * f + t) / (Wb + 1.0), f)
        col = torch.where(upd[:, None], (Wb[:, None] * col + rgb[l][p]) / (Wb[:, None] + 1.0), col)
    return f, col


def ref_diffs(tsdf, obs):
    """D_k(j) for k = x, y, z: (nz, ny, nx, 3) float32 from tsdf (nz, ny, nx) float32 and the observed mask."""
    out = np.zeros(tsdf.shape + (3,), np.float32)
    for k in range(3):
        ax = 2 - k
        fp, fm = np.roll(tsdf, -1, ax), np.roll(tsdf, 1, ax)
        op, om = np.roll(obs, -1, ax), np.roll(obs, 1, ax)
        last, first = [slice(None)] * 3, [slice(None)] * 3
        last[ax], first[ax] = -1, 0
        op[tuple(last)] = False
        om[tuple(first)] = False
        d = np.where(op & om, np.float32(0.5) * (fp - fm), np.where(op, fp - tsdf, np.where(om, tsdf - fm, np.float32(0))))
        assert d.dtype == np.float32
        out[..., k] = d
    return out


def ref_extract(tsdf, weight, color, v, origin, minw):
    """One batch element, numpy float32 as written in the header -> dict(edge, j0, j1, axis, s, points, normals, colors)."""
    nz, ny, nx = tsdf.shape
    v32 = np.float32(v)
    obs = weight >= np.float32(minw)
    jidx = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    e_all, j0_all, j1_all, a_all = [], [], [], []
    for a in range(3):
        s0, s1 = [slice(None)] * 3, [slice(None)] * 3
        s0[2 - a], s1[2 - a] = slice(0, -1), slice(1, None)
        s0, s1 = tuple(s0), tuple(s1)
        f0, f1 = tsdf[s0], tsdf[s1]
        cross = obs[s0] & obs[s1] & ((f0 < 0) != (f1 < 0))
        j0_all.append(jidx[s0][cross])
        j1_all.append(jidx[s1][cross])
        a_all.append(np.full(int(cross.sum()), a))
        e_all.append(3 * jidx[s0][cross] + a)
    e, j0, j1, ax = (np.concatenate(x) for x in (e_all, j0_all, j1_all, a_all))
    order = np.argsort(e, kind="stable")
    e, j0, j1, ax = e[order], j0[order], j1[order], ax[order]
    f = tsdf.reshape(-1)
    f0, f1 = f[j0], f[j1]
    s = f0 / (f0 - f1)
    pts = ref_centres((nx, ny, nz), v, origin)[j0].copy()
    rows = np.arange(len(e))
    pts[rows, ax] = pts[rows, ax] + s * v32
    D = ref_diffs(tsdf, obs).reshape(-1, 3)
    g = D[j0] + s[:, None] * (D[j1] - D[j0])
    nn = np.sqrt((g.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    nn[nn == 0] = 1
    out = dict(edge=e.astype(np.int32), j0=j0, j1=j1, axis=ax, s=s, points=pts, normals=g / nn[:, None], colors=None)
    if color is not None:
        c = color.reshape(-1, 3)
        out["colors"] = c[j0] + s[:, None] * (c[j1] - c[j0])
        assert out["colors"].dtype == np.float32
    assert s.dtype == np.float32 and pts.dtype == np.float32
    return out


def ref_extract_backward(tsdf, color, v, j0, j1, axis, g_points, g_colors, absolute=False):
    """The explicit reverse formulas in float64 -> (g_tsdf (nvox,), g_color (nvox, 3)); absolute=True: the sums of the
    absolute terms."""
    f, c = tsdf.reshape(-1).astype(np.float64), color.reshape(-1, 3).astype(np.float64)
    v = float(np.float32(v))
    f0, f1 = f[j0], f[j1]
    s = f0 / (f0 - f1)
    gp = g_points.astype(np.float64)[np.arange(len(j0)), axis]
    gc = g_colors.astype(np.float64)
    dc = c[j1] - c[j0]
    ab = np.abs if absolute else (lambda x: x)
    g_s = ab(v * gp) + (ab(gc * dc)).sum(1)
    ds0, ds1 = -f1 / (f0 - f1) ** 2, f0 / (f0 - f1) ** 2
    g_tsdf, g_color = np.zeros_like(f), np.zeros_like(c)
    np.add.at(g_tsdf, j0, ab(g_s * ds0))
    np.add.at(g_tsdf, j1, ab(g_s * ds1))
    np.add.at(g_color, j0, ab((1.0 - s)[:, None] * gc))
    np.add.at(g_color, j1, ab(s[:, None] * gc))
    return g_tsdf, g_color


def small_cpu_scene(seed=0):
    """A 3-frame 24x32 sequence and a (7, 5, 9) volume around the wall, with the numpy projection: everything ref_integrate takes."""
    colors, depths, K, poses = make_sequence(1, 3, 24, 32, seed=seed)
    dims, v, origin = (7, 5, 9), 0.05, (0.25, -0.1, 1.8)  # (beside the band of invalid depth columns)
    cent = ref_centres(dims, v, origin)
    proj = [np_project(cent, poses[0, l].numpy(), K[0, 0].numpy(), 24, 32) for l in range(3)]
    act, pix, z = (np.stack([p[k] for p in proj]) for k in range(3))
    return dict(dims=dims, v=v, origin=origin, act=act, pix=pix, z=z, depth=depths[0].reshape(3, -1).numpy(),
                rgb=colors[0].reshape(3, -1, 3).numpy(), n=len(cent))


# ------------------------------------------------------------------ CPU: ABI, error contracts, the references themselves
def test_tsdf_symbols_load_and_are_declared():
    lib = nv.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
        assert name + "(" in header, name
        decl = header[header.index(name + "("):]
        assert decl[: decl.index(";")].count(",") + 1 == nargs, name
    assert lib.gs_abi_version() == 3
    assert hasattr(ops, "_TsdfIntegrateFn") and hasattr(ops, "_TsdfExtractFn") and gs.structures.TSDFVolume is gs.TSDFVolume


def test_tsdf_c_entry_points_refuse_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    lib = nv.lib()
    P = 4096
    ok = [P, P, P, P, 1, 2, 8, 8, 4, 4, 4, 0.1, P, 0.3, 8.0, P, P, P, P, P, P, None]
    for pos in (0, 2, 3, 12, 15, 16, 18, 19, 1, 17, 20):  # (the last three: colours go together)
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_integrate(*args) == -1, pos
    for pos, bad in ((4, 0), (4, 65536), (5, 0), (6, 0), (7, -1), (8, 0), (9, -3), (10, 0), (8, 1 << 30), (11, 0.0), (11, float("nan")),
                     (11, float("inf")), (13, 0.0), (13, float("inf")), (14, -1.0), (14, float("nan"))):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_integrate(*args) == -1, (pos, bad)
    args = list(ok)
    args[8], args[9], args[10] = 1024, 1024, 513  # nx ny nz > 2^29
    assert lib.gs_tsdf_integrate(*args) == -1
    assert b"gs_tsdf_integrate" in lib.gs_last_error()

    assert lib.gs_tsdf_extract_ws_bytes(2, 42, 22, 56) == 2 * (-(-(4 * 2 * -(-(3 * 42 * 22 * 56) // 1024)) // 256) * 256)
    assert lib.gs_tsdf_extract_ws_bytes(0, 4, 4, 4) == 0 and lib.gs_tsdf_extract_ws_bytes(1, 1024, 1024, 513) == 0
    ok = [P, P, P, 1, 4, 4, 4, 0.1, P, 1.0, 8, P, P, P, P, P, P, 1 << 20, None]
    for pos in (0, 1, 8, 15, 11, 12, 14):
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_extract(*args) == -1, pos
    for pos, bad in ((3, 0), (4, 0), (7, -1.0), (9, float("nan")), (10, -1)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_extract(*args) == -1, (pos, bad)
    args = list(ok)
    args[16], args[17] = None, 0
    assert lib.gs_tsdf_extract(*args) == -2
    args = list(ok)
    args[17] = lib.gs_tsdf_extract_ws_bytes(1, 4, 4, 4) - 1
    assert lib.gs_tsdf_extract(*args) == -2

    npix = 2 * 3 * 8 * 8
    assert lib.gs_tsdf_integrate_backward_ws_bytes(2, 3, 8, 8) == 256 + 4 * npix + 64 * npix
    assert lib.gs_tsdf_integrate_backward_ws_bytes(1, 40, 8, 8) == 256 + 68 * 32 * 64  # at most one chunk of 32 frames
    ok = [P, P, P, 1, 2, 8, 8, 4, 4, 4, 0.1, P, 0.3, 8.0, P, P, P, P, P, P, P, P, 1 << 20, None]
    for pos in (0, 1, 2, 11, 14, 15, 17, 19, 16, 18, 20):
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_integrate_backward(*args) == -1, pos
    args = list(ok)
    args[22] = lib.gs_tsdf_integrate_backward_ws_bytes(1, 2, 8, 8) - 1
    assert lib.gs_tsdf_integrate_backward(*args) == -2
    ok = [P, P, 1, 4, 4, 4, 0.1, P, P, 8, P, P, P, P, None]
    for pos in (0, 7, 8, 12):
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_extract_backward(*args) == -1, pos
    for pos, bad in ((2, 0), (3, 0), (6, 0.0), (9, 0)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_extract_backward(*args) == -1, (pos, bad)
    assert b"gs_tsdf_extract_backward" in lib.gs_last_error()


def test_tsdf_python_error_contracts():
    T = gs.structures.TSDFVolume
    for bad in ((0, 4, 4), (4, 4), (4, 4, -1), (4.0, 4, 4), "abc", 7, (1024, 1024, 513)):
        with pytest.raises(ValueError, match="dims|voxels"):
            T(bad, 0.1)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-60, "x", None):
        with pytest.raises(ValueError, match="voxel_size"):
            T((4, 4, 4), bad)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="trunc"):
            T((4, 4, 4), 0.1, trunc=bad)
        with pytest.raises(ValueError, match="max_weight"):
            T((4, 4, 4), 0.1, max_weight=bad)
    for bad in ((0.0, float("nan"), 0.0), (0.0, 0.0), [[0.0, 0.0, float("inf")]], "origin"):
        with pytest.raises(ValueError, match="origin"):
            T((4, 4, 4), 0.1, origin=bad)
    with pytest.raises(ValueError, match="batch_size"):
        T((4, 4, 4), 0.1, batch_size=0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        T((4, 4, 4), 0.1, device="cpu")
    # the ops refuse CPU tensors and bad shapes before anything is launched
    t, w, c = torch.ones(1, 4, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4, 3)
    colors, depths, K, poses = make_sequence(1, 2, 8, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_integrate_raw(depths, colors, K, poses, t, w, c, (0.0, 0.0, 0.0), 0.1, 0.4, 8.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_integrate(depths, colors, K, poses, t, w, c, (0.0, 0.0, 0.0), 0.1, 0.4, 8.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_extract_raw(t, w, c, (0.0, 0.0, 0.0), 0.1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_extract(t, w, c, (0.0, 0.0, 0.0), 0.1, cap=4)
    with pytest.raises(ValueError, match="cap"):
        ops.tsdf_extract(t, w, c, (0.0, 0.0, 0.0), 0.1, cap=0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_extract_backward_raw(t, c, 0.1, torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="tensor"):
        ops.tsdf_extract_raw([1.0], w, c, (0.0, 0.0, 0.0), 0.1)
    with pytest.raises(ValueError, match="poses"):
        ops.tsdf_integrate_raw(depths, colors, K, None, t, w, c, (0.0, 0.0, 0.0), 0.1, 0.4, 8.0)
    # TSDFVolume.integrate checks its frames before it looks at any tensor: an unconstructed volume is enough
    vol = object.__new__(T)
    vol._B = 2
    with pytest.raises(TypeError, match="RGBDImages"):
        T.integrate(vol, depths)
    with pytest.raises(ValueError, match="poses"):
        T.integrate(vol, gs.RGBDImages(colors, depths, K))
    with pytest.raises(ValueError, match="Batch size"):
        T.integrate(vol, gs.RGBDImages(colors, depths, K, poses))


def test_reference_integrator_against_the_closed_form_of_a_plane():
    """A fronto-parallel plane at z = 1 seen with the identity pose: every voxel not more than trunc behind it holds
    clamp((z_plane - z_c) / trunc), whatever the number of frames; the others are untouched."""
    hh, ww, z_plane, v, trunc = 24, 32, 1.0, 0.05, 0.15
    dims, origin = (6, 5, 12), (-0.15, -0.125, 0.6)
    cent = ref_centres(dims, v, origin)
    assert cent.dtype == np.float32 and cent.shape == (360, 3)
    np.testing.assert_array_equal(cent[0], np.float32(origin) + np.float32(0.5) * np.float32(v))
    np.testing.assert_array_equal(cent[1] - cent[0] > 0, [True, False, False])  # x fastest
    act, pix, z = np_project(cent, np.eye(4), make_intrinsics(hh, ww)[0, 0].numpy(), hh, ww)
    assert act.all() and np.array_equal(z, cent[:, 2])
    L = 3
    depth = np.full((L, hh * ww), z_plane, np.float32)
    rgb = np.full((L, hh * ww, 3), 100.0, np.float32)
    f, w, col, rec = ref_integrate(np.stack([act] * L), np.stack([pix] * L), np.stack([z] * L), depth, rgb, np.ones(360), np.zeros(360),
                                   np.zeros((360, 3)), trunc, 2.0)
    sdf = z_plane - cent[:, 2].astype(np.float64)
    t32 = float(np.float32(trunc))
    seen = ~(sdf < -t32)
    assert 0 < seen.sum() < 360 and (sdf > t32).any()
    np.testing.assert_allclose(f, np.where(seen, np.clip(sdf / t32, None, 1.0), 1.0), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(w, np.where(seen, 2.0, 0.0))  # three updates, capped at max_weight = 2
    np.testing.assert_allclose(col, np.where(seen[:, None], 100.0, 0.0) * np.ones(3), rtol=0, atol=1e-12)
    assert all(np.array_equal(r["W"], np.where(seen, min(l, 2), 0.0)) for l, r in enumerate(rec))


def test_reverse_formulas_against_float64_autograd():
    sc = small_cpu_scene()
    rng = np.random.RandomState(3)
    n = sc["n"]
    f0, w0, c0 = rng.uniform(-1, 1, n), rng.randint(0, 3, n).astype(np.float64), rng.uniform(0, 255, (n, 3))
    _, _, _, rec = ref_integrate(sc["act"], sc["pix"], sc["z"], sc["depth"], sc["rgb"], f0, w0, c0, 0.15, 2.0)
    assert sum(int(r["lin"].sum()) for r in rec) > 50 and sum(int(r["sat"].sum()) for r in rec) > 0
    assert any((r["W"][r["upd"]] == 2).any() for r in rec) and any((r["W"][r["upd"]] == 0).any() for r in rec)
    depth, rgb = (torch.tensor(sc[k], dtype=torch.float64, requires_grad=True) for k in ("depth", "rgb"))
    f, c = torch.tensor(f0, requires_grad=True), torch.tensor(c0, requires_grad=True)
    out_f, out_c = torch_integrate(rec, sc["pix"], sc["z"], depth, rgb, f, c, 0.15)
    want_f, _, want_c, _ = ref_integrate(sc["act"], sc["pix"], sc["z"], sc["depth"], sc["rgb"], f0, w0, c0, 0.15, 2.0)
    np.testing.assert_allclose(out_f.detach().numpy(), want_f, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out_c.detach().numpy(), want_c, rtol=0, atol=1e-10)
    g_f, g_c = rng.randn(n), rng.randn(n, 3)
    (out_f * torch.from_numpy(g_f)).sum().add((out_c * torch.from_numpy(g_c)).sum()).backward()
    got = ref_integrate_backward(rec, sc["pix"], g_f, g_c, 0.15, sc["depth"].shape[1])
    for name, a, b in zip(("tsdf", "color", "depth", "rgb"), got, (f.grad, c.grad, depth.grad, rgb.grad)):
        np.testing.assert_allclose(a, b.numpy(), rtol=1e-12, atol=1e-14, err_msg=name)
        assert np.abs(a).max() > 0, name

    # the extraction's formulas, on the state this integration leaves
    nx, ny, nz = sc["dims"]
    tsdf, weight = want_f.astype(np.float32).reshape(nz, ny, nx), np.ones((nz, ny, nx), np.float32)
    color = want_c.astype(np.float32).reshape(nz, ny, nx, 3)
    ref = ref_extract(tsdf, weight, color, sc["v"], sc["origin"], 1.0)
    m = len(ref["edge"])
    assert m > 20 and len(set(ref["axis"])) == 3
    ft, ct = torch.tensor(tsdf.reshape(-1), dtype=torch.float64, requires_grad=True), torch.tensor(color.reshape(-1, 3), dtype=torch.float64,
                                                                                                    requires_grad=True)
    j0, j1 = torch.from_numpy(ref["j0"]), torch.from_numpy(ref["j1"])
    s = ft[j0] / (ft[j0] - ft[j1])
    base = torch.from_numpy(ref_centres(sc["dims"], sc["v"], sc["origin"]).astype(np.float64))[j0]
    onehot = torch.nn.functional.one_hot(torch.from_numpy(ref["axis"]), 3).double()
    pts = base + onehot * (s * float(np.float32(sc["v"])))[:, None]
    cols = ct[j0] + s[:, None] * (ct[j1] - ct[j0])
    np.testing.assert_allclose(pts.detach().numpy(), ref["points"], rtol=0, atol=1e-6)
    g_p, g_c = rng.randn(m, 3), rng.randn(m, 3)
    ((pts * torch.from_numpy(g_p)).sum() + (cols * torch.from_numpy(g_c)).sum()).backward()
    got_t, got_c = ref_extract_backward(tsdf, color, sc["v"], ref["j0"], ref["j1"], ref["axis"], g_p, g_c)
    np.testing.assert_allclose(got_t, ft.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got_c, ct.grad.numpy(), rtol=1e-12, atol=1e-12)
    A_t, A_c = ref_extract_backward(tsdf, color, sc["v"], ref["j0"], ref["j1"], ref["axis"], g_p, g_c, absolute=True)
    assert (A_t >= np.abs(got_t) * (1 - 1e-12)).all() and (A_c >= np.abs(got_c) * (1 - 1e-12)).all()


def test_extraction_reference_on_a_hand_made_volume():
    """3 x 2 x 2 voxels: the crossings, f0 == 0 (outside: no crossing with a positive neighbour, a crossing at s = 1 with a
    negative one) and an unobserved end."""
    nx, ny, nz = 3, 2, 2
    tsdf = np.full((nz, ny, nx), 0.5, np.float32)
    weight = np.ones((nz, ny, nx), np.float32)
    tsdf[0, 0, 1] = -0.5
    tsdf[1, 1, 0] = -0.25
    tsdf[1, 1, 2] = 0.0
    tsdf[1, 0, 2] = -0.5
    weight[0, 1, 0] = 0.0  # below (0,1,1) = -0.25: that z edge would cross
    color = np.zeros((nz, ny, nx, 3), np.float32)
    color[..., 0] = np.arange(12, dtype=np.float32).reshape(nz, ny, nx)
    ref = ref_extract(tsdf, weight, color, 0.5, (0.0, 0.0, 0.0), 1.0)
    assert ref["edge"].tolist() == [0, 3, 4, 5, 8, 19, 21, 25, 27]
    np.testing.assert_array_equal(ref["s"], np.float32([0.5, 0.5, 0.5, 0.5, 0.5, np.float32(0.5) / np.float32(0.75), 0.5, 1.0,
                                                        np.float32(-0.25) / np.float32(-0.75)]))
    np.testing.assert_array_equal(ref["points"][0], np.float32([0.5, 0.25, 0.25]))    # x edge from voxel (0,0,0), s = 0.5
    np.testing.assert_array_equal(ref["points"][3], np.float32([0.75, 0.25, 0.5]))    # z edge from voxel (1,0,0)
    np.testing.assert_array_equal(ref["points"][7], np.float32([1.25, 0.75, 0.75]))   # y edge (2,0,1) -> (2,1,1): at the zero voxel's centre
    np.testing.assert_array_equal(ref["colors"][0], np.float32([0.5, 0, 0]))          # between colours 0 and 1
    np.testing.assert_array_equal(ref["colors"][7], np.float32([11, 0, 0]))
    # the normal of the first point: D_x(0,0,0) = f(1) - f(0) = -1 (one-sided), D_x(1,0,0) = 0.5 (1/2 - 1/2) = 0; y: voxel
    # (0,1,0) is unobserved, so D_y(0,0,0) = 0, and D_y(1,0,0) = 0.5 - -0.5 = 1; z: 0 and 1 -> g = (-0.5, 0.5, 0.5)
    np.testing.assert_allclose(ref["normals"][0], np.float32([-1, 1, 1]) / np.sqrt(3), rtol=0, atol=1e-7)
    assert np.allclose(np.linalg.norm(ref["normals"], axis=1), 1.0, atol=1e-6)
    # min_weight above every weight: nothing is observed
    assert len(ref_extract(tsdf, weight, color, 0.5, (0.0, 0.0, 0.0), 1.5)["edge"]) == 0


# ------------------------------------------------------------------ GPU: shared scene, state and references (computed once)
def to_dev(*xs):
    return tuple(x.to(DEV) for x in xs)


def frames_of(seq, b=None, l=None):
    colors, depths, K, poses = seq
    bs = slice(None) if b is None else slice(b, b + 1)
    ls = slice(None) if l is None else slice(l, l + 1)
    return gs.RGBDImages(colors[bs, ls].contiguous(), depths[bs, ls].contiguous(), K[bs].contiguous(), poses[bs, ls].contiguous())


@lru_cache(maxsize=None)
def scene():
    return to_dev(*make_sequence(2, 3, H, W, seed=0))


def new_volume(dims=DIMS, origins=ORIGINS, sentinel=False, **kw):
    vol = gs.structures.TSDFVolume(dims, V, origin=origins, trunc=TRUNC, max_weight=MAXW, device=DEV, **kw)
    if sentinel:
        vol.tsdf.fill_(SENT_T)
        vol.color.fill_(SENT_C)
    return vol


def device_pixels(cent, seq):
    """(active, pix) (B, L, n) of the centres cent (B, n, 3) from ops.project_active_raw, and z (B, L, n) in float64."""
    _, depths, K, poses = seq
    B, L = poses.shape[:2]
    n = cent.shape[1]
    pts = torch.from_numpy(cent).to(DEV)
    counts = torch.full((B,), n, dtype=torch.int32, device=DEV)
    act, pix = np.zeros((B, L, n), bool), np.zeros((B, L, n), np.int64)
    z = np.zeros((B, L, n))
    P = poses.cpu().numpy().astype(np.float64)
    for l in range(L):
        rows, cnt = ops.project_active_raw(pts, counts, poses[:, l].contiguous(), K[:, 0].contiguous(), depths.shape[2], depths.shape[3])
        r = rows[: int(cnt)].cpu().numpy()
        act[r[:, 0], l, r[:, 1]] = True
        pix[r[:, 0], l, r[:, 1]] = r[:, 2] * depths.shape[3] + r[:, 3]
        for b in range(B):
            z[b, l] = (cent[b].astype(np.float64) - P[b, l, :3, 3]) @ P[b, l, :3, 2]
    return act, pix, z


def reference_state(dims, origins, seq, f0, w0, c0, maxw=MAXW):
    """The float64 reference of every batch element from the state (f0, w0, c0), each (B, n[, 3]) -> list of (f, w, col, rec),
    and (act, pix, z)."""
    colors, depths, _, _ = seq
    B, L = depths.shape[:2]
    cent = np.stack([ref_centres(dims, V, o) for o in origins])
    act, pix, z = device_pixels(cent, seq)
    d, c = depths.reshape(B, L, -1).cpu().numpy(), colors.reshape(B, L, -1, 3).cpu().numpy()
    out = [ref_integrate(act[b], pix[b], z[b], d[b], c[b], f0[b], w0[b], c0[b], TRUNC, maxw) for b in range(B)]
    return out, (act, pix, z)


def flat(vol):
    B = len(vol)
    return (vol.tsdf.reshape(B, -1).cpu().numpy(), vol.weight.reshape(B, -1).cpu().numpy(), vol.color.reshape(B, -1, 3).cpu().numpy())


def check_against_reference(dims, origins, seq):
    """Test 1's comparison for one volume; returns the figures it printed."""
    B = len(origins)
    n = dims[0] * dims[1] * dims[2]
    L = seq[1].shape[1]
    vol = new_volume(dims, origins, sentinel=True)
    out = vol.integrate(frames_of(seq))
    assert out is not vol and torch.equal(vol.tsdf, torch.full_like(vol.tsdf, SENT_T)) and float(vol.weight.abs().max()) == 0.0
    ref, _ = reference_state(dims, origins, seq, np.full((B, n), SENT_T), np.zeros((B, n)), np.full((B, n, 3), SENT_C))
    f, w, c = flat(out)
    figures = []
    for b in range(B):
        rf, rw, rc, rec = ref[b]
        tie = np.any([r["tie_skip"] for r in rec], 0)
        touched = np.any([r["upd"] for r in rec], 0)
        share = tie.mean()
        keep = ~tie
        assert np.array_equal(w[b][keep], rw[keep].astype(np.float32)), "weight"
        dt = np.abs(f[b].astype(np.float64) - rf)[keep].max()
        dc = np.abs(c[b].astype(np.float64) - rc)[keep].max()
        print("dims", dims, "b", b, "tie share", share, "max |d tsdf|", dt, "max |d color|", dc, "touched", int(touched.sum()),
              "pairs: outside", sum(int((~r["seen"]).sum()) for r in rec), "occluded", sum(int(r["occ"].sum()) for r in rec),
              "saturated", sum(int(r["sat"].sum()) for r in rec), "linear", sum(int(r["lin"].sum()) for r in rec),
              "at the cap", int((rw >= MAXW).sum()))
        assert share <= 0.005
        assert dt <= 1e-5
        assert dc <= 6 * L * U * 255
        still = keep & ~touched  # no frame touched them: the previous BITS
        assert np.array_equal(f[b][still].view(np.uint32), np.full(int(still.sum()), SENT_T, np.float32).view(np.uint32))
        assert np.array_equal(c[b][still].view(np.uint32), np.full((int(still.sum()), 3), SENT_C, np.float32).view(np.uint32))
        assert (w[b][still] == 0).all()
        figures.append((int(touched.sum()), int(still.sum())))
    return figures


@lru_cache(maxsize=None)
def fused():
    """The common scene fused into a fresh volume (one call, L = 3): the state the extraction tests read."""
    return new_volume().integrate(frames_of(scene()))


def same_state(a, b):
    return torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and torch.equal(a.color, b.color)


# ------------------------------------------------------------------ GPU 1: integration against the float64 reference
@pytest.mark.gpu
@pytest.mark.parametrize("dims", [DIMS, (40, 22, 56)], ids=["nx42", "nx40_vector_path"])
def test_integrate_matches_the_float64_reference(dims):
    figures = check_against_reference(dims, ORIGINS, scene())
    for touched, still in figures:  # the scene holds both kinds of voxel, in numbers
        assert touched > 10000 and still > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 1, 1), (3, 2, 1)])
def test_integrate_tiny_volumes_match_the_reference(dims):
    check_against_reference(dims, [(0.0, 0.0, 1.9), (0.05, -0.1, 1.95)], scene())


# ------------------------------------------------------------------ GPU 2: equivalences, all bitwise
@pytest.mark.gpu
def test_one_call_equals_single_frame_calls_and_inplace_and_batches():
    seq = scene()
    want = fused()
    step = new_volume()
    for l in range(3):
        step = step.integrate(frames_of(seq, l=l))
    assert same_state(step, want)
    inpl = new_volume()
    ptrs = (inpl.tsdf.data_ptr(), inpl.weight.data_ptr(), inpl.color.data_ptr())
    assert inpl.integrate(frames_of(seq), inplace=True) is inpl
    assert ptrs == (inpl.tsdf.data_ptr(), inpl.weight.data_ptr(), inpl.color.data_ptr()) and same_state(inpl, want)
    for b in range(2):
        one = new_volume(origins=[ORIGINS[b]]).integrate(frames_of(seq, b=b))
        assert torch.equal(one.tsdf[0], want.tsdf[b]) and torch.equal(one.weight[0], want.weight[b]) and torch.equal(one.color[0], want.color[b])
    # channels-first frames are converted; a volume without colours takes the same tsdf and weight
    cf = new_volume().integrate(frames_of(seq).to_channels_first())
    assert same_state(cf, want)
    nocol = new_volume(color=False).integrate(frames_of(seq))
    assert nocol.color is None and torch.equal(nocol.tsdf, want.tsdf) and torch.equal(nocol.weight, want.weight)
    assert float(want.weight.max()) == MAXW and float(want.tsdf.min()) < -0.5


@pytest.mark.gpu
def test_33_frames_cross_the_chunk_of_32():
    seq = to_dev(*make_sequence(1, 33, H, W, seed=5))
    kw = dict(origins=[ORIGINS[0]])
    vol = gs.structures.TSDFVolume(DIMS, V, origin=[ORIGINS[0]], trunc=TRUNC, max_weight=40.0, device=DEV)  # the cap is not reached before frame 33
    one = vol.integrate(frames_of(seq))
    step = vol
    for l in range(33):
        step = step.integrate(frames_of(seq, l=l))
    assert same_state(one, step) and float(one.weight.max()) > 32.0
    capped = new_volume(**kw).integrate(frames_of(seq))
    step = new_volume(**kw)
    for l in range(33):
        step.integrate(frames_of(seq, l=l), inplace=True)
    assert same_state(capped, step) and float(capped.weight.max()) == MAXW


# ------------------------------------------------------------------ GPU 3: extraction on the device's own state
def extract_refs(vol, minw):
    f, w, c = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy()
    return [ref_extract(f[b], w[b], c[b], V, ORIGINS[b], minw) for b in range(len(vol))]


@pytest.mark.gpu
@pytest.mark.parametrize("minw", [1.0, 2.0])
def test_extraction_matches_the_numpy_reference_bitwise(minw):
    vol = fused()
    refs = extract_refs(vol, minw)
    counts = [len(r["edge"]) for r in refs]
    print("min_weight", minw, "surface points", counts, "per axis", [np.bincount(r["axis"], minlength=3).tolist() for r in refs])
    assert min(counts) > 500 and all(np.bincount(r["axis"], minlength=3).min() > 50 for r in refs)
    cap = max(counts)
    n0 = ops.tsdf_extract_raw(vol.tsdf, vol.weight, vol.color, vol.origin, V, minw, cap=0)
    assert n0[:4] == (None, None, None, None) and n0[4].tolist() == counts
    points, normals, colors, edge, n_points = ops.tsdf_extract_raw(vol.tsdf, vol.weight, vol.color, vol.origin, V, minw, cap=cap)
    assert n_points.tolist() == counts and n_points.dtype == torch.int32 and edge.dtype == torch.int32
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for b, r in enumerate(refs):
        m = counts[b]
        assert np.array_equal(edge[b, :m].cpu().numpy(), r["edge"])
        assert np.array_equal(bits(points[b, :m].cpu().numpy()), bits(r["points"]))
        assert np.array_equal(bits(colors[b, :m].cpu().numpy()), bits(r["colors"]))
        dn = np.abs(normals[b, :m].cpu().numpy() - r["normals"]).max()
        print("b", b, "max |d normal|", dn)
        assert dn <= 1e-5
        assert (edge[b, m:] == -1).all() and (points[b, m:] == 0).all() and (normals[b, m:] == 0).all() and (colors[b, m:] == 0).all()
    pc = vol.extract_pointcloud(min_weight=minw)
    assert isinstance(pc, gs.Pointclouds) and pc.num_points_per_pointcloud.tolist() == counts
    assert torch.equal(pc.points_padded, points) and torch.equal(pc.normals_padded, normals) and torch.equal(pc.colors_padded, colors)
    assert pc.points_list[1].shape == (counts[1], 3)
    # a cap below the count: the first cap rows, the full count
    small = 100
    p2, n2, c2, e2, k2 = ops.tsdf_extract_raw(vol.tsdf, vol.weight, vol.color, vol.origin, V, minw, cap=small)
    assert k2.tolist() == counts and torch.equal(e2, edge[:, :small]) and torch.equal(p2, points[:, :small])
    assert torch.equal(n2, normals[:, :small]) and torch.equal(c2, colors[:, :small])


@pytest.mark.gpu
def test_fresh_volume_gives_an_empty_pointcloud():
    pc = new_volume().extract_pointcloud()
    assert len(pc) == 2 and pc.num_points_per_pointcloud.tolist() == [0, 0]
    assert pc.points_padded.shape == (2, 0, 3) and pc.normals_padded.shape == (2, 0, 3) and pc.colors_padded.shape == (2, 0, 3)
    assert ops.tsdf_extract_raw(*(lambda v: (v.tsdf, v.weight, v.color, v.origin, V))(new_volume()), cap=8)[4].tolist() == [0, 0]


@pytest.mark.gpu
def test_surface_lies_on_the_analytic_wall_with_normals_towards_the_camera():
    pc = fused().extract_pointcloud()
    worst = 0.0
    for b in range(2):
        p, n = pc.points_list[b].cpu().numpy().astype(np.float64), pc.normals_list[b].cpu().numpy()
        dist = np.abs(p[:, 2] - (2.0 + 0.3 * np.sin(2.0 * p[:, 0]) * np.cos(2.0 * p[:, 1])))  # along z: no less than the distance
        worst = max(worst, dist.max())
        assert (n[:, 2] < 0).mean() > 0.99  # free space is on the camera's side (z below the wall)
        assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)
    print("max distance to the wall", worst)
    assert worst <= V / 2


# ------------------------------------------------------------------ GPU 4: gradients
@pytest.mark.gpu
def test_integrate_gradients_match_the_explicit_formulas_and_repeat_bitwise():
    seq = scene()
    colors, depths, K, poses = seq
    B, L = 2, 3
    n, npix = DIMS[0] * DIMS[1] * DIMS[2], H * W
    rng = np.random.RandomState(11)
    f0 = rng.uniform(-1, 1, (B, n)).astype(np.float32)
    w0 = rng.randint(0, 3, (B, n)).astype(np.float32)
    c0 = rng.uniform(0, 255, (B, n, 3)).astype(np.float32)
    ref, (act, pix, z) = reference_state(DIMS, ORIGINS, seq, f0, w0, c0)
    g_f, g_c = rng.randn(B, n).astype(np.float32), rng.randn(B, n, 3).astype(np.float32)
    for b in range(B):  # voxels that sit on a threshold get no upstream adjoint: their decision is not the reference's to take
        tie = np.any([r["tie"] for r in ref[b][3]], 0)
        assert tie.mean() <= 0.005
        g_f[b][tie] = 0
        g_c[b][tie] = 0
    shape = (B, DIMS[2], DIMS[1], DIMS[0])
    dev = lambda x, s: torch.from_numpy(x).reshape(s).to(DEV)
    origin = ops.tsdf_origin(ORIGINS, B, DEV)

    def run():
        d, c = depths.clone().requires_grad_(True), colors.clone().requires_grad_(True)
        t, col = dev(f0, shape).requires_grad_(True), dev(c0, shape + (3,)).requires_grad_(True)
        out_t, out_w, out_c = ops.tsdf_integrate(d, c, K, poses, t, dev(w0, shape), col, origin, V, TRUNC, MAXW)
        assert not out_w.requires_grad
        torch.autograd.backward([out_t, out_c], [dev(g_f, shape), dev(g_c, shape + (3,))])
        return out_t, out_w, (t.grad, col.grad, d.grad, c.grad)

    out_t, out_w, grads = run()
    for b in range(B):  # the forward from this state too
        keep = ~np.any([r["tie_skip"] for r in ref[b][3]], 0)
        assert np.array_equal(out_w[b].reshape(-1).cpu().numpy()[keep], ref[b][1][keep].astype(np.float32))
        assert np.abs(out_t[b].detach().reshape(-1).cpu().numpy() - ref[b][0])[keep].max() <= 1e-5
    got = [g.reshape(s).cpu().numpy() for g, s in zip(grads, ((B, n), (B, n, 3), (B, L, npix), (B, L, npix, 3)))]
    for b in range(B):
        rec = ref[b][3]
        want = ref_integrate_backward(rec, pix[b], g_f[b], g_c[b], TRUNC, npix)
        A = ref_integrate_backward(rec, pix[b], np.abs(g_f[b]), np.abs(g_c[b]), TRUNC, npix)
        for name, g, wnt, a in zip(("tsdf", "color", "depth", "rgb"), got, want, A):
            err = np.abs(g[b].astype(np.float64) - wnt)
            ratio = (err / np.maximum(a, 1e-300)).max() / U
            print("integrate adjoint", name, "b", b, "max err / (2^-24 A)", ratio, "nonzero", int((wnt != 0).sum()))
            assert (wnt != 0).sum() > 1000, name
            assert (err <= 32 * U * a).all(), name
    for flag in (True, False):
        torch.use_deterministic_algorithms(flag)
        try:
            again = run()[2]
        finally:
            torch.use_deterministic_algorithms(False)
        assert all(torch.equal(a, b) for a, b in zip(again, grads)), flag


TINY_DIMS, TINY_ORIGIN, TINY_H, TINY_W = (8, 6, 5), [(-0.2, -0.15, 1.85)], 12, 16  # a pixel is 0.15 wide at the wall: 3 voxels


@pytest.mark.gpu
@pytest.mark.parametrize("color", [True, False], ids=["color", "no_color"])
def test_integrate_reverse_with_non_finite_upstream_entries(color):
    """g_tsdf = +inf at one voxel and NaN at another, both updated inside the band by both frames.  A pixel that receives a
    non-finite term holds what a float sum of its terms gives (the terms: the kernel's fp32 chain (g / (W + 1)) / trunc, then
    g = g (W / (W + 1)), from the last frame to the first); every other element of g_depth and g_rgb holds the bits of the same
    call with the two entries set to zero."""
    seq = to_dev(*make_sequence(1, 2, TINY_H, TINY_W, seed=3, band=0))
    _, depths, K, poses = seq
    L, n, npix = 2, TINY_DIMS[0] * TINY_DIMS[1] * TINY_DIMS[2], TINY_H * TINY_W
    ref, (act, pix, z) = reference_state(TINY_DIMS, TINY_ORIGIN, seq, np.zeros((1, n)), np.zeros((1, n)), np.zeros((1, n, 3)))
    rec, pix = ref[0][3], pix[0]
    both = np.all([r["lin"] & ~r["tie"] for r in rec], 0)
    cand = np.nonzero(both)[0]
    assert len(cand) >= 2
    bad = {int(cand[0]): np.float32(np.inf), int(cand[-1]): np.float32(np.nan)}
    rng = np.random.RandomState(4)
    g_f, g_c = rng.randn(1, n).astype(np.float32), rng.randn(1, n, 3).astype(np.float32)
    g_bad, g_zero = g_f.copy(), g_f.copy()
    terms = {}  # (frame, pixel) -> the non-finite terms it receives
    for j, val in bad.items():
        g_bad[0, j], g_zero[0, j] = val, 0.0
        g = val
        with np.errstate(invalid="ignore"):
            for l in reversed(range(L)):
                Wb = np.float32(rec[l]["W"][j])
                den = Wb + np.float32(1.0)
                terms.setdefault((l, int(pix[l][j])), []).append((g / den) / np.float32(TRUNC))
                g = g * (Wb / den)
    shape = (1, TINY_DIMS[2], TINY_DIMS[1], TINY_DIMS[0])
    dev = lambda x, s: torch.from_numpy(x).reshape(s).to(DEV)
    origin = ops.tsdf_origin(TINY_ORIGIN, 1, DEV)
    w0 = torch.zeros(shape, device=DEV)
    run = lambda gt: ops.tsdf_integrate_backward_raw(depths, K, poses, w0, origin, V, TRUNC, MAXW, dev(gt, shape),
                                                     dev(g_c, shape + (3,)) if color else None)
    got, want = run(g_bad), run(g_zero)
    assert (got[3] is None) == (not color)
    gd, zd = (x[2].reshape(L, npix).cpu().numpy() for x in (got, want))
    hit = np.zeros((L, npix), bool)
    for (l, p), ts in terms.items():
        assert not np.isfinite(ts).any()
        hit[l, p] = True
        w, h = exact_sum_f32(ts), gd[l, p]
        assert (np.isnan(w) and np.isnan(h)) or w.view(np.uint32) == h.view(np.uint32), (l, p, w, h)
    assert hit.sum() <= 2 * L and np.isposinf(gd[hit]).any() and np.isnan(gd[hit]).any()
    assert np.array_equal(gd.view(np.uint32)[~hit], zd.view(np.uint32)[~hit]) and (zd != 0).sum() > 10  # (the volume covers 8 or 9 pixels of each frame)
    if color:
        assert torch.equal(got[3].view(torch.int32), want[3].view(torch.int32)) and torch.equal(got[1], want[1])
    keep = np.ones(n, bool)
    keep[list(bad)] = False
    assert torch.equal(got[0].reshape(-1)[torch.from_numpy(keep).to(DEV)].view(torch.int32),
                       want[0].reshape(-1)[torch.from_numpy(keep).to(DEV)].view(torch.int32))


@pytest.mark.gpu
def test_extract_gradients_match_the_explicit_formulas_and_repeat_bitwise():
    vol = fused()
    refs = extract_refs(vol, 1.0)
    counts = [len(r["edge"]) for r in refs]
    cap = max(counts)
    rng = np.random.RandomState(12)
    g_p, g_c = rng.randn(2, cap, 3).astype(np.float32), rng.randn(2, cap, 3).astype(np.float32)

    def run():
        t, c = vol.tsdf.clone().requires_grad_(True), vol.color.clone().requires_grad_(True)
        points, normals, colors, edge, n_points = ops.tsdf_extract(t, vol.weight, c, vol.origin, V, 1.0, cap=cap)
        assert not normals.requires_grad and n_points.tolist() == counts
        torch.autograd.backward([points, colors], [torch.from_numpy(g_p).to(DEV), torch.from_numpy(g_c).to(DEV)])
        return t.grad, c.grad

    grads = run()
    f, c = vol.tsdf.cpu().numpy(), vol.color.cpu().numpy()
    for b, r in enumerate(refs):
        m = counts[b]
        args = (f[b], c[b], V, r["j0"], r["j1"], r["axis"], g_p[b, :m], g_c[b, :m])
        want, A = ref_extract_backward(*args), ref_extract_backward(*args, absolute=True)
        for name, g, wnt, a in zip(("tsdf", "color"), grads, want, A):
            err = np.abs(g[b].reshape(wnt.shape).cpu().numpy().astype(np.float64) - wnt)
            print("extract adjoint", name, "b", b, "max err / (2^-24 A)", (err / np.maximum(a, 1e-300)).max() / U, "nonzero", int((wnt != 0).sum()))
            assert (wnt != 0).sum() > 1000, name
            assert (err <= 32 * U * a).all(), name
    for flag in (True, False):
        torch.use_deterministic_algorithms(flag)
        try:
            again = run()
        finally:
            torch.use_deterministic_algorithms(False)
        assert all(torch.equal(a, b) for a, b in zip(again, grads)), flag


# ------------------------------------------------------------------ GPU 5: end to end
@pytest.mark.gpu
def test_end_to_end_chamfer_loss_reaches_depth_and_rgb():
    """chamfer_distance differentiates the points only, so it reaches the depth images; the rgb images are reached through the
    surface's colours, by a colour term added to the loss.  chamfer_distance's own reverse pass adds with float atomics unless
    torch.use_deterministic_algorithms is on, so the bits of everything behind it are compared under the flag; the rgb adjoint
    passes through the TSDF nodes only and is the same bits without it."""
    colors, depths, K, poses = scene()
    target = pointclouds_from_rgbdimages(gs.RGBDImages(colors[:, :1], depths[:, :1], K, poses[:, :1]))

    def run():
        d, c = depths.clone().requires_grad_(True), colors.clone().requires_grad_(True)
        pc = new_volume().integrate(gs.RGBDImages(c, d, K, poses)).extract_pointcloud()
        loss = chamfer_distance(pc, target)
        (g_d,) = torch.autograd.grad(loss, d, retain_graph=True)
        (loss + 1e-3 * pc.colors_padded.mean()).backward()
        return loss.detach(), g_d, d.grad, c.grad

    first = run()
    assert torch.isfinite(first[0]) and 0.0 < float(first[0]) < 0.05
    for g in first[1:]:
        assert g is not None and torch.isfinite(g).all() and int((g != 0).sum()) > 100
    again = run()
    assert torch.equal(again[0], first[0]) and torch.equal(again[3], first[3])
    torch.use_deterministic_algorithms(True)
    try:
        a, b = run(), run()
    finally:
        torch.use_deterministic_algorithms(False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[3], first[3]) and all(int((g != 0).sum()) > 100 for g in a[1:])
