#!/usr/bin/env python3
"""The outputs of the five callers of the exact fold (gs_fixed128.hpp) on fixed inputs, as raw bytes:

    python tools/fold_ab.py OUTDIR

writes OUTDIR/<caller>_<shape>_<output>.bin and prints one "sha256  name" line per file.  The fold is exact, so two builds of
the library must give byte-identical files: run it on both and compare the listings.  Per caller a small shape (odd sizes, more
than one block, some non-finite terms) and a mid-sized one; every input comes from a seeded generator."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.synthetic import make_sequence

DEV = "cuda:0"


def spoil(x, rs, n):
    """n entries of x become NaN, +inf or -inf."""
    flat = x.reshape(-1)
    flat[rs.choice(flat.size, n, replace=False)] = rs.choice([np.nan, np.inf, -np.inf], n)
    return x


def voxel(rs, N, C, bad):
    pts = torch.from_numpy(rs.rand(2, N, 3).astype(np.float32)).to(DEV)
    counts = torch.tensor([N, N - N // 3], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(spoil(rs.randn(2, N, C).astype(np.float32) * 10.0 ** rs.randint(-3, 4, (2, N, 1)), rs, bad)).float().to(DEV)
    vof, nv, _, cnt, _ = ops.voxel_assign(pts, counts, 0.07)
    M = int(nv.max())
    return {"sum": ops.voxel_reduce_raw(x, counts, vof, nv, cnt, M, ops.VOXEL_SUM), "mean": ops.voxel_reduce_raw(x, counts, vof, nv, cnt, M),
            "sum_no_preagg": ops.voxel_reduce_raw(x, counts, vof, nv, cnt, M, ops.VOXEL_SUM | ops.VOXEL_NO_PREAGG)}


def knn(rs, Ns, Nt, K, bad):
    src, tgt = (torch.from_numpy(rs.rand(2, n, 3).astype(np.float32)).to(DEV) for n in (Ns, Nt))
    cs, ct = (torch.tensor([n, n - n // 3], dtype=torch.int32, device=DEV) for n in (Ns, Nt))
    keys = ops.knn_raw(src, tgt, cs, ct, K)
    g = torch.from_numpy(spoil(rs.randn(2, Ns, K).astype(np.float32), rs, bad)).to(DEV)
    g_src, g_tgt = ops.knn_backward_raw(src, tgt, cs, ct, keys, g)
    return {"g_src": g_src, "g_tgt": g_tgt}


def tsdf(rs, L, H, W, dims, origin, bad):
    """Integration's reverse pass, then the ray cast's reverse pass over the integrated volume."""
    colors, depths, K, poses = (t.to(DEV) for t in make_sequence(1, L, H, W, seed=3, band=0))
    vol = gs.TSDFVolume(dims, 0.05, origin=[origin], trunc=0.15, max_weight=2.0, device=DEV)
    n = dims[0] * dims[1] * dims[2]
    shape = (1, dims[2], dims[1], dims[0])
    g_t = torch.from_numpy(spoil(rs.randn(n).astype(np.float32), rs, bad)).reshape(shape).to(DEV)
    g_c = torch.from_numpy(rs.randn(n, 3).astype(np.float32)).reshape(shape + (3,)).to(DEV)
    o_t, o_c, g_depth, g_rgb = ops.tsdf_integrate_backward_raw(depths, K, poses, vol.weight, vol.origin, 0.05, 0.15, 2.0, g_t, g_c)
    out = {"integrate_g_tsdf_in": o_t, "integrate_g_color_in": o_c, "integrate_g_depth": g_depth, "integrate_g_rgb": g_rgb}
    out["integrate_nocolor_g_depth"] = ops.tsdf_integrate_backward_raw(depths, K, poses, vol.weight, vol.origin, 0.05, 0.15, 2.0, g_t)[2]
    vol = vol.integrate(gs.RGBDImages(colors, depths, K, poses))
    cast = ops.tsdf_raycast_raw(vol.tsdf, vol.weight, vol.color, vol.origin, 0.05, K, poses, H, W, 1, 0.075)
    gd = torch.from_numpy(spoil(rs.randn(*cast[0].shape).astype(np.float32), rs, bad)).to(DEV)
    gc = torch.from_numpy(rs.randn(*cast[2].shape).astype(np.float32)).to(DEV)
    args = (vol.origin, 0.05, K, poses, H, W, 1, 0.075, 1.0, cast[3])
    out["cast_hits"] = (cast[3] > 0).sum().reshape(1).int()
    out["cast_g_tsdf"], out["cast_g_color"] = ops.tsdf_raycast_backward_raw(vol.tsdf, vol.weight, vol.color, *args, gd, gc)
    out["cast_nocolor_g_tsdf"] = ops.tsdf_raycast_backward_raw(vol.tsdf, vol.weight, None, *args, gd, None)[0]
    return out


def det(rs, ns, nt, bad):
    """ops.icp_linearize's reverse pass under torch.use_deterministic_algorithms: the fold of gs_detfold.hpp."""
    src, tgt, nrm = (torch.from_numpy(rs.rand(n, 3).astype(np.float32)).to(DEV).requires_grad_(True) for n in (ns, nt, nt))
    gH = torch.from_numpy(spoil(rs.randn(6, 6).astype(np.float32), rs, bad)).to(DEV)
    gg, ge = torch.from_numpy(rs.randn(6, 1).astype(np.float32)).to(DEV), torch.tensor(0.5, device=DEV)
    old = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        best = ops.knn1_raw(src.detach(), tgt.detach())
        torch.autograd.backward(list(ops.icp_linearize(src, tgt, nrm, best, None)), [gH, gg, ge])
    finally:
        torch.use_deterministic_algorithms(old)
    return {"g_src": src.grad, "g_tgt": tgt.grad, "g_nrm": nrm.grad}


CASES = [("voxel_small", lambda rs: voxel(rs, 777, 13, 6)), ("voxel_mid", lambda rs: voxel(rs, 200000, 10, 0)),
         ("knn_small", lambda rs: knn(rs, 300, 70, 3, 4)), ("knn_mid", lambda rs: knn(rs, 50000, 30000, 8, 0)),
         ("tsdf_small", lambda rs: tsdf(rs, 2, 12, 16, (8, 6, 5), (-0.2, -0.15, 1.85), 2)),
         ("tsdf_mid", lambda rs: tsdf(rs, 3, 48, 64, (42, 22, 56), (-1.0, -0.55, -0.2), 0)),
         ("det_small", lambda rs: det(rs, 130, 40, 1)), ("det_mid", lambda rs: det(rs, 65536, 1024, 0))]


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    for k, (name, fn) in enumerate(CASES):
        for what, t in fn(np.random.RandomState(100 + k)).items():
            raw = t.detach().contiguous().cpu().numpy().tobytes()
            with open(os.path.join(outdir, "%s_%s.bin" % (name, what)), "wb") as f:
                f.write(raw)
            print(hashlib.sha256(raw).hexdigest(), "%s_%s" % (name, what), len(raw), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
