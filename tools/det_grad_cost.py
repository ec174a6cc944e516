#!/usr/bin/env python3
"""Cost of bit-reproducible gradients (torch.use_deterministic_algorithms): one JSON line, medians of 5 runs, of
  * the ICP reverse pass alone at c2 sizes (19 200 sources and targets, gradICP, 10 iterations), default vs `_det`;
  * 30 frames of c3 PointFusion gradICP forward + backward at 640x480 with the flag off;
  * the same with the flag on, with torch's fill of uninitialised memory on (its default) and off."""
import json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd.synthetic import make_sequence_cached as make_sequence

dev = "cuda:0"
REPS = 5


def icp_reverse_ms(det):
    c, d, K, P = make_sequence(1, 2, 120, 160, seed=3)
    r = gs.RGBDImages(c.to(dev), d.to(dev), K.to(dev), P[:, :1].repeat(1, 2, 1, 1).to(dev))
    tgt_pc = gs.structures.utils.pointclouds_from_rgbdimages(r[:, 0])
    src_pc = gs.structures.utils.pointclouds_from_rgbdimages(r[:, 1])
    s, tg, n = (x.clone().requires_grad_(True) for x in (src_pc.points_list[0], tgt_pc.points_list[0], tgt_pc.normals_list[0]))
    T0 = torch.eye(4, device=dev).requires_grad_(True)
    torch.use_deterministic_algorithms(det)
    try:
        T, _ = gs.odometry.icputils.point_to_plane_gradICP(s[None], tg[None], n[None], T0, numiters=10)
        gT = torch.randn(4, 4, device=dev)
        out = []
        for _ in range(REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.autograd.grad(T, (s, tg, n, T0), gT, retain_graph=True)
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
    finally:
        torch.use_deterministic_algorithms(False)
    return statistics.median(out[1:])  # (the first call sizes the workspaces)


def pointfusion_ms(det, fill=True):
    c, d, K, P = make_sequence(1, 30, 480, 640, seed=7)
    torch.use_deterministic_algorithms(det)
    torch.utils.deterministic.fill_uninitialized_memory = fill
    out = []
    try:
        for _ in range(REPS + 1):
            cc, dd, kk, pp = (x.to(dev).clone().requires_grad_(True) for x in (c, d, K, P))
            slam = gs.slam.PointFusion(odom="gradicp", dsratio=4, numiters=10, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pcs, poses = slam(gs.RGBDImages(cc, dd, kk, pp))
            (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
    finally:
        torch.use_deterministic_algorithms(False)
        torch.utils.deterministic.fill_uninitialized_memory = True
    return statistics.median(out[1:])  # (the first run warms the caches and the workspaces)


if __name__ == "__main__":
    r = {"tool": "det_grad_cost", "runs": REPS, "device": torch.cuda.get_device_name(0)}
    r["icp_reverse_c2_gradicp10_ms"] = {"default": round(icp_reverse_ms(False), 3), "det": round(icp_reverse_ms(True), 3)}
    off = pointfusion_ms(False)
    on_fill, on_nofill = pointfusion_ms(True, True), pointfusion_ms(True, False)
    r["pointfusion_c3_gradicp_30f_fwd_bwd_ms"] = {"flag_off": round(off, 1), "det_fill_on": round(on_fill, 1), "det_fill_off": round(on_nofill, 1)}
    r["det_over_default"] = {"icp_reverse": round(r["icp_reverse_c2_gradicp10_ms"]["det"] / r["icp_reverse_c2_gradicp10_ms"]["default"], 3),
                             "pointfusion_fill_on": round(on_fill / off, 3), "pointfusion_fill_off": round(on_nofill / off, 3)}
    print(json.dumps(r))
