#!/usr/bin/env python3
"""Cost of rendering the map into a camera (gs_render_map) against the torch-op chain it replaces: one JSON line, medians of
5 regions, at 640x480 on the map a 100-frame PointFusion run leaves behind, seen from the last frame's camera.
  (a) ops.render_map_raw (three launches) and ops.render_map_backward_raw (all four adjoints given, all four results wanted);
  (b) what a user writes without it: project_active_raw rows -> camera-frame z of those rows -> an int64 (z bits, row) key ->
      scatter_reduce_(amin) per pixel -> gathers of position, normal and colour; its backward is torch autograd through the
      gathers and z.
Also the algorithmic bytes of (a) from the shapes: 12 B read per map row + 8 B per candidate atomic, and per pixel 8 B of key
written and read + 8 B of index / depth + 72 B of gathered and written attributes."""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.synthetic import make_sequence_cached as make_sequence

dev = "cuda:0"
REGIONS, CALLS = 5, 20


def region_ms(fn):
    """median over REGIONS of the mean time of CALLS back-to-back calls (host clock around a device synchronise)"""
    fn()
    out = []
    for _ in range(REGIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / CALLS)
    return statistics.median(out)


def torch_chain(pts, nrm, col, counts, pose, K, H, W):
    """(b): -> (index (H,W) int64, depth, points, normals, colors), differentiable w.r.t. pts / nrm / col / pose"""
    rows, cnt = ops.project_active_raw(pts.detach(), counts, pose.detach(), K, H, W)
    rows = rows[: int(cnt.item())]
    n, pix = rows[:, 1], rows[:, 2] * W + rows[:, 3]
    R2, t = pose[0, :3, 2], pose[0, :3, 3]
    z = ((pts[0] - t) * R2).sum(-1)
    key = (z.detach()[n].view(torch.int32).to(torch.int64) << 32) | n
    none = torch.iinfo(torch.int64).max
    best = torch.full((H * W,), none, dtype=torch.int64, device=pts.device).scatter_reduce_(0, pix, key, "amin")
    hit = best != none
    index = torch.where(hit, best & 0xFFFFFFFF, torch.zeros_like(best))
    m = hit.unsqueeze(-1)
    depth = torch.where(hit, z[index], torch.zeros((), device=pts.device))
    img = lambda a: torch.where(m, a[0][index], torch.zeros((), device=pts.device)).view(H, W, 3)
    return torch.where(hit, index, -torch.ones_like(index)).view(H, W), depth.view(H, W), img(pts), img(nrm), img(col)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_cost.json"))
    a = ap.parse_args()
    H, W = a.height, a.width
    c, d, K, P = (x.to(dev) for x in make_sequence(1, a.frames, H, W, seed=7))
    pcs, _ = gs.slam.PointFusion(odom="gt", device=dev)(gs.RGBDImages(c, d, K, P))
    pts, nrm, col, counts = pcs.points_padded.contiguous(), pcs.normals_padded.contiguous(), pcs.colors_padded.contiguous(), pcs._counts_i32()
    pose, K1 = P[:, -1].contiguous(), K[:, 0].contiguous()
    N = pts.shape[1]

    index, depth, pimg, nimg, cimg = ops.render_map_raw(pts, nrm, col, counts, pose, K1, H, W)
    _, n_act = ops.project_active_raw(pts, counts, pose, K1, H, W)
    t_idx, t_depth, _, _, t_col = torch_chain(pts, nrm, col, counts, pose, K1, H, W)
    n_hit = int((index >= 0).sum())
    g = torch.Generator(device=dev).manual_seed(1)
    g_d = torch.randn(1, H, W, device=dev, generator=g)
    g_p, g_n, g_c = (torch.randn(1, H, W, 3, device=dev, generator=g) for _ in range(3))

    def torch_fwd_bwd():
        leaves = [x.clone().requires_grad_(True) for x in (pts, nrm, col, pose)]
        _, dd, pp, nn, cc = torch_chain(leaves[0], leaves[1], leaves[2], counts, leaves[3], K1, H, W)
        ((dd * g_d[0]).sum() + (pp * g_p[0]).sum() + (nn * g_n[0]).sum() + (cc * g_c[0]).sum()).backward()

    r = {"tool": "render_cost", "regions": REGIONS, "calls_per_region": CALLS, "device": torch.cuda.get_device_name(0),
         "frames": a.frames, "image": [H, W], "map_rows": N, "candidates": int(n_act.item()), "pixels_hit": n_hit,
         "index_pixels_differing_from_torch_chain": int((index[0].long() != t_idx).sum()),
         "depth_max_abs_diff_to_torch_chain": float((depth[0] - t_depth).abs().max())}
    r["render_map_ms"] = round(region_ms(lambda: ops.render_map_raw(pts, nrm, col, counts, pose, K1, H, W)), 4)
    r["render_map_backward_ms"] = round(region_ms(lambda: ops.render_map_backward_raw(pts, counts, pose, index, g_d, g_p, g_n, g_c)), 4)
    r["torch_chain_ms"] = round(region_ms(lambda: torch_chain(pts, nrm, col, counts, pose, K1, H, W)), 4)
    fb = region_ms(torch_fwd_bwd)
    r["torch_chain_fwd_bwd_ms"] = round(fb, 4)
    r["torch_chain_over_render_map"] = {"forward": round(r["torch_chain_ms"] / r["render_map_ms"], 2),
                                        "forward_backward": round(fb / (r["render_map_ms"] + r["render_map_backward_ms"]), 2)}
    r["render_map_algorithmic_bytes"] = {"per_map_row": 12, "per_candidate": 8, "per_pixel": 8 + 8 + 8 + 72,
                                         "total": 12 * N + 8 * int(n_act.item()) + 96 * H * W}
    line = json.dumps(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
