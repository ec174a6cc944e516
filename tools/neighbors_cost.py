#!/usr/bin/env python3
"""Cost of the exact K nearest neighbours (gs_knn), their reverse pass and the normals against the torch chain a user would
write: one JSON line, medians of 5 regions, host clock around a device synchronise (launches included).
  (a) ops.knn_raw with K = 16 as a self-query on one 640x480 frame's cloud (~300 k rows), image-ordered and shuffled, and on
      the map a 100-frame PointFusion run leaves behind (~2 M rows); ops.knn + backward; Pointclouds.estimate_normals on both;
  (b) the yardstick at the largest size it manages (--torch-rows, default 32768 rows of the frame's cloud): chunked
      torch.cdist + topk, gathers, autograd backward through the gathered distances, torch.linalg.eigh on batched 3x3."""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.synthetic import make_sequence_cached as make_sequence

dev = "cuda:0"
REGIONS = 5


def region_ms(fn, calls):
    """median over REGIONS of the mean time of `calls` back-to-back calls (host clock around a device synchronise)"""
    fn()
    out = []
    for _ in range(REGIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return statistics.median(out)


def torch_knn(x, K, chunk=4096):
    """(b): squared distances and rows of the K nearest, differentiable w.r.t. x (N, 3)"""
    idx = torch.cat([torch.cdist(x[i:i + chunk].detach(), x.detach()).topk(K, dim=1, largest=False).indices
                     for i in range(0, x.shape[0], chunk)])
    return ((x.unsqueeze(1) - x[idx]) ** 2).sum(-1), idx


def torch_normals(x, idx):
    nb = x[idx].double()
    d = nb - nb.mean(1, keepdim=True)
    C = d.transpose(1, 2) @ d / idx.shape[1]
    n = torch.linalg.eigh(C).eigenvectors[:, :, 0]
    return torch.where(((n * -x.double()).sum(-1, keepdim=True) < 0), -n, n).float()


def measure(name, pts, K, r, calls):
    cnt = torch.full((1,), pts.shape[1], dtype=torch.int32, device=dev)
    pc = gs.Pointclouds(pts)
    g = torch.randn(1, pts.shape[1], K, device=dev)

    def fwd_bwd():
        leaf = pts.clone().requires_grad_(True)
        d2, _ = ops.knn(leaf, leaf, cnt, cnt, K)
        (d2 * g).sum().backward()

    r[name] = {"rows": int(pts.shape[1]),
               "knn_ms": round(region_ms(lambda: ops.knn_raw(pts, pts, cnt, cnt, K), calls), 4),
               "knn_forward_backward_ms": round(region_ms(fwd_bwd, calls), 4),
               "estimate_normals_ms": round(region_ms(lambda: pc.estimate_normals(K), calls), 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--torch-rows", type=int, default=32768)
    ap.add_argument("--skip-map", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors_cost.json"))
    a = ap.parse_args()
    K, H, W = a.K, 480, 640
    c, d, Kc, P = (x.to(dev) for x in make_sequence(1, a.frames, H, W, seed=7))
    frame = gs.structures.utils.pointclouds_from_rgbdimages(gs.RGBDImages(c[:, :1], d[:, :1], Kc, P[:, :1])).points_padded.contiguous()
    r = {"tool": "neighbors_cost", "regions": REGIONS, "device": torch.cuda.get_device_name(0), "K": K}
    measure("frame_image_order", frame, K, r, 5)
    measure("frame_shuffled", frame[:, torch.randperm(frame.shape[1], device=dev)].contiguous(), K, r, 5)
    if not a.skip_map:
        pcs, _ = gs.slam.PointFusion(odom="gt", device=dev)(gs.RGBDImages(c, d, Kc, P))
        measure("map_{}_frames".format(a.frames), pcs.points_padded.contiguous(), K, r, 2)

    n = min(a.torch_rows, frame.shape[1])
    sub = frame[:, torch.randperm(frame.shape[1], device=dev)[:n]].contiguous()
    x = sub[0]
    gt = torch.randn(n, K, device=dev)

    def torch_fwd_bwd():
        leaf = x.clone().requires_grad_(True)
        d2, _ = torch_knn(leaf, K)
        (d2 * gt).sum().backward()

    _, tidx = torch_knn(x, K)
    t = {"rows": n,
         "knn_ms": round(region_ms(lambda: torch_knn(x, K), 3), 4),
         "knn_forward_backward_ms": round(region_ms(torch_fwd_bwd, 3), 4),
         "normals_given_neighbours_ms": round(region_ms(lambda: torch_normals(x, tidx), 3), 4)}
    r["torch_chain"] = t
    measure("ours_at_torch_rows", sub, K, r, 5)
    line = json.dumps(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
