#!/usr/bin/env python3
"""Cost of gs.metrics.chamfer_distance: one JSON line, medians of 5 regions, GPU time per call of the forward and of
forward + backward, on
  (a) two image-ordered ~300 k-point clouds: the valid pixels of two 640x480 frames of make_sequence, and
  (b) the same two clouds with their rows shuffled by a seeded permutation,
each with the targets scanned in cell-grid order (reorder=True) and as they come (reorder=False).  Beside them what the
package offered before gs.metrics on the same inputs: ops.knn1_raw both ways, knn1_unpack and torch reductions (forward),
and torch autograd through the gathers by the returned indices (forward + backward).  The `reorder=None` default of
gradslam_amd/metrics/maps.py is the setting whose slower case of (a) and (b) is faster ("default_choice" below)."""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.structures.utils import pointclouds_from_rgbdimages
from gradslam_amd.synthetic import make_sequence_cached as make_sequence

dev = "cuda:0"
REGIONS = 5


def region_ms(fn):
    """median over REGIONS of the mean time of back-to-back calls (host clock around a device synchronise); the number of
    calls per region is chosen from one timed call so that a region lasts ~0.3 s (2 .. 20 calls)"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = min(max(int(0.3 / max(time.perf_counter() - t0, 1e-6)), 2), 20)
    out = []
    for _ in range(REGIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return round(statistics.median(out), 4), calls


def knn_chain(a, b, grad):
    """the package without gs.metrics: two gs_knn1 calls, unpack, torch reductions; with `grad` the distances are rebuilt
    from gathers by the returned indices so that autograd reaches both clouds"""
    d2ab, iab = ops.knn1_unpack(ops.knn1_raw(a.detach(), b.detach()))
    d2ba, iba = ops.knn1_unpack(ops.knn1_raw(b.detach(), a.detach()))
    if not grad:
        return d2ab.mean() + d2ba.mean()
    return ((a - b[iab]) ** 2).sum(-1).mean() + ((b - a[iba]) ** 2).sum(-1).mean()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_cost.json"))
    args = ap.parse_args()
    H, W = args.height, args.width
    c, d, K, P = (x.to(dev) for x in make_sequence(1, 2, H, W, seed=11))
    frames = [pointclouds_from_rgbdimages(gs.RGBDImages(c[:, s:s + 1], d[:, s:s + 1], K, P[:, s:s + 1])).points_padded[0].contiguous()
              for s in (0, 1)]
    g = torch.Generator().manual_seed(12)
    shuffled = [x[torch.randperm(x.shape[0], generator=g).to(dev)].contiguous() for x in frames]
    r = {"tool": "metrics_cost", "regions": REGIONS, "device": torch.cuda.get_device_name(0), "image": [H, W],
         "points": [int(x.shape[0]) for x in frames]}

    def fwd_bwd(pa, pb, reorder):
        la, lb = pa.clone().requires_grad_(True), pb.clone().requires_grad_(True)
        gs.metrics.chamfer_distance(gs.Pointclouds(la.unsqueeze(0)), gs.Pointclouds(lb.unsqueeze(0)), reorder=reorder).backward()
        return la.grad, lb.grad

    def knn_fwd_bwd(pa, pb):
        la, lb = pa.clone().requires_grad_(True), pb.clone().requires_grad_(True)
        knn_chain(la, lb, True).backward()

    values = {}
    for case, (pa, pb) in (("image_ordered", frames), ("shuffled", shuffled)):
        A, Bc = gs.Pointclouds(pa.unsqueeze(0)), gs.Pointclouds(pb.unsqueeze(0))
        A._counts_i32(), Bc._counts_i32()
        for reorder in (True, False):
            tag = "%s/%s" % (case, "bucketed" if reorder else "unbucketed")
            values[tag] = float(gs.metrics.chamfer_distance(A, Bc, reorder=reorder))
            fwd, calls = region_ms(lambda: gs.metrics.chamfer_distance(A, Bc, reorder=reorder))
            fb, calls_fb = region_ms(lambda: fwd_bwd(pa, pb, reorder))
            r[tag] = {"forward_ms": fwd, "forward_backward_ms": fb, "calls_per_region": [calls, calls_fb]}
        values[case + "/knn1_chain"] = float(knn_chain(pa, pb, False))
        fwd, calls = region_ms(lambda: knn_chain(pa, pb, False))
        fb, calls_fb = region_ms(lambda: knn_fwd_bwd(pa, pb))
        r[case + "/knn1_chain"] = {"forward_ms": fwd, "forward_backward_ms": fb, "calls_per_region": [calls, calls_fb]}
    r["chamfer_values"] = values
    worst = {k: max(r["image_ordered/" + k]["forward_backward_ms"], r["shuffled/" + k]["forward_backward_ms"])
             for k in ("bucketed", "unbucketed")}
    r["slower_case_forward_backward_ms"] = worst
    r["default_choice"] = "reorder=True" if worst["bucketed"] <= worst["unbucketed"] else "reorder=False"
    line = json.dumps(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
