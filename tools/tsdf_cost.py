#!/usr/bin/env python3
"""Cost of the TSDF volume (gs_tsdf_integrate / gs_tsdf_extract and their reverse passes): one JSON line, medians of 5 regions
(host clock around a device synchronise), on a 256^3 volume of 1 cm voxels around the synthetic wall and 30 frames at 640x480.
  (a) integrate: the 30 frames in one call (one launch: the volume is read and written once);
  (b) integrate: the same frames as 30 single-frame calls (the volume is read and written 30 times);
  (c) the torch-op chain a user would write today for (b): centres, transform, projection, gather, where;
  (d) extract: the sizing call (cap = 0), then the rows; and through TSDFVolume.extract_pointcloud (with its host synchronisation);
  (e) both reverse passes (integrate: all four adjoints; extract: both).
Also the algorithmic bytes of (a) and (b) from the shapes: 20 B per voxel (tsdf, weight, colour) read and written per launch."""
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


def torch_frame(cent, tsdf, weight, color, depth, rgb, pose, K, H, W, trunc, maxw):
    """(c): one frame into the flat state (n,), (n,), (n, 3) with torch ops"""
    pc = (cent - pose[:3, 3]) @ pose[:3, :3]
    z = pc[:, 2]
    u, v = K[0, 0] * pc[:, 0] / z + K[0, 2], K[1, 1] * pc[:, 1] / z + K[1, 2]
    act = (z > 0) & (u > -1e-3) & (u < W - 0.999) & (v > -1e-3) & (v < H - 0.999)
    pix = v.round().clamp(0, H - 1).long() * W + u.round().clamp(0, W - 1).long()
    pix = torch.where(act, pix, torch.zeros_like(pix))
    d = depth.reshape(-1)[pix]
    sdf = d - z
    upd = act & (d > 0) & ~(sdf < -trunc)
    t = (sdf / trunc).clamp(max=1.0)
    den = weight + 1.0
    tsdf = torch.where(upd, (weight * tsdf + t) / den, tsdf)
    color = torch.where(upd[:, None], (weight[:, None] * color + rgb.reshape(-1, 3)[pix]) / den[:, None], color)
    weight = torch.where(upd, (weight + 1.0).clamp(max=maxw), weight)
    return tsdf, weight, color


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_cost.json"))
    a = ap.parse_args()
    H, W, L, n1, v = a.height, a.width, a.frames, a.dim, a.voxel
    c, d, K, P = (x.to(dev) for x in make_sequence(1, L, H, W, seed=7))
    frames = gs.RGBDImages(c, d, K, P)
    single = [gs.RGBDImages(c[:, l:l + 1].contiguous(), d[:, l:l + 1].contiguous(), K, P[:, l:l + 1].contiguous()) for l in range(L)]
    half = 0.5 * n1 * v
    origin = (-half + 0.15, -half, 2.0 - half)  # the wall z = 2 +- 0.3 in the middle, the camera path (x = 0 .. 0.3) centred
    new = lambda: gs.structures.TSDFVolume((n1, n1, n1), v, origin=origin, device=dev)
    vol = new()

    def chunked():
        return vol.integrate(frames)

    def one_by_one():
        out = new()
        for f in single:
            out.integrate(f, inplace=True)
        return out

    fused = chunked()
    assert all(torch.equal(x, y) for x, y in zip((fused.tsdf, fused.weight, fused.color), (lambda o: (o.tsdf, o.weight, o.color))(one_by_one())))
    nvox = n1 ** 3
    iz, iy, ix = torch.meshgrid(*(torch.arange(n1, device=dev, dtype=torch.float32) for _ in range(3)), indexing="ij")
    cent = torch.stack([origin[0] + (ix + 0.5) * v, origin[1] + (iy + 0.5) * v, origin[2] + (iz + 0.5) * v], -1).reshape(-1, 3)
    del iz, iy, ix

    def chain():
        t, w, col = torch.ones(nvox, device=dev), torch.zeros(nvox, device=dev), torch.zeros(nvox, 3, device=dev)
        for l in range(L):
            t, w, col = torch_frame(cent, t, w, col, d[0, l], c[0, l], P[0, l], K[0, 0], H, W, vol.trunc, vol.max_weight)
        return t, w, col

    t_chain, w_chain, _ = chain()
    same_w = float((w_chain.view_as(fused.weight) == fused.weight).float().mean())
    dt = float((t_chain.view_as(fused.tsdf) - fused.tsdf).abs().max())

    state = (fused.tsdf, fused.weight, fused.color, fused.origin, v, 1.0)
    counts = ops.tsdf_extract_raw(*state, cap=0)[4].tolist()
    cap = max(counts)
    rows = ops.tsdf_extract_raw(*state, cap=cap)
    g = torch.Generator(device=dev).manual_seed(1)
    g_t = torch.randn(fused.tsdf.shape, device=dev, generator=g)
    g_c = torch.randn(fused.color.shape, device=dev, generator=g)
    g_p, g_k = (torch.randn(1, cap, 3, device=dev, generator=g) for _ in range(2))
    g_depth = ops.tsdf_integrate_backward_raw(d, K, P, vol.weight, vol.origin, v, vol.trunc, vol.max_weight, g_t, g_c)[2]

    r = {"tool": "tsdf_cost", "regions": REGIONS, "device": torch.cuda.get_device_name(0), "frames": L, "image": [H, W],
         "dims": [n1, n1, n1], "voxel_size": v, "voxels": nvox, "voxels_observed": int((fused.weight > 0).sum()),
         "surface_points": counts[0], "depth_pixels_with_gradient": int((g_depth != 0).sum()),
         "torch_chain_weight_agreement": round(same_w, 6), "torch_chain_tsdf_max_abs_diff": dt}
    r["integrate_chunked_ms"] = round(region_ms(chunked, 5), 4)
    r["integrate_single_frame_calls_ms"] = round(region_ms(one_by_one, 2), 4)
    r["torch_chain_single_frames_ms"] = round(region_ms(chain, 1), 4)
    r["extract_count_ms"] = round(region_ms(lambda: ops.tsdf_extract_raw(*state, cap=0), 5), 4)
    r["extract_rows_ms"] = round(region_ms(lambda: ops.tsdf_extract_raw(*state, cap=cap), 5), 4)
    r["extract_pointcloud_ms"] = round(region_ms(lambda: fused.extract_pointcloud(), 5), 4)
    r["integrate_backward_ms"] = round(region_ms(
        lambda: ops.tsdf_integrate_backward_raw(d, K, P, vol.weight, vol.origin, v, vol.trunc, vol.max_weight, g_t, g_c), 2), 4)
    r["extract_backward_ms"] = round(region_ms(lambda: ops.tsdf_extract_backward_raw(fused.tsdf, fused.color, v, rows[3], rows[4], g_p, g_k), 5), 4)
    r["ratios"] = {"single_frame_calls_over_chunked": round(r["integrate_single_frame_calls_ms"] / r["integrate_chunked_ms"], 2),
                   "torch_chain_over_single_frame_calls": round(r["torch_chain_single_frames_ms"] / r["integrate_single_frame_calls_ms"], 2),
                   "torch_chain_over_chunked": round(r["torch_chain_single_frames_ms"] / r["integrate_chunked_ms"], 2)}
    state_bytes = 2 * 20 * nvox  # tsdf + weight + 3 colours, read and written
    r["algorithmic_bytes"] = {"chunked": state_bytes, "single_frame_calls": L * state_bytes}
    r["algorithmic_GBps"] = {"chunked": round(state_bytes / r["integrate_chunked_ms"] / 1e6, 1),
                             "single_frame_calls": round(L * state_bytes / r["integrate_single_frame_calls_ms"] / 1e6, 1)}
    print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
