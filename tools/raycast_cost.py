#!/usr/bin/env python3
"""Cost of ray casting the TSDF volume (gs_tsdf_raycast and its reverse pass) and of one KinectFusion frame: one JSON line,
medians of 5 regions (host clock around a device synchronise), on the workload of tools/tsdf_cost.py: a 256^3 volume of 1 cm
voxels around the synthetic wall, fused from 30 frames at 640x480.
  (a) one cast at full resolution (307 k rays, step = trunc / 2), and at stride 4;
  (b) its reverse pass (g_depth and g_rgb given; the fold's workspace is 68 B per voxel with colours);
  (c) one KinectFusion frame (dsratio = 4): cast at stride 4 from the previous pose, ICP against it, integrate;
  (d) the yardstick a user had before for a view of the volume: extract_pointcloud + ops.render_map of the extracted cloud.
Also the samples a ray visits inside the box, from the shapes, and the hits."""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.slam import KinectFusion
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_cost.json"))
    a = ap.parse_args()
    H, W, L, n1, v = a.height, a.width, a.frames, a.dim, a.voxel
    c, d, K, P = (x.to(dev) for x in make_sequence(1, L, H, W, seed=7))
    half = 0.5 * n1 * v
    origin = (-half + 0.15, -half, 2.0 - half)  # tsdf_cost.py's volume
    slam = KinectFusion(dims=(n1, n1, n1), voxel_size=v, origin=origin, odom="icp", dsratio=4, device=dev)
    vol = slam.new_volume(1).integrate(gs.RGBDImages(c, d, K, P))  # tsdf_cost.py's volume: all the frames fused
    pose = P[:, L - 2:L - 1].contiguous()  # the camera of the cast; the KinectFusion frame tracks the last frame from it
    step = 0.5 * vol.trunc
    state = (vol.tsdf, vol.weight, vol.color, vol.origin, v, K, pose, H, W)

    depth, normal, rgb, k_end = ops.tsdf_raycast_raw(*state, 1, step)
    g = torch.Generator(device=dev).manual_seed(1)
    g_d, g_c = torch.randn(depth.shape, device=dev, generator=g), torch.randn(rgb.shape, device=dev, generator=g)
    g_t, _ = ops.tsdf_raycast_backward_raw(*state, 1, step, 1.0, k_end, g_d, g_c)

    prev = gs.RGBDImages(c[:, L - 2:L - 1], d[:, L - 2:L - 1], K, pose)
    live = lambda: gs.RGBDImages(c[:, L - 1:], d[:, L - 1:], K)
    counts = vol.extract_pointcloud()._counts

    def yardstick():
        pc = vol.extract_pointcloud()
        return ops.render_map(pc.points_padded, pc.normals_padded, pc.colors_padded, pc._counts_i32(), pose[:, 0].contiguous(),
                              K[:, 0].contiguous(), H, W)

    r = {"tool": "raycast_cost", "regions": REGIONS, "device": torch.cuda.get_device_name(0), "frames_fused": L, "image": [H, W],
         "dims": [n1, n1, n1], "voxel_size": v, "trunc": vol.trunc, "step": step, "rays": H * W, "hits": int((k_end > 0).sum()),
         "samples_per_ray_inside_the_box_at_most": int(3 * n1 * v / step) + 2, "mean_ending_sample_of_a_hit": float(k_end[k_end > 0].float().mean()),
         "voxels_with_gradient": int((g_t != 0).sum()), "surface_points_extracted": counts[0],
         "backward_workspace_bytes": ops.ws_bytes("gs_tsdf_raycast_backward_ws_bytes", 1, n1, n1, n1, 1)}
    r["cast_ms"] = round(region_ms(lambda: ops.tsdf_raycast_raw(*state, 1, step), 10), 4)
    r["cast_stride4_ms"] = round(region_ms(lambda: ops.tsdf_raycast_raw(*state, 4, step), 10), 4)
    r["cast_backward_ms"] = round(region_ms(lambda: ops.tsdf_raycast_backward_raw(*state, 1, step, 1.0, k_end, g_d, g_c), 3), 4)
    r["kinectfusion_frame_ms"] = round(region_ms(lambda: slam.step(vol, live(), prev), 3), 4)
    r["raycast_pointcloud_stride4_ms"] = round(region_ms(lambda: vol.raycast_pointcloud(K, pose, H, W, stride=4), 5), 4)
    r["integrate_one_frame_ms"] = round(region_ms(lambda: vol.integrate(prev), 5), 4)
    r["extract_pointcloud_plus_render_map_ms"] = round(region_ms(yardstick, 3), 4)
    r["ratios"] = {"yardstick_over_cast": round(r["extract_pointcloud_plus_render_map_ms"] / r["cast_ms"], 2)}
    print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
