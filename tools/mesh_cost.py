#!/usr/bin/env python3
"""Cost of the triangle-mesh extraction (gs_tsdf_faces, TSDFVolume.extract_mesh) beside the point extraction it builds on
(gs_tsdf_extract, TSDFVolume.extract_pointcloud): one JSON line, on a 256^3 volume of 1 cm voxels integrated from the synthetic
sequence (the README's example volume).  Every figure is the median of RUNS single calls after WARMUP calls, each timed with a
pair of device events; the whole-method figures (extract_pointcloud, extract_mesh) include their host synchronisation and are
timed on the host clock around a device synchronise.
  faces_count_ms      gs_tsdf_faces with fcap = 0: count and scan (streams tsdf, and weight on the surface's shell)
  faces_rows_ms       gs_tsdf_faces with the rows: memset, count, scan, ordered write (binary search of the edge list)
  extract_count_ms    gs_tsdf_extract with cap = 0, extract_rows_ms with the rows: the yardstick
The achieved bytes per second are quoted against the volume's 8 B per voxel (tsdf and weight, read once)."""
import argparse, json, os, statistics, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.synthetic import make_sequence_cached as make_sequence

dev = "cuda:0"


def event_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def host_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the commit the figures are taken at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cost.json"))
    a = ap.parse_args()
    H, W, L, n1, v = a.height, a.width, a.frames, a.dim, a.voxel
    c, d, K, P = (x.to(dev) for x in make_sequence(1, L, H, W, seed=7))
    half = 0.5 * n1 * v
    origin = (-half + 0.15, -half, 2.0 - half)  # tools/tsdf_cost.py's volume: the wall z = 2 +- 0.3 in the middle
    vol = gs.structures.TSDFVolume((n1, n1, n1), v, origin=origin, device=dev).integrate(gs.RGBDImages(c, d, K, P))
    nvox = n1 ** 3
    state = (vol.tsdf, vol.weight, vol.color, vol.origin, v, 1.0)
    n_points = ops.tsdf_extract_raw(*state, cap=0)[4]
    n_faces = ops.tsdf_faces_raw(vol.tsdf, vol.weight, 1.0, None, None, fcap=0)[1]
    vcap, fcap = int(n_points.max()), int(n_faces.max())
    rows = ops.tsdf_extract_raw(*state, cap=vcap)
    edge = rows[3]
    faces, _ = ops.tsdf_faces_raw(vol.tsdf, vol.weight, 1.0, edge, n_points, fcap=fcap, points_fit=True)
    assert int(faces.min()) >= 0 and int(faces.max()) < vcap
    mesh = vol.extract_mesh()

    r = {"tool": "mesh_cost", "commit": a.commit or commit(), "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
         "frames": L, "image": [H, W], "dims": [n1, n1, n1], "voxel_size": v, "voxels": nvox,
         "voxels_observed": int((vol.weight > 0).sum()), "vertices": vcap, "faces": fcap,
         "surface_area_m2": float(mesh.surface_area()[0])}
    figures = {
        "extract_count_ms": (event_ms, lambda: ops.tsdf_extract_raw(*state, cap=0)),
        "extract_rows_ms": (event_ms, lambda: ops.tsdf_extract_raw(*state, cap=vcap)),
        "faces_count_ms": (event_ms, lambda: ops.tsdf_faces_raw(vol.tsdf, vol.weight, 1.0, None, None, fcap=0)),
        "faces_rows_ms": (event_ms, lambda: ops.tsdf_faces_raw(vol.tsdf, vol.weight, 1.0, edge, n_points, fcap=fcap, points_fit=True)),
        "extract_pointcloud_ms": (host_ms, lambda: vol.extract_pointcloud()),
        "extract_mesh_ms": (host_ms, lambda: vol.extract_mesh()),
    }
    for name, (timer, fn) in figures.items():
        med, lo, hi = timer(fn, a.runs, a.warmup)
        r[name] = round(med, 4)
        r[name.replace("_ms", "_min_max_ms")] = [round(lo, 4), round(hi, 4)]
    r["volume_bytes_8_per_voxel"] = 8 * nvox
    r["GBps_against_8B_per_voxel"] = {k: round(8 * nvox / r[k] / 1e6, 1) for k in ("extract_count_ms", "extract_rows_ms", "faces_count_ms", "faces_rows_ms")}
    r["ratios"] = {"faces_count_over_extract_count": round(r["faces_count_ms"] / r["extract_count_ms"], 2),
                   "faces_rows_over_extract_rows": round(r["faces_rows_ms"] / r["extract_rows_ms"], 2),
                   "extract_mesh_over_extract_pointcloud": round(r["extract_mesh_ms"] / r["extract_pointcloud_ms"], 2)}
    print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
