#!/usr/bin/env python3
"""bench.py -- RGB-D frames/sec of the per-frame point-to-plane ICP hot path on MI355X.

Workload (BASELINE.json configs[1], "c2"): synthetic TUM-shape 640x480 RGB-D, batch 1 per GPU,
dsratio 4, 10 ICP iterations.  One STEP = localising one live frame against the map, inputs already
resident in HBM: depth -> vertex/normal maps (local+global), ds-grid source cloud, active-map-point
projection of the ~300 k-point map + ds-grid target cloud, 10-iteration LM point-to-plane ICP
(exact 1-NN association, 6x6 Gauss-Newton reduce/solve, SE(3) exp, accept/reject on device), pose
composition -- i.e. ICPSLAM._localize of the reference (slam/icpslam.py:238-247), nothing skipped.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]   (N>1: launched by torch.distributed.run)

Prints ONE JSON line on rank 0.  A plain run sets the workload up, runs W warm-up steps, times ONE region of exactly K
steps and reports it: `value` (frames/s) and `ms_per_step` come from that region.  --dump-outputs DIR then writes what
the last timed step handed back (the pose and the live frame's local vertex / normal maps) as DIR/<name>.npy, float32;
the inputs are seeded, so two runs with the same arguments see the same frames.
--full adds what takes runs of its own: `value` becomes the MEDIAN of GS_BENCH_REPEATS (default 5) timed regions of
exactly K steps each (one region of 20 steps is a 4.6 ms sample); `repeats_ms_per_step` lists them all.
`roofline` is the HBM roofline of the ICP associate+reduce kernel (J) at a size that streams from HBM (2^24 points,
40 algorithmic bytes per point), timed live in a second timed region -- the only size at which an HBM fraction is
physically meaningful; its `traffic` is NOT measured in this run: it comes from the committed
PMC passes (profiles/).  `roofline_timed_region` describes the dominant kernel of the c2 timed region itself (the
fused step + association + linearise kernel, L2-resident at this size): launch time from HIP events recorded on the
launch stream inside the C library (gs_profile_*), executed work (VALU instructions, issue utilisation) from the
committed counter passes.  `aux` carries the other sizes SURVEY 8(d) asks for (ds = 1, 1296x968), the fusion update's
HBM view at ~1 M map points and BASELINE configs[2] at full length (200 frames, forward and forward + backward).
`cpu_baseline` times the CPU oracle on bounded samples of the same workloads on the host cores (rank 0, N=1 only;
--no-cpu-baseline leaves it out).
"""
import argparse
import ctypes
import gc
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W, DS, ITERS = 480, 640, 4, 10
N_LIVE = 4  # distinct live frames cycled through (fresh RGBDImages each step: nothing is cached)


def build_workload(gs, dev, seed):
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    c, d, K, P = make_sequence(1, 1 + N_LIVE, H, W, seed=seed)
    c, d, K, P = c.to(dev), d.to(dev), K.to(dev), P.to(dev)
    slam = gs.slam.PointFusion(odom="icp", dsratio=DS, numiters=ITERS, device=dev)
    frames = gs.RGBDImages(c, d, K, P)
    with torch.no_grad():
        f0 = frames[:, 0]
        world_map, _ = slam.step(gs.Pointclouds(device=dev), f0, None)  # map after frame 0
    lives = [(c[:, s:s + 1].contiguous(), d[:, s:s + 1].contiguous()) for s in range(1, 1 + N_LIVE)]
    # prime the path (lazy code-object loading, allocator, the library's launch-mode decision): part of building
    # the workload, so that even a very short --warmup never times one-off initialisation
    with torch.no_grad():
        for i in range(int(os.environ.get("GS_BENCH_PRIME", "8"))):
            one_step(gs, slam, world_map, f0, lives[i % N_LIVE], K)
    torch.cuda.synchronize()
    return slam, world_map, f0, lives, K, (c, d, K, P)


def one_step(gs, slam, world_map, prev, live_cd, K, keep=None):
    live = gs.RGBDImages(live_cd[0], live_cd[1], K)  # fresh object: maps are recomputed every step
    if keep is not None:
        keep.append(live)  # the step leaves the live frame's local maps on it: outputs too (--dump-outputs)
    return slam._localize(world_map, live, prev)


def dump_outputs(out_dir, pose, live):
    """--dump-outputs: what the last timed step handed back -- the pose (B,1,4,4) and the local vertex / normal maps
    (B,1,H,W,3) the fused step left on the live frame -- as float32 .npy files (7.4 MB in all at 640x480)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    for name, t in (("pose", pose), ("vertex_map", live.vertex_map), ("normal_map", live.normal_map)):
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().to(torch.float32).cpu().numpy())


def prof_read(nv, tag):
    n, ms = ctypes.c_long(0), ctypes.c_double(0.0)
    nv.lib().gs_profile_read(tag, ctypes.byref(n), ctypes.byref(ms))
    return n.value, ms.value


def hbm_roofline_linearize(gs, dev, n_pts=1 << 24, reps=20):
    """J (linearise + 6x6 reduce) on 2^24 points with image-order-coherent associations: 40
    algorithmic bytes per source point (src 12 + idx 4 + gathered tgt 12 + gathered normal 12)."""
    from gradslam_amd import ops
    from gradslam_amd._native import call, ptr, stream, workspace, ws_bytes

    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.rand((n_pts, 3), device=dev, generator=g)
    tgt = src + 0.01
    nrm = torch.nn.functional.normalize(torch.rand((n_pts, 3), device=dev, generator=g), dim=-1)
    idx = torch.arange(n_pts, device=dev, dtype=torch.int64)
    jitter = torch.randint(-8, 9, (n_pts,), device=dev, generator=g)
    idx = (idx + jitter).clamp_(0, n_pts - 1)
    d2 = torch.full((n_pts,), 1e-4, device=dev).view(torch.int32).to(torch.int64)
    best = (d2 << 32) | idx
    out = torch.empty(44, device=dev)
    ws = workspace(ws_bytes("gs_icp_linearize_ws_bytes", n_pts), dev, "linearize")
    d_n = ops.dev_int(n_pts, dev)
    run = lambda: call("gs_icp_linearize", ptr(src), ptr(d_n), n_pts, ptr(tgt), ptr(nrm), ptr(best), -1.0, ptr(out), ptr(ws),
                       ws.numel(), stream())
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:  # torch's current stream IS the stream the kernel is launched on (stream())
        a.record()
        run()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    med = ms[len(ms) // 2]
    kept = [m for m in ms if m <= 3.0 * med]  # a pre-empted launch (tens of ms, seen once) is not the kernel's duration
    avg = sum(kept) / len(kept)
    alg = 40.0 * n_pts
    ach = alg / (avg * 1e-3) / 1e9
    traffic, traffic_file, traffic_commit = None, None, None
    for name in ("r03_pmc_traffic.json", "r01_pmc_traffic.json"):  # HBM bytes per launch from the committed PMC passes (newest first)
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                pj = json.load(f)
            if pj.get("n_points") == n_pts:
                traffic, traffic_file, traffic_commit = pj["linearize_k"]["hbm_bytes_per_launch"], name, pj.get("commit", "round 1")
                break
        except Exception:
            pass
    return {"kernel": "gs_icp_linearize = linearize_k + finalize44_k (J: gather associated target point + normal, "
                      "Jacobian row, 6x6 / 6 / 1 reduce)", "bound": "hbm", "achieved": round(ach, 1),
            "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4), "traffic": traffic,
            "traffic_source": "profiles/{}: separate --pmc FETCH_SIZE / WRITE_SIZE passes over this kernel at this size (gfx950 FETCH "
                              "correction calibrated on transform_k) taken at commit {} -- read from the committed profile, NOT measured "
                              "in this run".format(traffic_file, traffic_commit),
            "n_points": n_pts,
            "bytes_per_point": 40, "algorithmic_bytes_per_launch": alg, "avg_launch_ms": round(avg, 4), "launches": len(kept),
            "launches_discarded_as_preempted": len(ms) - len(kept),
            "scope": "streaming-size launch (2^24 source points, image-coherent associations), timed live with HIP "
                     "events on the launch stream in a second timed region of this run: the c2 timed region's own "
                     "kernels move <1 MB per launch (L2-resident, launch-bound), see roofline_timed_region; the loops "
                     "themselves never launch this kernel (J is fused into the association kernel's epilogue), it serves "
                     "gauss_newton_solve and the per-op autograd formulation; idx = arange +- 8 is a best-case gather",
            "note": "peak = 8.0 TB/s HBM3E spec (6.29 TB/s is the measured float4-copy ceiling, i.e. frac of achievable "
                    "= achieved / 6290)"}


def hbm_linearize_real_associations(gs, dev, side=4096, reps=10):
    """The same kernel (J at 2^24 points) with REAL associations instead of `arange +- 8`: source = a side x side depth image
    of the synthetic wall back-projected (image order, like the ICP clouds), target = the same wall seen from a camera moved
    by a few pixels' worth and slightly rotated, nearest neighbours from an actual exact search (gs_knn1).  The gather then
    has the locality a real association has -- neighbours of neighbouring pixels, with the row-to-row jumps and the local
    disorder of a real search -- not the best case."""
    from gradslam_amd import ops
    from gradslam_amd._native import call, ptr, stream, workspace, ws_bytes

    n_pts = side * side
    f = 525.0 * side / 640.0
    cxy = (side - 1) / 2.0
    v, u = torch.meshgrid(torch.arange(side, device=dev, dtype=torch.float32), torch.arange(side, device=dev, dtype=torch.float32), indexing="ij")
    wall = lambda x, y: 2.0 + 0.3 * torch.sin(2.0 * x) * torch.cos(2.0 * y)

    def cloud(du, dv, rot):
        uu, vv = u + du, v + dv
        x, y = (uu - cxy) / f * 2.0, (vv - cxy) / f * 2.0
        z = wall(x, y)
        p = torch.stack([(uu - cxy) / f * z, (vv - cxy) / f * z, z], -1).reshape(-1, 3)
        R = torch.tensor([[math.cos(rot), 0, math.sin(rot)], [0, 1, 0], [-math.sin(rot), 0, math.cos(rot)]], device=dev)
        return (p @ R.t()).contiguous()

    tgt = cloud(0.0, 0.0, 0.0)
    src = cloud(2.37, -1.21, 0.0007)
    nrm = torch.nn.functional.normalize(torch.stack([-0.6 * torch.ones_like(tgt[:, 0]), 0.1 * torch.ones_like(tgt[:, 0]), -torch.ones_like(tgt[:, 0])], -1), dim=-1).contiguous()
    t0 = time.perf_counter()
    best = ops.knn1_raw(src, tgt)
    torch.cuda.synchronize()
    t_search = time.perf_counter() - t0
    idx = best & 0xffffffff
    jump = (idx[1:] - idx[:-1]).abs().float()
    out = torch.empty(44, device=dev)
    ws = workspace(ws_bytes("gs_icp_linearize_ws_bytes", n_pts), dev, "linearize")
    d_n = ops.dev_int(n_pts, dev)
    run = lambda: call("gs_icp_linearize", ptr(src), ptr(d_n), n_pts, ptr(tgt), ptr(nrm), ptr(best), -1.0, ptr(out), ptr(ws),
                       ws.numel(), stream())
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        run()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    med = ms[len(ms) // 2]
    kept = [m for m in ms if m <= 3.0 * med]
    avg = sum(kept) / len(kept)
    alg = 40.0 * n_pts
    return {"n_points": n_pts, "avg_launch_ms": round(avg, 4), "achieved": round(alg / (avg * 1e-3) / 1e9, 1), "unit": "GB/s",
            "frac": round(alg / (avg * 1e-3) / 8e12, 4), "bound": "hbm", "peak": 8000.0,
            "association": {"search_s": round(t_search, 3), "median_index_jump": float(jump.median()), "p99_index_jump": float(jump.quantile(0.99)),
                            "monotone_fraction": round(float((idx[1:] >= idx[:-1]).float().mean()), 4)},
            "note": "gs_icp_linearize at 2^24 points with nearest neighbours from an exact search of a shifted, slightly rotated view "
                    "of the same surface ({}x{} image order): 40 algorithmic bytes per point, HIP events on the launch stream".format(side, side)}


def aux_pointfusion(gs, dev, raw, n_frames=30):
    """Auxiliary, NOT part of `value`: forward frames/s of the full PointFusion step (localise + map update,
    BASELINE configs[2] shape) over a short synthetic sequence, map growing from empty."""
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    c, d, K, P = make_sequence(1, n_frames, H, W, seed=100)
    frames = gs.RGBDImages(c.to(dev), d.to(dev), K.to(dev), P.to(dev))
    slam = gs.slam.PointFusion(odom="icp", dsratio=DS, numiters=ITERS, device=dev)
    with torch.no_grad():
        slam(gs.RGBDImages(c[:, :3].to(dev), d[:, :3].to(dev), K.to(dev), P[:, :3].to(dev)))  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pcs, poses = slam(frames)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    err = float((poses.cpu() - P).abs().max())
    out = {"pointfusion_c3_forward_fps": round(n_frames / dt, 2), "frames": n_frames,
           "final_map_points": int(pcs.num_points_per_pointcloud.item()), "pose_max_abs_err_vs_gt": round(err, 5),
           "note": "PointFusion(odom='icp') forward over a 640x480 synthetic sequence (arena-backed sequence driver: "
                   "localise + map update = two C calls per frame, one host sync per sequence), not part of `value`"}
    slam.streamed = False
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        slam(frames)
        torch.cuda.synchronize()
        out["pointfusion_c3_forward_fps_stepwise_api"] = round(n_frames / (time.perf_counter() - t0), 2)
    # forward + backward (BASELINE configs[2] asks for both), default odometry = gradicp, loss as in the golden vectors
    for rep in range(2):  # first pass warms the allocator
        leaves = [x.to(dev).clone().requires_grad_(True) for x in (c, d, K, P)]
        slam = gs.slam.PointFusion(odom="gradicp", dsratio=DS, numiters=ITERS, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pcs, poses = slam(gs.RGBDImages(*leaves))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        finite = all(bool(torch.isfinite(x.grad).all()) for x in leaves)
        del pcs, poses
    out.update({"pointfusion_c3_gradicp_fwd_ms_per_frame": round(1e3 * (t1 - t0) / n_frames, 3),
                "pointfusion_c3_gradicp_bwd_ms_per_frame": round(1e3 * (t2 - t1) / n_frames, 3),
                "pointfusion_c3_gradicp_fwd_bwd_fps": round(n_frames / (t2 - t0), 2), "grads_finite": finite})
    return out


def aux_association_sizes(gs, dev):
    """the association at ds = 1 (307 k x 307 k) and at the 1296x968 shape (ds = 4: 78 k x 78 k): one
    10-iteration LM loop, frame 1 against frame 0's cloud, timed with HIP events; ms per association = loop / 11."""
    from gradslam_amd import ops
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    out = {}
    for tag, (h, w, ds) in (("640x480_ds1", (480, 640, 1)), ("1296x968_ds4", (968, 1296, 4))):
        c, d, K, P = make_sequence(1, 2, h, w, seed=5)
        fr = gs.RGBDImages(c.to(dev), d.to(dev), K.to(dev), P[:, :1].repeat(1, 2, 1, 1).to(dev))
        with torch.no_grad():
            tgt = gs.odometry.icputils.downsample_rgbdimages(fr[:, 0], ds)
            src = gs.odometry.icputils.downsample_rgbdimages(fr[:, 1], ds)
            args = (src.points_list[0].contiguous(), tgt.points_list[0].contiguous(), tgt.normals_list[0].contiguous(),
                    torch.eye(4, device=dev), ITERS, 1e-8, None)
            ops.icp_device_loop(*args)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                ops.icp_device_loop(*args)
            e1.record()
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 3.0
        ns, nt = args[0].shape[0], args[1].shape[0]
        out[tag] = {"source_points": ns, "target_points": nt, "loop_ms": round(ms, 3), "ms_per_association": round(ms / (ITERS + 1), 4),
                    "J_algorithmic_bytes_per_association": 40 * ns}
    out["note"] = ("10-iteration LM loop (11 associations incl. the folded steps), image-ordered clouds without search hints "
                   "(gs_icp_point_to_plane), HIP events on the launch stream; the association is VALU / latency bound at these "
                   "sizes, the J bytes are listed for scale only")
    return out


def aux_fusion_update_roofline(gs, dev, n_frames=31):
    """HBM view of the PointFusion map update (gs_pointfusion_update) on a ~1 M-point map: algorithmic bytes per
    frame by SURVEY 8(d)'s formula -- 12 N (projection) + 32 P (table) + 48 P (similar + unique) + 120 U (merge) +
    52 HW (maps) -- over the measured time of the call (HIP events), as a fraction of 8 TB/s."""
    from gradslam_amd import ops
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    c, d, K, P = make_sequence(1, n_frames, H, W, seed=100)
    slam = gs.slam.PointFusion(odom="gt", dsratio=DS, numiters=ITERS, device=dev)
    with torch.no_grad():
        pcs, _ = slam(gs.RGBDImages(c[:, :-1].to(dev), d[:, :-1].to(dev), K.to(dev), P[:, :-1].to(dev)))
        n_map = int(pcs.num_points_per_pointcloud.item())
        cap = n_map + H * W
        mk = lambda x, w_: torch.cat([x, torch.zeros((1, H * W, w_), device=dev)], 1).contiguous()
        base = [mk(pcs.points_padded, 3), mk(pcs.normals_padded, 3), mk(pcs.colors_padded, 3), mk(pcs.features_padded, 1)]
        d_s, c_s = d[:, -1].to(dev).contiguous(), c[:, -1].to(dev).contiguous()
        Kd, Pd = K.to(dev), P[:, -1:].to(dev).contiguous()
        stats = torch.zeros(5, dtype=torch.int32, device=dev)
        times = []
        for rep in range(6):
            arrs = [x.clone() for x in base]
            counts = torch.tensor([n_map], dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.pointfusion_update_raw(d_s, c_s, Kd, Pd, arrs[0], arrs[1], arrs[2], arrs[3], counts, 0.05, math.cos(math.radians(20)), 0.6, stats)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        st = stats.tolist()
    ms = sorted(times[1:])[len(times[1:]) // 2]
    n_act, n_uni = st[0], st[1]
    alg = 12.0 * n_map + 32.0 * n_act + 48.0 * n_act + 120.0 * n_uni + 52.0 * H * W
    return {"map_points": n_map, "active_rows": n_act, "unique_rows": n_uni, "call_ms": round(ms, 4), "algorithmic_bytes_per_frame": alg,
            "achieved_GBps": round(alg / (ms * 1e-3) / 1e9, 1), "frac_of_8TBps": round(alg / (ms * 1e-3) / 8e12, 4),
            "note": "one gs_pointfusion_update call (7 launches: maps + alpha, table-free correspondence passes 1 / 2, in-place merge, "
                    "append count / write, finish) on a map of {} points (capacity {}), median of 5 HIP-event timings; bytes by "
                    "SURVEY.md 8(d), whose 32 B/row table and 48 B/row unique stage this chain no longer moves".format(n_map, cap)}


def aux_c3_full_length(gs, dev, n_frames=200):
    """BASELINE configs[2] in full: PointFusion on 200 frames of 640x480, batch 1 -- forward (odom 'icp' and 'gradicp')
    and forward + backward (gradicp, the loss of the golden vectors)."""
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    c, d, K, P = make_sequence(1, n_frames, H, W, seed=100)
    cd, dd, Kd, Pd = c.to(dev), d.to(dev), K.to(dev), P.to(dev)
    out = {"frames": n_frames}
    with torch.no_grad():
        for odom in ("icp", "gradicp"):
            slam = gs.slam.PointFusion(odom=odom, dsratio=DS, numiters=ITERS, device=dev)
            best = 0.0
            for rep in range(2):  # the first pass grows the allocator's pools to the 3.3 M-point arena
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pcs, poses = slam(gs.RGBDImages(cd, dd, Kd, Pd))
                torch.cuda.synchronize()
                best = max(best, n_frames / (time.perf_counter() - t0))
            out["forward_fps_" + odom] = round(best, 2)
            if odom == "icp":
                # the headline's localisation step in the state configs[2] lives in: the SAME call (ICPSLAM._localize, 10 LM
                # iterations) against the map after 200 frames, previous frame = frame 199 under its recovered pose
                prev = gs.RGBDImages(cd[:, -1:].contiguous(), dd[:, -1:].contiguous(), Kd, poses[:, -1:].contiguous())
                lives = [(cd[:, s:s + 1].contiguous(), dd[:, s:s + 1].contiguous()) for s in (n_frames - 1, n_frames - 2)]
                for i in range(6):
                    one_step(gs, slam, pcs, prev, lives[i % 2], Kd)
                torch.cuda.synchronize()
                reps = 50
                t0 = time.perf_counter()
                for i in range(reps):
                    one_step(gs, slam, pcs, prev, lives[i % 2], Kd)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / reps
                out["c2_on_dense_map"] = {"ms_per_step": round(1e3 * dt, 4), "frames_per_s": round(1.0 / dt, 1),
                                          "map_points": int(pcs.num_points_per_pointcloud.item()),
                                          "note": "the c2 step (`value`) against the map after {} frames instead of the one-frame map: "
                                                  "projection of every map point, a target of ~10 points per ds-grid pixel".format(n_frames)}
        out["final_map_points"] = int(pcs.num_points_per_pointcloud.item())
        del pcs, poses
    for rep in range(3):  # the first passes warm the allocator (7.7 GB of tapes per pass); the last one is reported
        gc.collect()
        leaves = [x.clone().requires_grad_(True) for x in (cd, dd, Kd, Pd)]
        slam = gs.slam.PointFusion(odom="gradicp", dsratio=DS, numiters=ITERS, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pcs, poses = slam(gs.RGBDImages(*leaves))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        finite = all(bool(torch.isfinite(x.grad).all()) for x in leaves)
        del pcs, poses, leaves, slam
    out.update({"gradicp_fwd_ms_per_frame": round(1e3 * (t1 - t0) / n_frames, 3), "gradicp_bwd_ms_per_frame": round(1e3 * (t2 - t1) / n_frames, 3),
                "gradicp_fwd_bwd_fps": round(n_frames / (t2 - t0), 2), "grads_finite": finite,
                "note": "forward: arena-backed sequence driver; forward + backward: one autograd node per sequence (taped arena "
                        "update, reverse pass over the frames), loss = poses.sum() + points.sum() + colors.mean()"})
    return out


def cpu_baseline(raw, n_frames=24):
    """The CPU oracle (kind 'port') on the same workload: localise live frames 1..n against the map (the c2 step of
    `value`), plus the two figures BASELINE.md section 3 plans beside it: ONE nearest-neighbour search of the c2 size
    on a single thread (pytorch3d / chamferdist's CPU search is a serial loop) and the full PointFusion step of
    configs[2] over 10 frames."""
    from oracle import fusion as ofu
    from oracle import icp as oicp
    from oracle import knn as oknn
    from oracle import slam as oslam
    from oracle.cloud import Cloud

    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    oknn.set_threads(cores)
    c, d, K, P = (x.cpu() for x in raw)
    f0 = ofu.make_frame(c[:, :1], d[:, :1], K, P[:, :1])
    cloud = ofu.update_map_fusion(Cloud(), f0, 0.05, math.cos(math.radians(20)), 0.6)
    t0 = time.perf_counter()
    for i in range(n_frames):
        s = 1 + i % N_LIVE
        live = ofu.make_frame(c[:, s:s + 1], d[:, s:s + 1], K, f0["pose"])
        oslam.localize(cloud, live, f0, "icp", DS, numiters=ITERS, damp=1e-8, dist_thresh=None)
    dt = time.perf_counter() - t0
    out = {"value": round(n_frames / dt, 4), "unit": "frames/s", "cores": cores, "kind": "port",
           "sample": "{} frames of the same 640x480/ds4/10-iter localisation step, CPU oracle "
                     "(torch CPU ops + OpenMP C nearest-neighbour), {:.1f} s".format(n_frames, dt)}
    # one nearest-neighbour search of the c2 size, single thread
    live = ofu.make_frame(c[:, 1:2], d[:, 1:2], K, f0["pose"])
    src = oicp.downsample_frame(live["gV"], live["gN"], live["rgb"], live["depth"], DS).points[0]
    tgt = oicp.downsample_map(cloud, ofu.find_active_map_points(cloud, f0), DS).points[0]
    oknn.set_threads(1)
    oknn.knn1(src, tgt)
    t0 = time.perf_counter()
    for _ in range(3):
        oknn.knn1(src, tgt)
    t_nn = (time.perf_counter() - t0) / 3
    oknn.set_threads(cores)
    out["nn_single_thread"] = {"seconds_per_search": round(t_nn, 4), "source_points": int(src.shape[0]), "target_points": int(tgt.shape[0]),
                               "searches_per_frame": 2 * ITERS, "frames_per_s_search_only": round(1.0 / (2 * ITERS * t_nn), 4), "cores": 1,
                               "note": "oracle/knn_ref.c (pytorch3d's loop structure) on one thread; the reference calls it 2 x numiters "
                                       "times per frame"}
    # configs[2] on the CPU: PointFusion (localise + map update) over 10 frames
    L = 10
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    c3, d3, K3, P3 = make_sequence(1, L, H, W, seed=100)
    t0 = time.perf_counter()
    oslam.run(c3, d3, K3, P3, mode="pointfusion", odom="icp", dsratio=DS, numiters=ITERS)
    dt3 = time.perf_counter() - t0
    out["c3_pointfusion"] = {"frames": L, "seconds_per_frame": round(dt3 / L, 4), "frames_per_s": round(L / dt3, 4), "cores": cores,
                             "note": "oracle.slam.run, PointFusion odom='icp', 640x480, forward only, {:.1f} s".format(dt3)}
    return out


def full_report(line, args, gs, dev, raw, world, prof):
    """--full: what the headline does not need -- the timed region's dominant kernel (`prof` = steps, launches and ms of
    the HIP-event pass; committed counter passes), the HBM rooflines of J, the auxiliary workloads and the CPU baseline
    -- added to `line` (rank 0)."""
    n_prof, n_knn, ms_knn = prof
    ns = nt = (H // DS) * (W // DS)
    avg_knn_ms = ms_knn / max(n_knn, 1)
    valu = None
    for name in ("r03_pmc_knn1_loop_valu.json", "r02_pmc_knn1_loop_valu.json"):  # executed work of the same kernel on the same
        try:                                                                      # workload: committed counter passes, newest first
            with open(os.path.join(ROOT, "profiles", name)) as f:
                valu = json.load(f)
            valu["profile_file"] = name  # (each profile carries the commit it was taken at)
            break
        except Exception:
            pass
    line["roofline_timed_region"] = {
        "kernel": "knn1_loop_k<true> (X+K+J fused: the previous iteration's O(1) step -- reduce, LM decision, 6x6 solve, exp -- "
                  "on wave 0 while one wave plans the tile's windows, one prepares the lanes' rows and seeds and thirteen stage the targets; then rigid transform, exact 1-NN association by grid "
                  "search with a geometric proof per point (exact chunk-box search for the points it fails for), "
                  "Jacobian rows and 29-term reduce of its 64-point tile)",
        "launches": n_knn, "avg_launch_ms": round(avg_knn_ms, 5),
        "timing_source": "HIP events on the launch stream, second eager pass of {} steps".format(n_prof),
        "hbm_view": {"algorithmic_bytes_per_launch": 40.0 * ns, "achieved_GBps": round(40.0 * ns / (avg_knn_ms * 1e-3) / 1e9, 2)
                     if n_knn else 0.0, "frac_of_8TBps": round(40.0 * ns / (avg_knn_ms * 1e-3) / 8e12, 5) if n_knn else 0.0,
                     "note": "0.77 MB per launch lives in L2: not an HBM measurement (fetched / written bytes per launch from "
                             "counter passes: profiles/r05_pmc_knn1_loop_traffic.json -- 1.8 MiB / 0.45 MiB raw)"},
        "valu_view": valu if valu is not None else {"note": "no committed counter pass found under profiles/"}}
    try:
        line["roofline"] = hbm_roofline_linearize(gs, dev)
    except Exception as e:  # pragma: no cover
        line["roofline"] = {"error": str(e)}
    if world == 1 and not os.environ.get("GS_BENCH_SHORT"):
        try:
            line["roofline_real_associations"] = hbm_linearize_real_associations(gs, dev)
        except Exception as e:  # pragma: no cover
            line["roofline_real_associations"] = {"error": str(e)}
    if world == 1:
        try:
            line["aux"] = aux_pointfusion(gs, dev, raw)
        except Exception as e:  # pragma: no cover
            line["aux"] = {"error": str(e)}
        for key, fn in (("association_other_sizes", aux_association_sizes), ("fusion_update_hbm_view", aux_fusion_update_roofline),
                        ("pointfusion_c3_200_frames", aux_c3_full_length)):
            if os.environ.get("GS_BENCH_SHORT"):
                break
            try:
                line["aux"][key] = fn(gs, dev)
            except Exception as e:  # pragma: no cover
                line["aux"][key] = {"error": str(e)}
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(raw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also: median of GS_BENCH_REPEATS timed regions, per-kernel timing, rooflines, aux workloads, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import gradslam_amd as gs
    from gradslam_amd import _native as nv
    from gradslam_amd import parallel

    rank, world, local = parallel.init_from_env()
    assert world == args.gpus or world == 1, "launch with torch.distributed.run --nproc-per-node {}".format(args.gpus)
    assert torch.cuda.is_available(), "bench.py needs a HIP device (no CPU fallback)"
    local = local % max(torch.cuda.device_count(), 1)  # rehearsals may put several ranks on one card
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    nv.lib()

    slam, world_map, prev, lives, K, raw = build_workload(gs, dev, seed=rank)
    n_map = int(world_map.num_points_per_pointcloud.item())

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    poses, prof = [], None
    with torch.no_grad():
        p0 = None
        for i in range(args.warmup):
            p0 = one_step(gs, slam, world_map, prev, lives[i % N_LIVE], K)
        # the final collection of the poses is part of the timed region: run it once untimed too (the first launch
        # of a torch kernel in a process lazily loads its code object -- ~7 ms the first time on a fresh box)
        p0 = p0 if p0 is not None else one_step(gs, slam, world_map, prev, lives[0], K)
        parallel.gather_poses(torch.cat([p0] * max(args.steps, 1), 1), world)
        # A full (generation-2) pass of Python's cyclic collector over the ~1e6 objects that importing torch leaves
        # behind takes ~40 ms -- 180 steps' worth -- and, allocation counts being deterministic, it landed on step 30
        # of every run.  What long-running services do: collect now, then freeze the survivors out of future passes.
        gc.collect()
        gc.freeze()
        # EXACTLY --steps steps per timed region, bracketed by barrier + synchronize on both sides; --full repeats the
        # region and reports the MEDIAN (one 20-step region is a 4.6 ms sample: too noisy for a headline)
        repeats = max(1, int(os.environ.get("GS_BENCH_REPEATS", "5"))) if args.full else 1
        dts = []
        i_last = args.steps - 1
        for rep in range(repeats):
            poses, last = [], []
            barrier()
            t0 = time.perf_counter()
            marks = []
            for i in range(args.steps):
                poses.append(one_step(gs, slam, world_map, prev, lives[i % N_LIVE], K, keep=last if i == i_last else None))
                if os.environ.get("GS_BENCH_TRACE"):
                    marks.append(time.perf_counter() - t0)
            t_enq = time.perf_counter() - t0
            local_poses = torch.cat(poses, 1)                      # (1, K, 4, 4)
            all_poses = parallel.gather_poses(local_poses, world)  # final RCCL gather of the poses
            t_gat = time.perf_counter() - t0
            barrier()
            dts.append(time.perf_counter() - t0)
        dt = sorted(dts)[len(dts) // 2]
        if os.environ.get("GS_BENCH_TRACE"):
            st = (ctypes.c_double * 4)()
            nv.lib().gs_graph_stats(st)
            print("[trace] enqueue %.3f ms, +cat/gather %.3f ms, total %.3f ms | launch policy: %d eager enqueues timed, min %.2f us "
                  "per launch, %d graphs captured, %d replays" % (1e3 * t_enq, 1e3 * t_gat, 1e3 * dt, st[0], st[1], st[2], st[3]),
                  file=sys.stderr)
            print("[trace] per-step host ms:", " ".join("%.2f" % (1e3 * (b - a)) for a, b in zip([0.0] + marks[:-1], marks)), file=sys.stderr)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, poses[-1], last[0])
        if args.full:
            # per-kernel durations: a second, short pass of the same steps with HIP events recorded around the
            # hot kernel on its launch stream (events force eager launches; the timed region above runs in the
            # library's automatic mode: eager launches on a fast host, hipGraph replay of the loop on a slow one)
            n_prof = min(args.steps, 20)
            nv.lib().gs_profile_enable(1)
            for i in range(n_prof):
                one_step(gs, slam, world_map, prev, lives[i % N_LIVE], K)
            torch.cuda.synchronize()
            prof = (n_prof,) + prof_read(nv, 0)
            nv.lib().gs_profile_enable(0)

    # how many ranks really took part, counted THROUGH the collective the poses travel on (N > 1: RCCL = backend "nccl")
    backend_name = torch.distributed.get_backend() if world > 1 else "none (single process)"
    one = torch.ones(1, dtype=torch.float64, device="cpu" if backend_name == "gloo" else dev)
    if world > 1:
        torch.distributed.all_reduce(one, op=torch.distributed.ReduceOp.SUM)
    ranks_seen = int(one.item())
    red_dev = "cpu" if (world > 1 and torch.distributed.get_backend() == "gloo") else dev
    tmax = torch.tensor(dts, dtype=torch.float64, device=red_dev)   # every repeat: MAX over ranks, then the median
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dts = sorted(tmax.tolist())
    dt = dts[len(dts) // 2]

    if rank == 0:
        # sanity: the recovered motion is the synthetic trajectory's (guards against a fast wrong answer)
        ref = raw[3][0, 1:1 + N_LIVE].cpu()
        got = all_poses[0, :min(args.steps, N_LIVE)].cpu()
        pose_err = float((got - ref[: got.shape[0]]).abs().max()) if got.numel() else 0.0
        # (10 point-to-plane iterations on a nearly fronto-parallel wall slide a little along it: 2-3 cm over the 1-4 cm
        # of motion; a wrong association or a broken solve is off by decimetres.  Exact parity: tests/, -m gpu.)
        assert pose_err < 0.06, "recovered poses are off the synthetic trajectory by {} m".format(pose_err)
        line = {
            "metric": "RGB-D frames/sec (640x480, 10 ICP iters)",
            "value": round(world * args.steps / dt, 3),
            "unit": "frames/s",
            "n_gpus": world,
            "ranks_seen": ranks_seen, "collective_backend": backend_name,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "repeats_ms_per_step": [round(1e3 * x / args.steps, 4) for x in dts],
            "config": {"workload": "c2: ICP odometry localisation step, 640x480 TUM-shape synthetic RGB-D, batch 1 per GPU, "
                                   "dsratio 4 (~19k x ~19k points), 10 LM iterations, map {} points".format(n_map),
                       "parallelism": "one sequence per GPU, final RCCL all_gather of poses", "pose_max_abs_err": pose_err,
                       "timing": "median of {} timed regions of {} steps each".format(len(dts), args.steps) if len(dts) > 1
                                 else "one timed region of {} steps".format(args.steps)},
        }
        if args.full:
            full_report(line, args, gs, dev, raw, world, prof)
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
