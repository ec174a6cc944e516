#!/usr/bin/env python3
"""Cost of the dense RGB-D odometry (ops.rgbd_odometry / gs_rgbd_odometry) on a frame pair of the synthetic sequence with a
smooth texture: one JSON line (profiles/rgbd_cost.json).  Every figure is the median (min, max) of RUNS single calls after WARMUP
calls, each timed with a pair of device events.
  odometry_ms        the whole call: both pyramids, then numiters[l] x (linearise + step) per level, coarse to fine
  pyramids_ms        the same call with zero iterations at every level: the pyramids and the start-up launch
  level0_iter_us     (call with numiters (N0 + 10, ..) - call with (N0, ..)) / 10: one linearise + step pair at level 0
  gradicp_ms         one GradICPOdometryProvider.provide on the same pair at dsratio = 4 (clouds built outside the timing)
  taped_forward_ms   the call with differentiable=True and inputs that require gradients: the taped loop (and the tape's allocation)
  forward_backward_ms  that call and .backward() of a sum over T: the reverse pass (gs_rgbd_odometry_bwd) on top
  backward_launches, backward_ws_bytes  the reverse pass's launches (3 per iteration) and its workspace
The level-0 linearise launch must move 8 B per source pixel, 8 B per target pixel (every corner once) and 116 B per block of 256
pixels: `level0_bytes`, quoted against the HBM bandwidth as `level0_hbm_floor_us`.  The sums of the 480 x 640 call are also
checked against a float64 sum of the device's own rows (what no test does at this size: more than 512 partial rows)."""
import argparse, json, os, statistics, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops
from gradslam_amd.odometry.icputils import downsample_rgbdimages
from gradslam_amd.synthetic import make_sequence_cached as make_sequence

dev = "cuda:0"
HBM_BYTES_PER_S = 8.0e12  # MI355X peak


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
    return [round(x, 4) for x in (statistics.median(out), min(out), max(out))]


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--numiters", type=int, nargs="+", default=[10, 5, 3])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--date", default=None, help="the day of the run (the GPU host's clock is not trusted)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbd_cost.json"))
    a = ap.parse_args()
    H, W, levels, counts = a.height, a.width, a.levels, tuple(a.numiters)
    _, d, K, P = (x.to(dev) for x in make_sequence(1, 2, H, W, seed=3))
    frames = gs.RGBDImages(torch.zeros(1, 2, H, W, 3, device=dev), d, K, P)
    g = frames.global_vertex_map  # a smooth texture of world coordinates, so that both frames see the same colours
    tex = torch.stack([127.5 + 127.5 * (torch.sin(9.0 * g[..., 0] + 5.0 * g[..., 1] + ph) + torch.sin(13.0 * g[..., 1] - 4.0 * g[..., 0]
                                                                                                   + 2 * ph)) / 2 for ph in (0.0, 1.3, 2.9)], -1)
    frames = gs.RGBDImages(tex.contiguous(), d, K, P)
    tgt, src = frames[:, 0], frames[:, 1]
    args = (tgt.depth_image[:, 0], tgt.rgb_image[:, 0], src.depth_image[:, 0], src.rgb_image[:, 0], K)
    run = lambda n: ops.rgbd_odometry(*args, numiters=n, levels=levels)
    T, info = run(counts)
    true = torch.linalg.inv(P[0, 0].double()) @ P[0, 1].double()
    more = (counts[0] + 10,) + counts[1:]
    full, pyr, longer = event_ms(lambda: run(counts), a.runs, a.warmup), event_ms(lambda: run((0,) * levels), a.runs, a.warmup), \
        event_ms(lambda: run(more), a.runs, a.warmup)
    # the differentiable call: the taped forward alone, then with the reverse pass
    leaves = [x.clone().requires_grad_(True) for x in args[:4]]
    taped_run = lambda: ops.rgbd_odometry(*leaves, K, numiters=counts, levels=levels, differentiable=True)
    T_taped, info_taped = taped_run()
    assert torch.equal(T_taped.detach(), T) and torch.equal(info_taped, info)

    def fwd_bwd():
        for x in leaves:
            x.grad = None
        taped_run()[0][:, :3].sum().backward()

    taped, both = event_ms(taped_run, a.runs, a.warmup), event_ms(fwd_bwd, a.runs, a.warmup)
    assert all(torch.isfinite(x.grad).all() and x.grad.abs().max() > 0 for x in leaves)
    used = sum(1 for n in counts if n > 0)
    bwd_launches = 2 * levels + 2 + 1 + 3 * sum(counts) + 2 * used + 2 * levels  # pyramids, zero, begin | loop | fold zero + finish | adjoint pyramids
    bwd_ws = int(nv.ws_bytes("gs_rgbd_odometry_bwd_ws_size", 1, H, W, levels, sum(counts)))
    # the sums at this size against float64 sums of the device's own rows
    valid, rows, sums = ops.rgbd_rows_raw(*args, T)
    r = rows.double().reshape(-1, 14)
    JI, rI, JD, rD = r[:, :6], r[:, 6], r[:, 7:13], r[:, 13]
    terms = [JI[:, m] * JI[:, n] + JD[:, m] * JD[:, n] for m in range(6) for n in range(m, 6)] + \
            [-(JI[:, m] * rI + JD[:, m] * rD) for m in range(6)] + [rI * rI + rD * rD, valid.double().reshape(-1)]
    nblocks = -(-H * W // 256)
    k = 6 + 4 + -(-nblocks // 32) + 32  # butterfly, the block's waves, the group's rows, the 32 groups
    worst = max(float((sums[0, q].double() - t.sum()).abs() / (k * 2.0 ** -24 * t.abs().sum()).clamp_min(1e-300)) for q, t in enumerate(terms))
    assert worst <= 1.0, worst
    # GradICP on the same pair, downsampled by 4
    tc, sc = downsample_rgbdimages(tgt, 4), downsample_rgbdimages(gs.RGBDImages(src.rgb_image, src.depth_image, K, P[:, :1]), 4)
    prov = gs.odometry.GradICPOdometryProvider(numiters=20)
    with torch.no_grad():
        gradicp = event_ms(lambda: prov.provide(tc, sc), a.runs, a.warmup)
    level0_bytes = 16 * H * W + 116 * nblocks
    line = {"what": "rgbd_odometry", "H": H, "W": W, "B": 1, "levels": levels, "numiters": list(counts), "runs": a.runs,
            "odometry_ms": full, "pyramids_ms": pyr, "level0_iter_us": round(100.0 * (longer[0] - full[0]), 2),
            "launches": 1 + 2 * levels + 2 * sum(counts), "level0_bytes": level0_bytes,
            "level0_hbm_floor_us": round(1e6 * level0_bytes / HBM_BYTES_PER_S, 3), "gradicp_dsratio4_numiters20_ms": gradicp,
            "taped_forward_ms": taped, "forward_backward_ms": both, "backward_launches": bwd_launches, "backward_ws_bytes": bwd_ws,
            "info": info[0].tolist(), "translation_error_m": float((T[0, :3, 3].double() - true[:3, 3]).norm()),
            "sums_worst_error_over_bound": round(worst, 4), "chain_length": k, "device": torch.cuda.get_device_name(0),
            "date": a.date, "commit": a.commit or commit()}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(line) + "\n")
