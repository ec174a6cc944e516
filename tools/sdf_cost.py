#!/usr/bin/env python3
"""Cost of the SDF odometry (ops.sdf_odometry / gs_sdf_odometry) and of a KinectFusion step tracked with it, against the ICP- and
RGB-D-tracked steps of another tree (--parent DIR: a checkout of the parent commit with its library built), measured in ONE
session on the same frames and the same volume, the trees alternated: one JSON line (profiles/sdf_cost.json).  480 x 640, B = 1;
every figure is the median (min, max) of RUNS single calls after WARMUP calls, each timed with a pair of device events.
  sdf_odometry_ms       the whole call at stride 1: numiters[l] x (linearise + step) per level, coarse to fine, and the start
  level0_iter_us        (call with numiters (N0 + 10, ..) - call with (N0, ..)) / 10: one linearise + step pair at level 0
  step_sdf_ms           one KinectFusion.step with odom="sdf" (track + integrate), at dsratio 4 (the ICP branch's pixel subset)
                        and at dsratio 1
  step_icp_ms, step_rgbd_ms   the other tree's KinectFusion.step with odom="icp" (dsratio 4, 20 iterations: ray cast, cloud, two
                        host reads, ICP, integrate) and odom="rgbd" (coloured cast, alignment, integrate)
Every measurement runs in a child process of its own (`--worker`), which imports gradslam_amd from the tree it is given; the
children run one after another, `--rounds` times round the trees.  The volume holds frame 0 of the synthetic sequence under its true
pose; the step tracks frame 1 from frame 0's pose.  A kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 tools/sdf_cost.py --worker sdf_call --runs 20 --warmup 5"""
import argparse, json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, V, TRUNC, ORIGIN = (128, 96, 48), 0.025, 0.075, (-1.6, -1.2, 1.45)  # the wall z = 2 +- 0.3 as 480 x 640 pixels at f = 525 see it
COUNTS, LEVELS = (10, 5, 3), 3


def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import gradslam_amd as gs
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    assert os.path.abspath(gs.__file__).startswith(os.path.abspath(a.tree)), gs.__file__
    dev = "cuda:0"

    def event_ms(fn):
        for _ in range(a.warmup):
            fn()
        out = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            out.append(t0.elapsed_time(t1))
        return [round(x, 4) for x in (statistics.median(out), min(out), max(out))]

    H, W = a.height, a.width
    c, d, K, P = (x.to(dev) for x in make_sequence(1, 2, H, W, seed=3))
    frames = gs.RGBDImages(c, d, K, P)
    kw = dict(dims=DIMS, voxel_size=V, origin=[ORIGIN], trunc=TRUNC, device=dev)
    out = {"what": a.worker, "tree": a.tree}
    with torch.no_grad():
        if a.worker == "sdf_call":
            from gradslam_amd import ops
            vol = gs.TSDFVolume(DIMS, V, origin=[ORIGIN], trunc=TRUNC, color=False, device=dev).integrate(frames[:, 0])
            run = lambda n: ops.sdf_odometry(d[:, 1], K, P[:, 0], vol.tsdf, vol.weight, vol.origin, V, TRUNC, numiters=n, levels=LEVELS)
            T, info = run(COUNTS)
            true = P[0, 1].double() @ torch.linalg.inv(P[0, 0].double())  # the world-frame delta from frame 0's pose to frame 1's
            more = (COUNTS[0] + 10,) + COUNTS[1:]
            full, longer, none = event_ms(lambda: run(COUNTS)), event_ms(lambda: run(more)), event_ms(lambda: run((0,) * LEVELS))
            out.update(sdf_odometry_ms=full, start_only_ms=none, level0_iter_us=round(100.0 * (longer[0] - full[0]), 2),
                       launches=1 + 2 * sum(COUNTS), info=info[0].tolist(),
                       translation_error_m=float((T[0, :3, 3].double() - true[:3, 3]).norm()),
                       translation_m=float(true[:3, 3].norm()))
        else:
            odom, dsratio = {"step_sdf4": ("sdf", 4), "step_sdf1": ("sdf", 1), "step_icp": ("icp", 4), "step_rgbd": ("rgbd", 4)}[a.worker]
            extra = dict(numiters=COUNTS, levels=LEVELS) if odom != "icp" else dict(numiters=20)
            slam = gs.slam.KinectFusion(odom=odom, dsratio=dsratio, color=odom == "rgbd", **kw, **extra)
            vol0, _ = slam.step(slam.new_volume(1), frames[:, 0])

            def step():
                live = gs.RGBDImages(c[:, 1:2], d[:, 1:2], K)
                return slam.step(vol0, live, frames[:, 0])[1]

            pose = step()
            out.update(step_ms=event_ms(step), odom=odom, dsratio=dsratio, numiters=list(COUNTS) if odom != "icp" else 20,
                       translation_error_m=float((pose[0, 0, :3, 3] - P[0, 1, :3, 3]).norm()),
                       translation_m=float((P[0, 1, :3, 3] - P[0, 0, :3, 3]).norm()))
    out["device"] = torch.cuda.get_device_name(0)
    print("RESULT " + json.dumps(out))


def child(a, what, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--tree", tree, "--runs", str(a.runs), "--warmup", str(a.warmup),
           "--height", str(a.height), "--width", str(a.width)]
    txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=240).stdout
    return json.loads([l for l in txt.splitlines() if l.startswith("RESULT ")][-1][7:])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, choices=["sdf_call", "step_sdf4", "step_sdf1", "step_icp", "step_rgbd"])
    ap.add_argument("--tree", default=HERE, help="the tree a worker imports gradslam_amd from")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its odom='icp' and 'rgbd' steps")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--date", default=None, help="the day of the run (the GPU host's clock is not trusted)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sdf_cost.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a)
        sys.exit(0)
    plan = [("sdf_call", HERE), ("step_sdf4", HERE), ("step_sdf1", HERE)]
    if a.parent:
        plan += [("step_icp", a.parent), ("step_rgbd", a.parent)]
    rounds = []
    for r in range(a.rounds):  # one child at a time, the trees alternated
        rounds.append({what: child(a, what, tree) for what, tree in plan})
        print("round", r, json.dumps({k: v.get("step_ms", v.get("sdf_odometry_ms")) for k, v in rounds[-1].items()}), flush=True)
    first = rounds[0]
    line = {"what": "sdf_odometry", "H": a.height, "W": a.width, "B": 1, "levels": LEVELS, "numiters": list(COUNTS), "runs": a.runs,
            "rounds": a.rounds, "dims": list(DIMS), "voxel_size": V, "trunc": TRUNC,
            "sdf_odometry_ms": [r["sdf_call"]["sdf_odometry_ms"] for r in rounds],
            "start_only_ms": [r["sdf_call"]["start_only_ms"] for r in rounds],
            "level0_iter_us": [r["sdf_call"]["level0_iter_us"] for r in rounds], "launches": first["sdf_call"]["launches"],
            "info": first["sdf_call"]["info"], "translation_m": first["sdf_call"]["translation_m"],
            "sdf_translation_error_m": first["sdf_call"]["translation_error_m"],
            "step_sdf_dsratio4_ms": [r["step_sdf4"]["step_ms"] for r in rounds],
            "step_sdf_dsratio1_ms": [r["step_sdf1"]["step_ms"] for r in rounds],
            "step_translation_error_m": {k: first[k]["translation_error_m"] for k in first if k.startswith("step_")},
            "device": first["sdf_call"]["device"], "date": a.date, "commit": a.commit}
    if a.parent:
        line.update(parent_commit=a.parent_commit, parent_step_icp_dsratio4_numiters20_ms=[r["step_icp"]["step_ms"] for r in rounds],
                    parent_step_rgbd_ms=[r["step_rgbd"]["step_ms"] for r in rounds])
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(line) + "\n")
