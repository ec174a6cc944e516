#!/usr/bin/env python3
"""Cost of the SDF odometry's reverse pass (ops.sdf_odometry(differentiable=True): gs_sdf_odometry_taped + gs_sdf_odometry_bwd)
relative to the plain forward call, measured in ONE process per case: one JSON line (profiles/sdf_grad_cost.json).  B = 1,
`numiters=(10, 5, 3)`, stride 1; every figure is the median (min, max) of RUNS single calls after WARMUP calls, each timed with a
pair of device events; the variants of a case are alternated ROUNDS times round.
  small   a 48 x 64 frame against a 24 x 20 x 16 volume of 5 cm voxels (the size of tests/test_sdf_odometry.py's "48x64")
  large   a 480 x 640 frame against a 256^3 volume of 1.25 cm voxels (16.8 M voxels: the room holds 335 MB of fold)
The volume holds frame 0 of the synthetic sequence under its true pose; frame 1 is tracked from frame 0's pose.
  plain_ms        ops.sdf_odometry, no gradients
  taped_ms        differentiable=True with inputs that require gradients: the taped forward alone (tape allocation included)
  fwd_bwd_ms      the taped forward + .backward() of a sum over T: depth, poses, init and tsdf require gradients
  fwd_bwd_no_volume_ms   the same with the tsdf detached: no second sweep, no fold, no fold memory
A kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 tools/sdf_grad_cost.py --worker large --runs 10 --warmup 3 --rounds 1"""
import argparse, json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"small": dict(H=48, W=64, dims=(24, 20, 16), v=0.05, origin=(-0.6, -0.5, 1.7)),
         "large": dict(H=480, W=640, dims=(256, 256, 256), v=0.0125, origin=(-1.6, -1.6, 0.4))}
COUNTS, LEVELS = (10, 5, 3), 3


def worker(a):
    sys.path.insert(0, HERE)
    import torch
    import gradslam_amd as gs
    from gradslam_amd import ops
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    dev, c = "cuda:0", CASES[a.worker]
    H, W, v, trunc = c["H"], c["W"], c["v"], 3 * c["v"]

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    col, d, K, P = (x.to(dev) for x in make_sequence(1, 2, H, W, seed=3))
    with torch.no_grad():
        vol = gs.TSDFVolume(c["dims"], v, origin=[c["origin"]], trunc=trunc, color=False, device=dev).integrate(gs.RGBDImages(col, d, K, P)[:, 0])
    depth, pose, init = d[:, 1, ..., 0].contiguous(), P[:, 0].contiguous(), torch.eye(4, device=dev).view(1, 4, 4)
    call = lambda dd, pp, ii, tt, diff: ops.sdf_odometry(dd, K, pp, tt, vol.weight, vol.origin, v, trunc, init=ii, numiters=COUNTS, levels=LEVELS,
                                                          differentiable=diff)
    leaf = lambda t: t.clone().requires_grad_(True)

    def plain():
        with torch.no_grad():
            call(depth, pose, init, vol.tsdf, False)

    def taped():
        call(leaf_d, leaf_p, leaf_i, leaf_t, True)

    def fwd_bwd():
        for t in (leaf_d, leaf_p, leaf_i, leaf_t):
            t.grad = None
        call(leaf_d, leaf_p, leaf_i, leaf_t, True)[0].sum().backward()

    def fwd_bwd_no_volume():
        for t in (leaf_d, leaf_p, leaf_i):
            t.grad = None
        call(leaf_d, leaf_p, leaf_i, vol.tsdf, True)[0].sum().backward()

    leaf_d, leaf_p, leaf_i, leaf_t = leaf(depth), leaf(pose), leaf(init), leaf(vol.tsdf)
    variants = dict(plain_ms=plain, taped_ms=taped, fwd_bwd_ms=fwd_bwd, fwd_bwd_no_volume_ms=fwd_bwd_no_volume)
    with torch.no_grad():
        T, info = call(depth, pose, init, vol.tsdf, False)
    true = P[0, 1].double() @ torch.linalg.inv(P[0, 0].double())
    fwd_bwd()
    grads = {k: float(t.grad.abs().max()) for k, t in (("depth", leaf_d), ("poses", leaf_p), ("init", leaf_i), ("tsdf", leaf_t))}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):  # the variants alternated
        for k, fn in variants.items():
            times[k] += [event_ms(fn) for _ in range(a.runs)]
    out = {"what": a.worker, "H": H, "W": W, "dims": list(c["dims"]), "voxel_size": v, "trunc": trunc, "numiters": list(COUNTS),
           "runs": a.runs, "rounds": a.rounds, "info": info[0].tolist(), "valid_level0": info[0, 0, 0].item(),
           "translation_error_m": float((T[0, :3, 3].double() - true[:3, 3]).norm()), "translation_m": float(true[:3, 3].norm()),
           "largest_gradient_entries": grads,
           "room_bytes": [int(ops.ws_bytes("gs_sdf_odometry_bwd_room", 1, H, W, 1, LEVELS, sum(COUNTS), *c["dims"], k)) for k in (1, 0)],
           "tape_bytes": int(ops.ws_bytes("gs_sdf_odometry_tape_bytes_for", 1, H, W, 1, LEVELS, sum(COUNTS))),
           "device": torch.cuda.get_device_name(0)}
    for k, xs in times.items():
        out[k] = [round(x, 4) for x in (statistics.median(xs), min(xs), max(xs))]
    out["fwd_bwd_over_plain"] = round(out["fwd_bwd_ms"][0] / out["plain_ms"][0], 2)
    out["fwd_bwd_no_volume_over_plain"] = round(out["fwd_bwd_no_volume_ms"][0] / out["plain_ms"][0], 2)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, choices=sorted(CASES))
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--date", default=None, help="the day of the run (the GPU host's clock is not trusted)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sdf_grad_cost.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a)
        sys.exit(0)
    line = {"what": "sdf_odometry_gradients", "date": a.date, "commit": a.commit}
    for what in ("small", "large"):  # one child at a time
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--runs", str(a.runs), "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
        txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
        line[what] = json.loads([l for l in txt.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(what, json.dumps({k: v for k, v in line[what].items() if k.endswith("_ms") or k.endswith("_plain")}), flush=True)
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(line) + "\n")
