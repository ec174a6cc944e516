#!/usr/bin/env python3
"""Cost of Pointclouds.voxel_downsample's device work: one JSON line.

Input: the PointFusion map of `--frames` (100) synthetic 640x480 frames of make_sequence (ground-truth odometry; ~2 M points
with normals, colours and confidence counts), in map order (frame after frame, each in image order) and with its rows shuffled
by a seeded permutation; voxel sizes 0.01 and 0.05.  Timed with device events, median of `--runs` (20) after warm-up:
  hip        ops.voxel_assign, the read-back of n_voxels / n_dropped (the operation's one host synchronisation), and
             ops.voxel_reduce_raw of the four attributes (points, normals, colours: mean; features: sum); also assign alone, the
             four reductions alone, and the reductions without the pre-aggregation of neighbouring lanes
  torch      what a user writes without it: int64 keys from floor((p - o) / v), torch.unique(keys, return_inverse=True),
             index_add_ per attribute, bincount, division
Counted, not timed (launch counts are stated in DESIGN.md from the source, not here): integer atomics on the accumulators' low words per point and component with
and without pre-aggregation (from voxel_of: one add per run of lanes of a 64-lane wave that share a voxel; each may be followed
by one add on the high word); the bytes floor (every input row read once: 12 B points + 40 B attributes; voxel_of, voxel_count,
voxel_first written: 12 B per point; 40 B per voxel of output) and the fraction of it achieved at 8 TB/s.
"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.synthetic import make_sequence_cached as make_sequence

dev = "cuda:0"
HBM_BYTES_PER_S = 8.0e12  # HBM3E spec
TOLERANCE = 1e-5  # of the largest output element: a float sum of a few hundred members against the exact one


def event_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(statistics.median(out), 4)


def voxel_keys(p, v):
    """floor(p / v) in fp32, packed.  The divisor is a TENSOR of p's shape: torch evaluates `p / python_scalar` as a multiplication
    by 1 / v, which floors a few coordinates per million to the neighbouring voxel (the kernels divide, as numpy does)."""
    k = torch.floor(p / torch.full_like(p, v)).to(torch.int64) + (1 << 20)
    return k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def torch_downsample(attrs, v):
    """the formulation without the kernels: a device-wide sort (torch.unique) and float scatter-adds"""
    p = attrs[0]
    keys = voxel_keys(p, v)
    uniq, inv = torch.unique(keys, return_inverse=True)
    M = uniq.shape[0]
    cnt = torch.bincount(inv, minlength=M).to(torch.float32)
    outs = []
    for j, x in enumerate(attrs):
        s = torch.zeros((M, x.shape[1]), dtype=torch.float32, device=x.device).index_add_(0, inv, x)
        outs.append(s if j == 3 else s / cnt[:, None])
    return outs, cnt


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_timing: needs a HIP device (times are taken on the GPU or not at all)")
    c, d, K, P = (x.to(dev) for x in make_sequence(1, args.frames, args.height, args.width, seed=100))
    with torch.no_grad():
        world, _ = gs.slam.PointFusion(odom="gt", device=dev)(gs.RGBDImages(c, d, K, P))
    del c, d
    N = int(world.num_points_per_pointcloud[0])
    ordered = [x[0, :N].contiguous() for x in (world.points_padded, world.normals_padded, world.colors_padded, world.features_padded)]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(7)).to(dev)
    clouds = {"map_order": ordered, "shuffled": [x[perm].contiguous() for x in ordered]}
    counts = torch.full((1,), N, dtype=torch.int32, device=dev)
    widths = [x.shape[1] for x in ordered]
    props = torch.cuda.get_device_properties(0)
    r = {"tool": "voxel_timing", "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""),
         "compute_units": props.multi_processor_count, "memory_GiB": round(props.total_memory / 2 ** 30, 1), "tolerance": TOLERANCE,
         "frames": args.frames, "image": [args.height, args.width],
         "points": N, "components": widths, "runs": args.runs}
    modes = [ops.VOXEL_MEAN, ops.VOXEL_MEAN, ops.VOXEL_MEAN, ops.VOXEL_SUM]
    for case, attrs in clouds.items():
        padded = [x.unsqueeze(0) for x in attrs]
        for v in (0.01, 0.05):
            state = {}

            def assign():
                state["a"] = ops.voxel_assign(padded[0], counts, v)

            def sizes():
                host = torch.cat([state["a"][1], state["a"][2]]).tolist()
                state["M"] = max(host[0], 1)

            def reduce(extra=0):
                voxel_of, n_voxels, _, voxel_count, _ = state["a"]
                state["out"] = [ops.voxel_reduce_raw(x, counts, voxel_of, n_voxels, voxel_count, state["M"], m | extra)
                                for x, m in zip(padded, modes)]

            def whole():
                assign(); sizes(); reduce()

            whole()
            M = state["M"]
            voxel_of = state["a"][0][0]
            # the same answer as the torch formulation, asserted before anything is timed (its sums are float atomics in
            # arrival order: compared to TOLERANCE of the largest element, not bitwise)
            t_out, t_cnt = torch_downsample(attrs, v)
            assert t_cnt.shape[0] == M and int(state["a"][2][0]) == 0
            # torch.unique numbers voxels by key, the kernels by first row: compare in key order
            by_key = torch.argsort(voxel_keys(attrs[0][state["a"][4][0, :M].long()], v))
            assert torch.equal(state["a"][3][0, :M][by_key].to(torch.float32), t_cnt), "member counts differ from torch.unique's"
            worst = max(float((state["out"][j][0][by_key] - t_out[j]).abs().max() / t_out[j].abs().max().clamp(min=1e-30)) for j in range(4))
            assert worst <= TOLERANCE, "%s v=%g: differs from the torch formulation by %g of the largest element" % (case, v, worst)
            heads = torch.ones(N, dtype=torch.bool, device=dev)
            heads[1:] = voxel_of[1:] != voxel_of[:-1]
            heads[::64] = True
            tag = "%s/v=%g" % (case, v)
            total = event_ms(whole, args.runs)
            floor_bytes = N * (12 + 4 * sum(widths)) + 12 * N + 4 * sum(widths) * M
            r[tag] = {
                "voxels": M,
                "hip_ms": total,
                "hip_assign_ms": event_ms(assign, args.runs),
                "hip_reduce4_ms": event_ms(reduce, args.runs),
                "hip_reduce4_no_preagg_ms": event_ms(lambda: reduce(ops.VOXEL_NO_PREAGG), args.runs),
                "torch_unique_index_add_ms": event_ms(lambda: torch_downsample(attrs, v), args.runs),
                "low_word_atomics_per_point_and_component": {"preagg": round(float(heads.sum()) / N, 4), "no_preagg": 1.0},
                "bytes_floor": floor_bytes,
                "fraction_of_bytes_floor_at_8TBps": round(floor_bytes / HBM_BYTES_PER_S / (total * 1e-3), 4),
                "max_rel_diff_vs_torch": worst,
            }
            r[tag]["speedup_vs_torch"] = round(r[tag]["torch_unique_index_add_ms"] / total, 3)
    line = json.dumps(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
