#!/usr/bin/env python3
"""Results of the arena-backed sequence drivers as an .npz, for comparing two trees of the package bit for bit.

    sequence_ab.py run PACKAGE_ROOT OUT.npz      # import gradslam_amd from PACKAGE_ROOT, run the scenes, write every result
    sequence_ab.py compare A.npz B.npz           # one line per array: equal bits, or the largest difference

Scenes (5 frames of 120 x 160, dsratio 2, 6 iterations): PointFusion `icp` and ICPSLAM `gradicp` streamed, for one sequence
and for a batch of two -- poses, map, the per-frame counter rows (as the warnings hook sees them) and last_appended; PointFusion
`gradicp` with gradients as one node, one sequence, under torch.use_deterministic_algorithms(True) -- poses, map and the four
input gradients."""
import sys

import numpy as np


def run(root, out):
    sys.path.insert(0, root)
    import torch

    import gradslam_amd as gs
    from gradslam_amd.synthetic import make_sequence

    dev, res = "cuda:0", {}

    def keep(tag, pcs, poses):
        res[tag + "/poses"] = poses.detach().cpu().numpy()
        for attr in ("points", "normals", "colors", "features"):
            if getattr(pcs, "has_" + attr):
                for b, x in enumerate(getattr(pcs, attr + "_list")):
                    res["{}/{}{}".format(tag, attr, b)] = x.detach().cpu().numpy()

    for name, cls, odom in (("pointfusion_icp", gs.slam.PointFusion, "icp"), ("icpslam_gradicp", gs.slam.ICPSLAM, "gradicp")):
        for B in (1, 2):
            tag = "{}_B{}".format(name, B)
            slam = cls(odom=odom, dsratio=2, numiters=6, device=dev)
            rows, hook = [], slam._stream_warnings
            slam._stream_warnings = lambda s, row: (rows.append(list(row)), hook(s, row))[1]
            with torch.no_grad():
                pcs, poses = slam(gs.RGBDImages(*(x.to(dev) for x in make_sequence(B, 5, 120, 160, seed=11))))
            keep(tag, pcs, poses)
            res[tag + "/stats"] = np.array(rows)
            res[tag + "/last_appended"] = np.array(slam.last_appended)
    torch.use_deterministic_algorithms(True)
    leaves = [x.to(dev).requires_grad_(True) for x in make_sequence(1, 5, 120, 160, seed=13)]
    pcs, poses = gs.slam.PointFusion(odom="gradicp", dsratio=2, numiters=6, device=dev)(gs.RGBDImages(*leaves))
    loss = (poses * torch.linspace(0.5, 1.5, poses.numel(), device=dev).view_as(poses)).sum() + pcs.points_padded.sum() + \
        (pcs.normals_padded * 0.3).sum() + pcs.colors_padded.mean() + (pcs.features_padded ** 2).sum() * 1e-3
    loss.backward()
    keep("node", pcs, poses)
    for name, x in zip(("colors", "depths", "intrinsics", "poses"), leaves):
        res["node/grad_" + name] = x.grad.cpu().numpy()
    np.savez(out, **res)
    print("wrote", out, len(res), "arrays")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    print("compare", a, b)
    assert sorted(A.files) == sorted(B.files), (sorted(A.files), sorted(B.files))
    worst = True
    for k in sorted(A.files):
        x, y = A[k], B[k]
        same = x.shape == y.shape and x.tobytes() == y.tobytes()
        worst = worst and same
        print("  {:40s} {}".format(k, "bitwise equal" if same else "DIFFERENT shapes {} {} max |a-b| {}".format(
            x.shape, y.shape, float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.shape == y.shape else "n/a")))
    print("ALL BITWISE EQUAL" if worst else "NOT ALL EQUAL")
    return worst


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
