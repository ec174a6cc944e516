#!/usr/bin/env python3
"""Every result that passes through the fixed-order sums of gs_rowsum.hpp, as an .npz, for comparing two trees bit for bit.

    rowsum_ab.py run PACKAGE_ROOT OUT.npz      # import gradslam_amd (and tests) from PACKAGE_ROOT, run the calls, write every result
    rowsum_ab.py compare A.npz B.npz           # one line per array: equal bits, or the largest difference

Calls, each on seeded inputs and sized so that a fold group holds more than one row: vertex_normal_maps backward at 70 x 257
(71 rows, 32 groups), with and without poses; render_map backward at 120 x 160, B = 2 (75 rows, 64 groups); the TSDF pose
gradients of integration and ray cast on tests/test_tsdf_pose_grads.py's scenes; rgbd_odometry backward at 96 x 130 (49 rows, 16
groups); icp_linearize; icp_loop_autograd on 5000 source points (20 rows, 16 groups) and slam_localize_autograd at 120 x 160
with dsratio 1 (75 rows), LM and gradLM, with and without torch.use_deterministic_algorithms."""
import sys

import numpy as np


def run(root, out):
    sys.path.insert(0, root)
    import torch

    import gradslam_amd as gs
    from gradslam_amd import ops
    from gradslam_amd.structures.utils import pointclouds_from_rgbdimages
    from gradslam_amd.synthetic import make_sequence
    from tests import test_tsdf as tt
    from tests import test_tsdf_pose_grads as tp
    from tests import test_tsdf_raycast as tr

    dev, res = "cuda:0", {}
    rng = np.random.RandomState(2026)
    rand = lambda *shape: torch.from_numpy((rng.randn(*shape) * 10.0 ** rng.uniform(-2, 2, shape)).astype(np.float32)).to(dev)

    def keep(tag, xs):
        for i, x in enumerate(xs):
            if x is not None:
                res["%s/%d" % (tag, i)] = x.detach().cpu().numpy()

    def flagged(tag, fn):
        for flag in (False, True):
            torch.use_deterministic_algorithms(flag)
            try:
                keep("%s_%s" % (tag, "det" if flag else "plain"), fn())
            finally:
                torch.use_deterministic_algorithms(False)

    # ---- maps
    c, d, K, P = (x.to(dev) for x in make_sequence(2, 2, 70, 257, seed=3))
    ups = [rand(2, 2, 70, 257, 3) for _ in range(4)]

    def maps(with_poses):
        leaves = [x.clone().requires_grad_(True) for x in ((d, K, P) if with_poses else (d, K))]
        outs = ops.vertex_normal_maps(leaves[0], leaves[1], leaves[2] if with_poses else None)
        torch.autograd.backward([o for o in outs if o is not None], [u for o, u in zip(outs, ups) if o is not None])
        return [x.grad for x in leaves]

    flagged("maps_posed", lambda: maps(True))
    flagged("maps_unposed", lambda: maps(False))

    # ---- render
    seq = make_sequence(2, 3, 120, 160, seed=5)
    fr = gs.RGBDImages(seq[0][:, 2:3].to(dev), seq[1][:, 2:3].to(dev), seq[2].to(dev), seq[3][:, 2:3].to(dev))
    pc = pointclouds_from_rgbdimages(fr)
    up_r = [rand(2, 120, 160)] + [rand(2, 120, 160, 3) for _ in range(3)]

    def render():
        leaves = [x.detach().clone().requires_grad_(True) for x in (pc.points_padded, pc.normals_padded, pc.colors_padded, fr.poses[:, 0])]
        outs = ops.render_map(leaves[0], leaves[1], leaves[2], pc._counts_i32(), leaves[3], fr.intrinsics[:, 0].contiguous(), 120, 160)
        torch.autograd.backward(list(outs[1:]), up_r)
        return [outs[0]] + [x.grad for x in leaves]

    flagged("render", render)

    # ---- TSDF pose gradients
    for L in (3, 33):
        colors, depths, Ki, poses = tp.to_dev(*tp.integrate_scene(L))
        f0, w0, c0, g_f, g_c = tp.integrate_inputs(L)
        shape = (tp.I_B, tp.I_DIMS[2], tp.I_DIMS[1], tp.I_DIMS[0])
        t = lambda x, s: torch.from_numpy(x).reshape(s).to(dev)
        origin = ops.tsdf_origin(tp.I_ORIGINS, tp.I_B, dev)
        for color in (True, False):
            keep("tsdf_integrate_L%d_%s" % (L, "color" if color else "nocolor"), ops.tsdf_integrate_backward_poses_raw(
                depths, Ki, poses, t(w0, shape), origin, tt.V, tt.TRUNC, 2.0, t(g_f, shape), t(g_c, shape + (3,)) if color else None))
    Kc, pc_ = tp.cast_cameras()
    for stride in (1, 3):
        for step in tr.STEPS:
            vol = tr.device_volume(color=True)
            fwd = ops.tsdf_raycast_raw(vol.tsdf, vol.weight, vol.color, vol.origin, tr.V, Kc, pc_, tp.C_H, tp.C_W, stride, step)
            gd, gc = (torch.from_numpy(x).to(dev) for x in tp.cast_upstream(stride))
            keep("tsdf_cast_s%d_%g" % (stride, step), ops.tsdf_raycast_backward_poses_raw(
                vol.tsdf, vol.weight, vol.color, vol.origin, tr.V, Kc, pc_, tp.C_H, tp.C_W, stride, step, 1.0, fwd[3], gd, gc))

    # ---- RGB-D odometry
    c, d, K, P = (x.to(dev) for x in make_sequence(2, 2, 96, 130, seed=9, step_t=0.004, step_r=0.001))
    W = rand(2, 3, 4)

    def rgbd():
        leaves = [x.clone().requires_grad_(True) for x in (d[:, 0], c[:, 0], d[:, 1], c[:, 1], torch.eye(4, device=dev).repeat(2, 1, 1))]
        T, info = ops.rgbd_odometry(*leaves[:4], K, init=leaves[4], numiters=(3, 2), levels=2, differentiable=True)
        (W * T[:, :3]).sum().backward()
        return [T, info] + [x.grad for x in leaves]

    flagged("rgbd", rgbd)

    # ---- ICP: a wavy surface and 5000 of its points moved a little
    g = np.stack(np.meshgrid(np.arange(80), np.arange(75), indexing="ij"), -1).reshape(-1, 2) * 0.05
    z = 2.0 + 0.3 * np.sin(1.3 * g[:, 0]) * np.cos(0.9 * g[:, 1])
    nrm = np.stack([-0.39 * np.cos(1.3 * g[:, 0]) * np.cos(0.9 * g[:, 1]), 0.27 * np.sin(1.3 * g[:, 0]) * np.sin(0.9 * g[:, 1]), np.ones(len(g))], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tgt = np.concatenate([g, z[:, None]], 1)
    ang = 0.01
    R = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    src = tgt[rng.permutation(len(tgt))[:5000]] @ R.T + np.array([0.004, -0.003, 0.006]) + rng.randn(5000, 3) * 1e-3
    src, tgt, nrm = (torch.from_numpy(x.astype(np.float32)).to(dev) for x in (src, tgt, nrm))
    Wt = rand(4, 4)
    gH, gg, ge = rand(6, 6), rand(6, 1), torch.tensor(0.5, device=dev)

    def linearize():
        x = [v.clone().requires_grad_(True) for v in (src, tgt, nrm)]
        outs = ops.icp_linearize(*x, ops.knn1_raw(src, tgt), None)
        torch.autograd.backward(list(outs), [gH, gg, ge])
        return list(outs) + [v.grad for v in x]

    flagged("icp_linearize", linearize)
    for name, grad in (("lm", None), ("gradlm", (2.0, 1.0, 1.0, 200.0))):
        def loop():
            x = [v.clone().requires_grad_(True) for v in (src, tgt, nrm, torch.eye(4, device=dev))]
            T, best = ops.icp_loop_autograd(*x, 6, 1e-8, None, grad_params=grad)
            (T * Wt).sum().backward()
            return [T, best] + [v.grad for v in x]

        flagged("icp_loop_" + name, loop)

    # ---- localisation: frame 1 against the map of frame 0, every pixel a source point
    c, d, K, P = (x.to(dev) for x in make_sequence(1, 2, 120, 160, seed=6))
    with torch.no_grad():
        pcs, _ = gs.slam.PointFusion(odom="gt", device=dev)(gs.RGBDImages(c[:, :1], d[:, :1], K, P[:, :1]))
    mp, mn, cnt = pcs.points_padded.contiguous(), pcs.normals_padded.contiguous(), pcs.num_points_per_pointcloud.to(torch.int32).contiguous()
    depth, prev = d[:, 1:2].contiguous(), P[:, :1].contiguous()
    gV = ops.vertex_normal_maps_raw(depth, K, prev, False, True)[2]
    Wp = rand(1, 1, 4, 4)
    for name, grad in (("lm", None), ("gradlm", (2.0, 1.0, 1.0, 200.0))):
        def localize():
            x = [v.clone().requires_grad_(True) for v in (gV, mp, mn, prev)]
            out = ops.slam_localize_autograd(x[0], depth, K, x[3], x[1], x[2], cnt, 1, 6, 1e-8, 0.1, grad)
            (out * Wp).sum().backward()
            return [out] + [v.grad for v in x]

        flagged("slam_localize_" + name, localize)

    torch.cuda.synchronize()
    np.savez(out, **res)
    print("wrote", out, len(res), "arrays")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    print("compare", a, b)
    assert sorted(A.files) == sorted(B.files), (sorted(A.files), sorted(B.files))
    same_all = True
    for k in sorted(A.files):
        x, y = A[k], B[k]
        same = x.shape == y.shape and x.tobytes() == y.tobytes()
        same_all = same_all and same
        print("  {:40s} {}".format(k, "bitwise equal" if same else "DIFFERENT shapes {} {} max |a-b| {}".format(
            x.shape, y.shape, float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))) if x.shape == y.shape else "n/a")))
    print("ALL BITWISE EQUAL (%d arrays)" % len(A.files) if same_all else "NOT ALL EQUAL")
    return same_all


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
