"""gs.slam.KinectFusion: the frame loop raycast -> ICP against the cast surface -> integrate, on TSDFVolume.

The driver is host-side composition of public pieces, so the tests pin the wiring: every pose is, bit for bit, the hand
composition of TSDFVolume.raycast_pointcloud, downsample_rgbdimages, the odometry provider and compose_transformations, and the
volume is TSDFVolume.integrate of the frames under those poses.  Quality is measured against ICPSLAM(odom="icp") on the same
frames: ATE_kf <= max(2 ATE_icpslam, voxel_size) (the target is the surface of a 5 cm grid and has fewer points; voxel_size is
the resolution of the map tracked against).
"""
import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd.geometry.geometryutils import compose_transformations
from gradslam_amd.metrics import absolute_trajectory_error
from gradslam_amd.odometry.icputils import downsample_rgbdimages
from gradslam_amd.slam import ICPSLAM, KinectFusion
from gradslam_amd.synthetic import make_sequence

DEV = "cuda:0"
# a volume that holds what the cameras see of the wall z = 2 +- 0.3 (48 x 64 pixels at 52.5 px focal length: |x| < 1.3, |y| < 1 there):
# ICP runs without a distance threshold, so frame points beyond the volume would pair with the cast surface's rim
DIMS, V, TRUNC = (56, 40, 24), 0.05, 0.15
ORIGINS = [(-1.4, -1.0, 1.4), (-1.35, -0.95, 1.45)]
H, W, L = 48, 64, 6


def kf(B=1, **kw):
    kw.setdefault("odom", "icp")
    return KinectFusion(dims=DIMS, voxel_size=V, origin=ORIGINS[:B], trunc=TRUNC, device=DEV, **kw)


def frames(B=1, dev=DEV):
    colors, depths, K, poses = (t.to(dev) for t in make_sequence(B, L, H, W, seed=0))
    return gs.RGBDImages(colors, depths, K, poses)


def same_volume(a, b):
    return torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and torch.equal(a.color, b.color)


# ------------------------------------------------------------------ CPU: the error contracts
def test_kinectfusion_error_contracts():
    assert gs.slam.KinectFusion is KinectFusion and isinstance(kf(), torch.nn.Module)
    with pytest.raises(ValueError, match="not supported"):
        kf(odom="orb")
    with pytest.raises(ValueError, match="dsratio"):
        kf(dsratio=0)
    with pytest.raises(TypeError):
        KinectFusion(DIMS, V)  # keyword-only
    slam = kf()
    assert slam.odomprov.numiters == 20 and slam.dsratio == 4 and kf(odom="gt").odomprov is None
    with pytest.raises(TypeError, match="RGBDImages"):
        slam(torch.zeros(1, 2, 4, 4, 3))
    fr = frames(dev="cpu")
    vol = object.__new__(gs.TSDFVolume)
    vol._B = 1
    with pytest.raises(TypeError, match="TSDFVolume"):
        slam.step(gs.Pointclouds(), fr[:, 0])
    with pytest.raises(TypeError, match="RGBDImages"):
        slam.step(vol, fr.depth_image)
    with pytest.raises(TypeError, match="prev_frame"):
        slam.step(vol, fr[:, 0], fr.depth_image)
    with pytest.raises(ValueError, match="Sequence length"):
        slam.step(vol, fr[:, 0:2])
    vol._B = 2
    with pytest.raises(ValueError, match="Batch size"):
        slam.step(vol, fr[:, 0])
    vol._B = 1
    no_pose = gs.RGBDImages(fr.rgb_image[:, :1], fr.depth_image[:, :1], fr.intrinsics)
    with pytest.raises(ValueError, match="must have poses"):
        slam.step(vol, no_pose)
    with pytest.raises(ValueError, match="should have poses"):
        slam.step(vol, fr[:, 1], no_pose)
    # a volume that is not on a device
    with pytest.raises(ValueError, match="no CPU fallback"):
        KinectFusion(dims=DIMS, voxel_size=V, origin=ORIGINS[:1], device="cpu")(fr)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_ground_truth_odometry_is_integrate_of_the_sequence(B):
    fr = frames(B)
    volume, poses = kf(B, odom="gt")(fr)
    assert torch.equal(poses, fr.poses)
    whole = gs.TSDFVolume(DIMS, V, origin=ORIGINS[:B], trunc=TRUNC, device=DEV).integrate(fr)
    assert same_volume(volume, whole) and int((volume.weight > 0).sum()) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_forward_equals_steps_equals_the_hand_composition(B):
    fr = frames(B)
    slam = kf(B)
    volume, poses = slam(fr)
    assert poses.shape == (B, L, 4, 4) and torch.equal(poses[:, 0], fr.poses[:, 0])
    # frame by frame through step()
    vol_s, prev, got = slam.new_volume(B), None, []
    for s in range(L):
        live = fr[:, s]
        vol_s, p = slam.step(vol_s, live, prev)
        prev = live
        got.append(p[:, 0])
    assert torch.equal(torch.stack(got, 1), poses) and same_volume(vol_s, volume)
    # by hand from the public pieces
    vol_h = gs.TSDFVolume(DIMS, V, origin=ORIGINS[:B], trunc=TRUNC, device=DEV)
    pose = fr.poses[:, :1]
    for s in range(L):
        live = gs.RGBDImages(fr.rgb_image[:, s:s + 1], fr.depth_image[:, s:s + 1], fr.intrinsics, pose)
        if s > 0:
            target = vol_h.raycast_pointcloud(fr.intrinsics, pose, H, W, stride=4, step=None, min_weight=1.0)
            source = downsample_rgbdimages(live, 4)
            T = slam.odomprov.provide(target, source)
            pose = compose_transformations(T.squeeze(1), pose.squeeze(1)).unsqueeze(1)
            live = gs.RGBDImages(fr.rgb_image[:, s:s + 1], fr.depth_image[:, s:s + 1], fr.intrinsics, pose)
        assert torch.equal(pose[:, 0], poses[:, s]), s
        vol_h = vol_h.integrate(live)
    assert same_volume(vol_h, volume)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_trajectory_is_as_good_as_icpslam_up_to_the_grid(B):
    """Measured on the MI355X (B = 1; B = 2): ATE_kf 0.0047; 0.0047, 0.0044 m against ATE_icpslam 0.0304; 0.0304, 0.0280 m (ICPSLAM's nearest
    neighbours between two clouds of 15 cm spacing do not see a step of 1 cm: its poses stay where they started; the cast
    surface and the frame are sampled on the same rays)."""
    fr = frames(B)
    _, poses = kf(B)(fr)
    _, ref_poses = ICPSLAM(odom="icp", dsratio=4, device=DEV)(fr)
    ate_kf = absolute_trajectory_error(poses, fr.poses)
    ate_icp = absolute_trajectory_error(ref_poses, fr.poses)
    print("B", B, "ATE KinectFusion", ate_kf.tolist(), "ATE ICPSLAM", ate_icp.tolist())
    assert torch.isfinite(ate_kf).all()
    assert (ate_kf <= torch.clamp(2 * ate_icp, min=V)).all()
    assert not torch.equal(poses[:, 1:], fr.poses[:, :-1].expand_as(poses[:, 1:]))  # it moved: not the previous pose handed on


@pytest.mark.gpu
def test_a_volume_the_camera_does_not_see_raises_on_frame_1():
    fr = frames(2)
    slam = KinectFusion(dims=DIMS, voxel_size=V, origin=[ORIGINS[0], (50.0, 50.0, 50.0)], trunc=TRUNC, odom="icp", device=DEV)
    with pytest.raises(RuntimeError, match="frame 1, batch element 1"):
        slam(fr)
    empty = gs.RGBDImages(fr.rgb_image, torch.zeros_like(fr.depth_image), fr.intrinsics, fr.poses)
    vol, _ = kf(2).step(kf(2).new_volume(2), fr[:, 0])
    live = empty[:, 1]
    before = live.poses.clone()
    with pytest.raises(RuntimeError, match="KinectFusion: batch element 0: the frame has no valid pixel"):
        kf(2).step(vol, live, fr[:, 0])
    assert torch.equal(live.poses, before)  # a step that raises leaves the caller's frame as it was


@pytest.mark.gpu
@pytest.mark.parametrize("odom", ["icp", "gradicp"])
def test_gradients_reach_the_first_depth_through_raycast_icp_and_integrate(odom):
    base = frames(1)

    def run():
        d = base.depth_image.clone().requires_grad_(True)
        c = base.rgb_image.clone().requires_grad_(True)
        _, poses = kf(1, odom=odom)(gs.RGBDImages(c, d, base.intrinsics, base.poses))
        poses[:, -1].sum().backward()
        return poses.detach(), d.grad

    torch.use_deterministic_algorithms(True)
    try:
        (p0, g0), (p1, g1) = run(), run()
    finally:
        torch.use_deterministic_algorithms(False)
    assert g0 is not None and torch.isfinite(g0).all()
    assert int((g0[:, 0] != 0).sum()) > 50, "frame 0's depth is reached only through the volume that is cast"
    assert torch.equal(p0, p1) and torch.equal(g0, g1)
