"""KinectFusion: frame loop = ray-cast the volume from the previous pose, ICP against the cast surface, integrate
(the paper's volumetric pipeline; the reference ships no counterpart)."""
import warnings
from typing import Optional, Union

import torch
import torch.nn as nn

from ..geometry.geometryutils import compose_transformations
from ..odometry.gradicp import GradICPOdometryProvider
from ..odometry.icp import ICPOdometryProvider
from ..odometry.icputils import downsample_rgbdimages
from ..odometry.rgbd import RGBDOdometryProvider
from ..odometry.sdf import SDFOdometryProvider
from ..structures.rgbdimages import RGBDImages
from ..structures.tsdfvolume import TSDFVolume

__all__ = ["KinectFusion"]


class KinectFusion(nn.Module):
    r"""Volumetric SLAM: the map is a TSDFVolume of `dims` voxels of edge `voxel_size` at `origin` (`trunc`, `max_weight`, `color`
    as in TSDFVolume).  Per frame s >= 1 with an ICP odometry (`odom` "icp" or "gradicp", parameters as in ICPSLAM):

        target = volume.raycast_pointcloud(K, pose_{s-1}, H, W, stride=dsratio, step=step, min_weight=min_weight)
        source = downsample_rgbdimages(live frame carrying pose_{s-1}, dsratio)
        pose_s = compose_transformations(odomprov.provide(target, source), pose_{s-1})

    and the frame is integrated under pose_s.  Frame 0 takes `frames.poses[:, 0]` if given, else the identity.  With
    `odom="gt"` the frames' poses are used.  Under autograd every piece is a node of its own: gradients reach the depths and
    colours through raycast, ICP and integrate (never the intrinsics).  With `pose_gradients=False` (the default) the volume
    takes its poses as constants: raycast, raycast_pointcloud and integrate are handed detached copies, while the frames'
    poses and the returned poses stay attached, so a gradient reaches an earlier frame through the tsdf values alone.  With
    `pose_gradients=True` they are handed over attached and the chain pose_{s-1} -> raycast -> ICP -> pose_s -> integrate ->
    volume -> raycast .. is whole: a gradient also flows through where each frame was put.  The volume should hold what the
    cameras see (or `dist_thresh` be set): ICP pairs every frame point with its nearest cast point, and frame points beyond the
    volume pair with the rim of the cast surface.

    `odom="rgbd"` tracks frame to model with the dense photometric + depth alignment of RGBDOdometryProvider (`numiters`, `damp`,
    `levels`, `lambda_geo`; it needs `color=True`):

        target = volume.raycast(K, pose_{s-1}, H, W, step=step, min_weight=min_weight)     (the coloured image of the model)
        pose_s = compose_transformations(odomprov.provide(target, live frame), pose_{s-1})

    at full resolution (`dsratio` and `dist_thresh` are not used).  The alignment is differentiated only with
    `odom_gradients=True`, which builds the provider with `differentiable=True`: gradients then reach the depths and colours of
    the frames through the alignment too (its decisions held constant, see RGBDOdometryProvider), and together with
    `pose_gradients=True` the chain pose_{s-1} -> coloured cast -> alignment -> pose_s -> integrate is attached like the ICP
    branch's.  With `odom_gradients=False` (the default) it is as it was: under autograd with inputs that require gradients
    `provide` raises NotImplementedError, whatever `pose_gradients` says.  A camera that sees nothing of the volume, or a frame without valid
    pixels, leaves the pose where it was and sets the status bit in `odomprov.last_info` (nothing synchronises the host).

    `odom="sdf"` tracks the frame directly against the volume's distance field with SDFOdometryProvider (`numiters`, `levels`,
    `damp`, `min_weight`; `stride = dsratio`, the ICP branch's pixel subset; colour is not needed):

        pose_s = compose_transformations(odomprov.provide(volume, live frame carrying pose_{s-1}), pose_{s-1})

    There is no ray cast, no cloud and no host read.  A camera that sees nothing of the volume leaves the pose where it was and
    sets the status bit, as `odom="rgbd"` does.  `odom="sdf"` carries no gradients: `odom_gradients=True` is refused, and under
    autograd inputs that require gradients raise NotImplementedError.  `odom="gradsdf"` (named as "icp" / "gradicp" are) is the
    same tracker built with `differentiable=True`: the same poses bit for bit, and the transform carries the graph -- gradients
    reach the live frame's depth, the previous pose and the volume's tsdf (so the depths of the frames fused before) through
    where the frame was put; the volume and the previous poses are handed over as they are.  `odom_gradients` does not apply to
    it and is refused."""

    def __init__(self, *, dims, voxel_size, origin=(0.0, 0.0, 0.0), trunc=None, max_weight: float = 128.0, color: bool = True,
                 odom: str = "gradicp", dsratio: int = 4, numiters: int = 20, damp: float = 1e-8,
                 dist_thresh: Union[float, int, None] = None, lambda_max: Union[float, int] = 2.0, B: Union[float, int] = 1.0,
                 B2: Union[float, int] = 1.0, nu: Union[float, int] = 200.0, step: Optional[float] = None, min_weight: float = 1.0,
                 device: Union[torch.device, str, None] = None, levels: int = 3, lambda_geo: float = 0.968,
                 pose_gradients: bool = False, odom_gradients: bool = False):
        super().__init__()
        if odom not in ["gt", "icp", "gradicp", "rgbd", "gradsdf", "sdf"]:
            msg = "odometry method ({}) not supported for KinectFusion. ".format(odom)
            msg += "Currently supported odometry modules for KinectFusion are: 'gt', 'icp', 'gradicp', 'rgbd', 'gradsdf', 'sdf'"
            raise ValueError(msg)
        if odom == "rgbd" and not color:
            raise ValueError("KinectFusion: odom='rgbd' tracks against the colours of the volume and needs color=True.")
        if not isinstance(dsratio, int) or isinstance(dsratio, bool) or dsratio < 1:
            raise ValueError("KinectFusion: dsratio should be a positive integer. Got {!r}.".format(dsratio))
        if not isinstance(pose_gradients, bool):
            raise TypeError("KinectFusion: pose_gradients should be a bool. Got {!r}.".format(pose_gradients))
        if not isinstance(odom_gradients, bool):
            raise TypeError("KinectFusion: odom_gradients should be a bool. Got {!r}.".format(odom_gradients))
        if odom_gradients and odom != "rgbd":
            raise ValueError("KinectFusion: odom_gradients belongs to odom='rgbd' (the ICP providers and odom='gradsdf' always "
                             "carry gradients; odom='sdf' never does).")
        odomprov = None
        if odom == "icp":
            odomprov = ICPOdometryProvider(numiters, damp, dist_thresh)
        elif odom == "gradicp":
            odomprov = GradICPOdometryProvider(numiters, damp, dist_thresh, lambda_max, B, B2, nu)
        elif odom == "rgbd":
            odomprov = RGBDOdometryProvider(numiters, levels, lambda_geo, damp=damp, differentiable=odom_gradients)
        elif odom in ("sdf", "gradsdf"):
            odomprov = SDFOdometryProvider(numiters, levels, stride=dsratio, min_weight=min_weight, damp=damp,
                                           differentiable=odom == "gradsdf")
        self.odom = odom
        self.odomprov = odomprov
        self.dsratio = dsratio
        self.step_size = step
        self.min_weight = min_weight
        self.pose_gradients = pose_gradients
        self.volume_args = dict(dims=dims, voxel_size=voxel_size, origin=origin, trunc=trunc, max_weight=max_weight, color=color)
        self.device = torch.device(device) if device is not None else torch.device("cuda")

    def new_volume(self, batch_size: int) -> TSDFVolume:
        """An empty volume for `batch_size` sequences (raises for a device that is no HIP device)."""
        return TSDFVolume(batch_size=batch_size, device=self.device, **self.volume_args)

    def forward(self, frames: RGBDImages):
        """frames (B, L, ...) -> (TSDFVolume, recovered poses (B, L, 4, 4))."""
        if not isinstance(frames, RGBDImages):
            raise TypeError("Expected frames to be of type gradslam.RGBDImages. Got {0}.".format(type(frames)))
        batch_size, seq_len = frames.shape[:2]
        volume = self.new_volume(batch_size)
        recovered = []
        prev_frame = None
        for s in range(seq_len):  # true serial dependence: pose s needs the volume of the frames before it
            live_frame = frames[:, s].to(self.device)
            if s == 0 and live_frame.poses is None:
                live_frame.poses = torch.eye(4, dtype=torch.float, device=self.device).view(1, 1, 4, 4).repeat(batch_size, 1, 1, 1)
            volume, live_frame.poses = self._step(volume, live_frame, prev_frame, "frame {}, ".format(s))
            prev_frame = live_frame if self.odom != "gt" else None
            recovered.append(live_frame.poses[:, 0])
        return volume, torch.stack(recovered, dim=1)

    def step(self, volume: TSDFVolume, live_frame: RGBDImages, prev_frame: Optional[RGBDImages] = None):
        """One step on `live_frame` (sequence length 1) -> (the volume with the frame integrated, live poses (B, 1, 4, 4)).
        `live_frame.poses` is set to the recovered poses once they exist: a step that raises leaves the frame as it was."""
        return self._step(volume, live_frame, prev_frame, "")

    def _step(self, volume, live_frame, prev_frame, where):
        if not isinstance(volume, TSDFVolume):
            raise TypeError("Expected volume to be of type gradslam.TSDFVolume. Got {0}.".format(type(volume)))
        if not isinstance(live_frame, RGBDImages):
            raise TypeError("Expected live_frame to be of type gradslam.RGBDImages. Got {0}.".format(type(live_frame)))
        live_frame.poses = self._localize(volume, live_frame, prev_frame, where)
        fused = live_frame
        if not self.pose_gradients and live_frame.poses.requires_grad:  # the volume takes the pose as a constant
            fused = RGBDImages(live_frame.rgb_image, live_frame.depth_image, live_frame.intrinsics, live_frame.poses.detach(),
                               channels_first=live_frame.channels_first)
        return volume.integrate(fused), live_frame.poses

    def _volume_poses(self, poses):
        """The poses as the volume's raycast receives them: attached only with pose_gradients=True."""
        return poses if self.pose_gradients else poses.detach()

    def _localize(self, volume: TSDFVolume, live_frame: RGBDImages, prev_frame: Optional[RGBDImages], where: str = ""):
        if not isinstance(prev_frame, (RGBDImages, type(None))):
            raise TypeError("Expected prev_frame to be of type gradslam.RGBDImages or None. Got {0}.".format(type(prev_frame)))
        if live_frame.shape[1] != 1:
            raise ValueError("Sequence length of live_frame must be 1, but was {0}.".format(live_frame.shape[1]))
        if len(live_frame) != len(volume):
            raise ValueError("Batch size of the frames and of the volume must match: ({0} != {1})".format(len(live_frame), len(volume)))
        if prev_frame is not None:
            if self.odom == "gt":
                warnings.warn("`prev_frame` is not used when using `odom='gt'` (should be None)")
            elif not prev_frame.has_poses:
                raise ValueError("`prev_frame` should have poses, but did not.")
        if prev_frame is None or self.odom == "gt":
            if not live_frame.has_poses:
                raise ValueError("`live_frame` must have poses when `prev_frame` is None or `odom='gt'`.")
            return live_frame.poses

        if live_frame.channels_first:
            live_frame = live_frame.to_channels_last()
        H, W = live_frame.shape[2:4]
        if self.odom in ("sdf", "gradsdf"):  # no cast, no cloud, no host read: the frame under the previous pose against the volume itself
            source = RGBDImages(live_frame.rgb_image, live_frame.depth_image, live_frame.intrinsics, prev_frame.poses)
            transform = self.odomprov.provide(volume, source)
            return compose_transformations(transform.squeeze(1), prev_frame.poses.squeeze(1)).unsqueeze(1)
        if self.odom == "rgbd":
            cast = volume.raycast(live_frame.intrinsics, self._volume_poses(prev_frame.poses), H, W, step=self.step_size,
                                  min_weight=self.min_weight)
            # (both frames carry the live frame's intrinsics tensor: the cast's own is a copy of it)
            target = RGBDImages(cast.rgb_image, cast.depth_image, live_frame.intrinsics, prev_frame.poses)
            source = RGBDImages(live_frame.rgb_image, live_frame.depth_image, live_frame.intrinsics, prev_frame.poses)
            transform = self.odomprov.provide(target, source)
            return compose_transformations(transform.squeeze(1), prev_frame.poses.squeeze(1)).unsqueeze(1)
        target = volume.raycast_pointcloud(live_frame.intrinsics, self._volume_poses(prev_frame.poses), H, W, stride=self.dsratio,
                                           step=self.step_size, min_weight=self.min_weight)
        # the frame under the previous pose, as a frame of its own: the caller's keeps its poses until the step has succeeded
        source = downsample_rgbdimages(RGBDImages(live_frame.rgb_image, live_frame.depth_image, live_frame.intrinsics, prev_frame.poses),
                                       self.dsratio)
        for b in range(len(volume)):  # never ICP on an empty cloud
            if target._counts[b] == 0:
                raise RuntimeError("KinectFusion: {}batch element {}: the camera of the previous pose sees nothing of the "
                                   "volume (no ray hits an observed surface).".format(where, b))
            if source._counts[b] == 0:
                raise RuntimeError("KinectFusion: {}batch element {}: the frame has no valid pixel.".format(where, b))
        transform = self.odomprov.provide(target, source)
        return compose_transformations(transform.squeeze(1), prev_frame.poses.squeeze(1)).unsqueeze(1)
