"""SDFOdometryProvider: a frame aligned directly against a TSDF volume's distance field (no counterpart in the reference; Bylow,
Sturm, Kerl, Kahl, Cremers, RSS 2013).  No ray cast, no association, no cloud, no host read: every observed voxel near the
surface constrains the pose, not only the first zero crossing along the previous camera's rays."""
from typing import Optional, Sequence, Union

import torch

from .. import ops
from ..structures.rgbdimages import RGBDImages
from ..structures.tsdfvolume import TSDFVolume
from .base import OdometryProvider, check_init, check_levels_numiters

__all__ = ["SDFOdometryProvider"]


class SDFOdometryProvider(OdometryProvider):
    """`provide(volume, source_frames)` returns the WORLD-frame transform (B, 1, 4, 4) that moves the frames, under the poses they
    carry, onto the volume's surface -- what the ICP providers return for a map cloud and a posed frame cloud, so the new pose is
    `compose_transformations(transform, poses)`.  `numiters`: Gauss-Newton iterations per level, finest first (an int: that
    count at every level); level l uses the pixel grid [::stride 2^l, ::stride 2^l] (there is no pyramid); a pixel counts where
    all 8 voxels around its point have weight >= `min_weight` and none of them is clamped free space.

    `differentiable=False` (the default): no gradients; under autograd a depth, poses, `init` or a volume tsdf that requires one is
    refused rather than cut silently (the stance of RGBDOdometryProvider(differentiable=False)).  `differentiable=True`: the
    transform carries the graph (ops.sdf_odometry: one autograd node, the decisions of the forward pass held constant) and
    gradients reach the depth, rows 0..2 of the poses and of `init`, and the volume's tsdf; never the intrinsics, which are refused
    when they require a gradient.  `last_info` is not differentiable."""

    def __init__(self, numiters: Union[int, Sequence[int]] = (10, 5, 3), levels: int = 3, stride: int = 1, min_weight: float = 1.0,
                 damp: float = 1e-8, differentiable: bool = False):
        numiters = check_levels_numiters("SDFOdometryProvider", numiters, levels)
        if not isinstance(differentiable, bool):
            raise TypeError("SDFOdometryProvider: differentiable should be a bool. Got {!r}.".format(differentiable))
        if not isinstance(stride, int) or isinstance(stride, bool) or stride < 1:
            raise ValueError("SDFOdometryProvider: stride should be a positive integer. Got {!r}.".format(stride))
        self.numiters = numiters
        self.levels = levels
        self.stride = stride
        self.min_weight = min_weight
        self.damp = damp
        self.differentiable = differentiable
        self.last_info = None  # (B, levels, 4) on the device, unsynchronised: cnt, err, status bits, iterations per level

    def provide(self, volume: TSDFVolume, source_frames: RGBDImages, init: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not isinstance(volume, TSDFVolume):
            raise TypeError("Expected volume to be of type gradslam.TSDFVolume. Got {0}.".format(type(volume)))
        if not isinstance(source_frames, RGBDImages):
            raise TypeError("Expected source_frames to be of type gradslam.RGBDImages. Got {0}.".format(type(source_frames)))
        if init is not None and not torch.is_tensor(init):
            raise TypeError("Expected init to be of type tensor or None. Got {0}.".format(type(init)))
        if len(volume) != len(source_frames):
            raise ValueError("Batch size of the volume and of source_frames should be equal ({0} != {1})".format(
                len(volume), len(source_frames)))
        if source_frames.shape[1] != 1:
            raise ValueError("Sequence length of source_frames must be 1, but was {0}.".format(source_frames.shape[1]))
        if not source_frames.has_poses:
            raise ValueError("source_frames must have poses (the pose the frame is tracked from).")
        B = len(volume)
        check_init(init, B)
        tensors = [source_frames.depth_image, source_frames.poses, init, volume.tsdf]
        if not self.differentiable and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
            raise NotImplementedError("SDFOdometryProvider: gradients are not implemented; detach the frames, the poses, init and "
                                      "the volume, or call under torch.no_grad().")
        src = source_frames.to_channels_last() if source_frames.channels_first else source_frames
        T, info = ops.sdf_odometry(src.depth_image[:, 0], src.intrinsics, src.poses[:, 0], volume.tsdf, volume.weight, volume.origin,
                                   volume.voxel_size, volume.trunc, init, self.numiters, self.levels, self.stride, self.min_weight,
                                   self.damp, differentiable=self.differentiable)
        self.last_info = info
        return T.unsqueeze(1)
