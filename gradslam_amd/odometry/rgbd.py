"""RGBDOdometryProvider: dense photometric + depth alignment of two RGB-D frames over an image pyramid (no counterpart in the
reference; Steinbruecker / Kerl, Park-Zhou-Koltun 2017).  The colour constrains what point-to-plane ICP leaves free on flat
surfaces: the in-plane translations and the rotation about the normal."""
from typing import Optional, Sequence, Union

import torch

from .. import ops
from ..structures.rgbdimages import RGBDImages
from .base import OdometryProvider, check_init, check_levels_numiters

__all__ = ["RGBDOdometryProvider"]


class RGBDOdometryProvider(OdometryProvider):
    """`provide(target_frames, source_frames)` returns the transform (B, 1, 4, 4) that takes source-camera coordinates to
    target-camera coordinates -- what the ICP providers return for a frame cloud and a map cloud, so it composes with the previous
    pose the same way.  `numiters`: Gauss-Newton iterations per pyramid level, finest first (an int: that count at every level);
    `lambda_geo` weighs the depth term against the photometric one; pixels whose depths differ by more than `depth_diff_max`
    are left out; intensities are `rgb_scale` times the luma of the colours.

    Gradients.  With `differentiable=False` (the default) the result carries no gradient, and frames or an `init` that require
    one are refused under autograd rather than cut silently.  With `differentiable=True` the returned T carries the graph (one
    autograd node, ops.rgbd_odometry): gradients reach the depth and the colours of both frames and rows 0..2 of `init`, with
    every decision of the forward pass held constant (which pixels are valid, the cells they fall in, the pyramid's foreground
    selection, which steps were applied).  The scalar parameters and `last_info` are not differentiable, nor are the intrinsics:
    intrinsics that require a gradient are refused, not cut silently."""

    def __init__(self, numiters: Union[int, Sequence[int]] = (10, 5, 3), levels: int = 3, lambda_geo: float = 0.968,
                 depth_diff_max: float = 0.07, damp: float = 1e-8, rgb_scale: float = 1.0 / 255.0, differentiable: bool = False):
        numiters = check_levels_numiters("RGBDOdometryProvider", numiters, levels)
        self.numiters = numiters
        self.levels = levels
        self.lambda_geo = lambda_geo
        self.depth_diff_max = depth_diff_max
        self.damp = damp
        self.rgb_scale = rgb_scale
        if not isinstance(differentiable, bool):
            raise TypeError("RGBDOdometryProvider: differentiable should be a bool. Got {!r}.".format(differentiable))
        self.differentiable = differentiable
        self.last_info = None  # (B, levels, 4) on the device, unsynchronised: cnt, err, status bits, iterations per level

    def provide(self, target_frames: RGBDImages, source_frames: RGBDImages, init: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not isinstance(target_frames, RGBDImages):
            raise TypeError("Expected target_frames to be of type gradslam.RGBDImages. Got {0}.".format(type(target_frames)))
        if not isinstance(source_frames, RGBDImages):
            raise TypeError("Expected source_frames to be of type gradslam.RGBDImages. Got {0}.".format(type(source_frames)))
        if init is not None and not torch.is_tensor(init):
            raise TypeError("Expected init to be of type tensor or None. Got {0}.".format(type(init)))
        if len(target_frames) != len(source_frames):
            raise ValueError("Batch size of target_frames and source_frames should be equal ({0} != {1})".format(
                len(target_frames), len(source_frames)))
        for name, fr in (("target_frames", target_frames), ("source_frames", source_frames)):
            if fr.shape[1] != 1:
                raise ValueError("Sequence length of {0} must be 1, but was {1}.".format(name, fr.shape[1]))
        if target_frames.shape[2:] != source_frames.shape[2:]:
            raise ValueError("Image size of target_frames and source_frames should be equal ({0} != {1})".format(
                tuple(target_frames.shape[2:]), tuple(source_frames.shape[2:])))
        B = len(target_frames)
        check_init(init, B)
        tensors = [target_frames.rgb_image, target_frames.depth_image, target_frames.intrinsics, source_frames.rgb_image,
                   source_frames.depth_image, source_frames.intrinsics, init]
        if not self.differentiable and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
            raise NotImplementedError("RGBDOdometryProvider: gradients are not implemented for a provider built with "
                                      "differentiable=False; build it with differentiable=True, detach the frames or call "
                                      "under torch.no_grad().")
        Kt, Ks = target_frames.intrinsics, source_frames.intrinsics
        if self.differentiable and torch.is_grad_enabled() and (Kt.requires_grad or Ks.requires_grad):
            raise NotImplementedError("RGBDOdometryProvider: gradients with respect to the intrinsics are not implemented; detach "
                                      "them (refused rather than cut silently).")
        if Kt is not Ks and (Kt.device != Ks.device or not torch.equal(Kt, Ks)):  # (two tensors: compared, one synchronisation)
            raise ValueError("Intrinsics of target_frames and source_frames should be equal.")
        tgt = target_frames.to_channels_last() if target_frames.channels_first else target_frames
        src = source_frames.to_channels_last() if source_frames.channels_first else source_frames
        T, info = ops.rgbd_odometry(tgt.depth_image[:, 0], tgt.rgb_image[:, 0], src.depth_image[:, 0], src.rgb_image[:, 0],
                                    tgt.intrinsics, init, self.numiters, self.levels, self.lambda_geo, self.depth_diff_max, self.damp,
                                    self.rgb_scale, differentiable=self.differentiable)
        self.last_info = info
        return T.unsqueeze(1)
