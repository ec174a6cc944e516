"""pointclouds_from_rgbdimages (reference structures/utils.py:7-57) and its inverse, rgbdimages_from_pointclouds."""
import torch

from .. import ops
from .pointclouds import Pointclouds
from .rgbdimages import RGBDImages

__all__ = ["pointclouds_from_rgbdimages", "rgbdimages_from_pointclouds"]


def pointclouds_from_rgbdimages(rgbdimages: RGBDImages, *, global_coordinates: bool = True,
                                filter_missing_depths: bool = True) -> Pointclouds:
    """One-frame RGBDImages -> Pointclouds of its (valid) pixels in row-major order."""
    if not isinstance(rgbdimages, RGBDImages):
        raise TypeError("Expected rgbdimages to be of type gradslam.RGBDImages. Got {0}.".format(type(rgbdimages)))
    if not rgbdimages.shape[1] == 1:
        raise ValueError("Expected rgbdimages to have sequence length of 1. Got {0}.".format(rgbdimages.shape[1]))
    B = rgbdimages.shape[0]
    rgbdimages = rgbdimages.to_channels_last()
    vmap = rgbdimages.global_vertex_map if global_coordinates else rgbdimages.vertex_map
    nmap = rgbdimages.global_normal_map if global_coordinates else rgbdimages.normal_map
    rgb = rgbdimages.rgb_image
    if not filter_missing_depths:
        return Pointclouds(points=vmap.reshape(B, -1, 3).contiguous(), normals=nmap.reshape(B, -1, 3).contiguous(),
                           colors=rgb.reshape(B, -1, 3).contiguous())
    mask = rgbdimages.valid_depth_mask.squeeze(-1)  # (B,1,H,W)
    per_b = [ops.select_rows_multi([vmap[b].reshape(-1, 3), nmap[b].reshape(-1, 3), rgb[b].reshape(-1, 3)],
                                   mask[b].reshape(-1)) for b in range(B)]
    return Pointclouds(points=[p[0] for p in per_b], normals=[p[1] for p in per_b], colors=[p[2] for p in per_b])


def rgbdimages_from_pointclouds(pointclouds: Pointclouds, intrinsics, poses, height: int, width: int, *,
                                return_maps: bool = False):
    """Pointclouds -> the one-frame channels-last RGBDImages a camera (intrinsics (B,1,4,4), poses (B,1,4,4)) sees of it:
    every pixel shows the nearest map point that find_active_map_points puts on it -- rgb from its colour, depth its
    camera-frame z -- and zeros where there is none (an invalid depth).  The inverse of pointclouds_from_rgbdimages: a
    frame's cloud rendered into the frame's own camera gives the frame back.  Differentiable w.r.t. the cloud's points and
    colours and the poses.  With return_maps also a dict: `index` (B,1,H,W) int32 (the point shown, -1: none),
    `global_vertex_map` (B,1,H,W,3) (its position) and `global_normal_map` (its normal; None for a cloud without normals)."""
    if not isinstance(pointclouds, Pointclouds):
        raise TypeError("Expected pointclouds to be of type gradslam.Pointclouds. Got {0}.".format(type(pointclouds)))
    if not pointclouds.has_colors:
        raise ValueError("Pointclouds must have colors to be rendered to RGBDImages")
    B = len(pointclouds)
    for name, val in (("intrinsics", intrinsics), ("poses", poses)):
        if not torch.is_tensor(val) or tuple(val.shape) != (B, 1, 4, 4):
            raise ValueError("Expected {0} to have shape {1}. Got {2} instead".format(
                name, (B, 1, 4, 4), tuple(val.shape) if torch.is_tensor(val) else type(val)))
    H, W = int(height), int(width)
    index, depth, pts, nrm, rgb = ops.render_map(pointclouds.points_padded, pointclouds.normals_padded, pointclouds.colors_padded,
                                                 pointclouds._counts_i32(), poses, intrinsics, H, W)
    out = RGBDImages(rgb.unsqueeze(1), depth.view(B, 1, H, W, 1), intrinsics, poses)
    if not return_maps:
        return out
    return out, {"index": index.unsqueeze(1), "global_vertex_map": pts.unsqueeze(1),
                 "global_normal_map": None if nrm is None else nrm.unsqueeze(1)}
