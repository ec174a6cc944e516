"""Map and trajectory metrics (the reference ships `gradslam.metrics` empty).

Map metrics compare two `Pointclouds` through their exact two-sided nearest neighbours, computed by one HIP call
(`ops.chamfer`): `chamfer_distance` is differentiable w.r.t. both clouds' points, `nearest_neighbor` returns the
neighbours themselves, `reconstruction_metrics` the usual evaluation figures.  Trajectory metrics
(`absolute_trajectory_error`, `relative_pose_error`) are plain, differentiable torch on (B, L, 4, 4) poses and run on any
device.
"""
from .maps import chamfer_distance, nearest_neighbor, reconstruction_metrics
from .trajectory import absolute_trajectory_error, relative_pose_error

__all__ = ["chamfer_distance", "nearest_neighbor", "reconstruction_metrics", "absolute_trajectory_error",
           "relative_pose_error"]
