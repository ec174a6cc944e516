"""TSDFVolume: a dense truncated signed-distance grid per batch element, the volumetric map of KinectFusion-style dense SLAM.

Posed RGB-D frames are fused into it (`integrate`), a surface is taken out of it as a `Pointclouds` (`extract_pointcloud`) or
as a triangle mesh (`extract_mesh`); all of it is differentiable.  The reference ships no counterpart (the paper describes one).  All arithmetic runs in the HIP
kernels of csrc/tsdf.hip and csrc/mesh.hip; nothing here computes on the CPU.
"""
from typing import Optional

import torch

from .. import ops
from .meshes import Meshes
from .pointclouds import Pointclouds
from .rgbdimages import RGBDImages

__all__ = ["TSDFVolume"]


class TSDFVolume(object):
    r"""A batch of B dense volumes of `dims = (nx, ny, nz)` voxels of edge `voxel_size`; `origin` ((3,) or (B, 3)) is the corner
    of voxel (0, 0, 0), so voxel i has its centre at origin + (i + 0.5) voxel_size.

    State, fp32, x fastest: `tsdf` (B, nz, ny, nx), 1 where unobserved; `weight` (B, nz, ny, nx), 0 where unobserved; `color`
    (B, nz, ny, nx, 3), 0 where unobserved (None with `color=False`).  `trunc` (default 4 voxel_size) is the truncation distance,
    `max_weight` (default 128) caps the running average's weight.  B is the number of origins given, or `batch_size`."""

    def __init__(self, dims, voxel_size, origin=(0.0, 0.0, 0.0), trunc=None, max_weight=128.0, batch_size: Optional[int] = None,
                 color: bool = True, device="cuda"):
        op = "TSDFVolume"
        self.dims = ops._tsdf_dims(dims, op)
        self.voxel_size = ops._positive(voxel_size, "voxel_size", op)
        self.trunc = ops._positive(4.0 * self.voxel_size if trunc is None else trunc, "trunc", op)
        self.max_weight = ops._positive(max_weight, "max_weight", op)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("{}: device is {}; TSDF volumes only live on a HIP device (no CPU fallback is provided).".format(op, self.device))
        if batch_size is None:
            shape = tuple(origin.shape) if torch.is_tensor(origin) else None
            if shape is None:
                try:
                    shape = tuple(torch.as_tensor(origin, dtype=torch.float32).shape)
                except (TypeError, ValueError, RuntimeError):
                    shape = ()
            batch_size = shape[0] if len(shape) == 2 else 1
        if not isinstance(batch_size, int) or isinstance(batch_size, bool) or not 1 <= batch_size <= 65535:
            raise ValueError("{}: batch_size should be an integer in 1 .. 65535. Got {!r}.".format(op, batch_size))
        self._B = batch_size
        self.origin = ops.tsdf_origin(origin, self._B, self.device, op)
        nx, ny, nz = self.dims
        self.tsdf = torch.ones((self._B, nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((self._B, nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((self._B, nz, ny, nx, 3), dtype=torch.float32, device=self.device) if color else None

    def __len__(self):
        return self._B

    @property
    def has_colors(self) -> bool:
        return self.color is not None

    def _with_state(self, tsdf, weight, color):
        out = object.__new__(type(self))
        out.__dict__.update(self.__dict__)
        out.tsdf, out.weight, out.color = tsdf, weight, color
        return out

    def detach(self):
        return self._with_state(self.tsdf.detach(), self.weight, None if self.color is None else self.color.detach())

    # ------------------------------------------------------------------ integration
    def integrate(self, rgbdimages: RGBDImages, inplace: bool = False):
        r"""Fuse a (B, L) batch of posed frames: per voxel and frame, in order, the voxel's centre is projected with the map's own
        rule (the pixel `find_active_map_points` would put a map point on); with d the pixel's depth and z the centre's depth,
        sdf = d - z; frames with no pixel, no depth or sdf < -trunc leave the voxel alone, the others update

            tsdf <- (W tsdf + min(1, sdf / trunc)) / (W + 1),   color likewise with the pixel's rgb,   W <- min(W + 1, max_weight).

        Exactly what integrating the frames one at a time gives.  Returns a NEW TSDFVolume, or this one updated with
        `inplace=True` (when a gradient is being recorded the state is written to fresh tensors either way).  Differentiable
        w.r.t. the depth and rgb images, the previous tsdf / color and the poses (through the camera-frame depth of the voxel
        centres; the pixel a voxel falls on, the skips and the weight cap are constants of the graph; the pose adjoint is
        computed only when `rgbdimages.poses` requires a gradient); not w.r.t. the intrinsics and the weights."""
        if not isinstance(rgbdimages, RGBDImages):
            raise TypeError("Expected rgbdimages to be of type gradslam.RGBDImages. Got {}.".format(type(rgbdimages)))
        if not rgbdimages.has_poses:
            raise ValueError("TSDFVolume.integrate: the frames need poses (rgbdimages.poses is None).")
        if len(rgbdimages) != self._B:
            raise ValueError("Batch size of the frames and of the volume must match: ({0} != {1})".format(len(rgbdimages), self._B))
        depth, rgb = rgbdimages._cl(rgbdimages.depth_image), rgbdimages._cl(rgbdimages.rgb_image)
        args = (depth, rgb if self.has_colors else None, rgbdimages.intrinsics, rgbdimages.poses)
        cfg = (self.origin, self.voxel_size, self.trunc, self.max_weight)
        grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                               for t in (depth, rgb, self.tsdf, self.color, rgbdimages.poses))
        if grad:
            tsdf, weight, color = ops.tsdf_integrate(*args, self.tsdf, self.weight, self.color, *cfg)
        else:
            tsdf, weight, color = ops.tsdf_integrate_raw(*args, self.tsdf, self.weight, self.color, *cfg, inplace=inplace)
        if inplace:
            self.tsdf, self.weight, self.color = tsdf, weight, color
            return self
        return self._with_state(tsdf, weight, color)

    # ------------------------------------------------------------------ extraction
    def extract_pointcloud(self, min_weight: float = 1.0) -> Pointclouds:
        r"""The surface as a Pointclouds with points, normals and (for a volume with colours) colours: one point on every grid
        edge whose two voxels are observed (weight >= min_weight) and lie on different sides of the surface, placed by linear
        interpolation of tsdf; colours interpolated the same way; normals from the tsdf differences of the observed
        neighbours, pointing into free space.  Points come in ascending edge order (voxel, then axis).  Differentiable w.r.t.
        tsdf and color (which edges cross is a constant of the graph; normals carry no gradient).  One host synchronisation
        (the sizes)."""
        state = (self.tsdf, self.weight, self.color, self.origin, self.voxel_size, min_weight)
        with torch.no_grad():
            n_points = ops.tsdf_extract_raw(*state, cap=0)[4]
        counts = n_points.tolist()  # the one host synchronisation
        cap = max(counts)
        out = Pointclouds(device=self.device)
        out._B = self._B
        if cap > 0:
            points, normals, colors, _, _ = ops.tsdf_extract(*state, cap=cap)
        else:  # nothing observed yet: padded attributes without rows, like the counts
            empty = lambda: torch.zeros((self._B, 0, 3), dtype=torch.float32, device=self.device)
            points, normals, colors = empty(), empty(), (empty() if self.has_colors else None)
        out._adopt_padded(points, normals, colors, None)
        out._set_counts(counts)
        return out

    def extract_mesh(self, min_weight: float = 1.0) -> Meshes:
        r"""The surface as a Meshes (marching cubes).  The vertices, normals and colours are `extract_pointcloud(min_weight)`'s,
        bit for bit and in its order (the same call, the same autograd node); the faces index those rows.  A cube of 8
        neighbouring voxels emits triangles iff all 8 are observed, so a vertex on the rim of the observed region may be
        referenced by no face: such vertices are kept (the rows stay the point cloud's).  Faces come in ascending cube id and
        run counter-clockwise seen from free space: the face normals point the way the vertex normals do.  Where the volume
        is observed the mesh is closed and manifold (the case table resolves an ambiguous cube face from that face's signs
        alone, so neighbouring cubes agree).  Anything computed from `verts` or `colors` is differentiable w.r.t. tsdf and
        color (which edges cross and which cubes emit are constants of the graph).  One host synchronisation (both sizes).
        An empty volume gives B meshes without vertices and faces."""
        state = (self.tsdf, self.weight, self.color, self.origin, self.voxel_size, min_weight)
        with torch.no_grad():
            n_points = ops.tsdf_extract_raw(*state, cap=0)[4]
            n_faces = ops.tsdf_faces_raw(self.tsdf, self.weight, min_weight, None, None, fcap=0)[1]
        sizes = torch.stack([n_points, n_faces]).tolist()  # the one host synchronisation
        vcap, fcap = max(sizes[0]), max(sizes[1])
        B = self._B
        if vcap > 0:
            verts, normals, colors, edge, n_pts = ops.tsdf_extract(*state, cap=vcap)
        else:
            empty = lambda: torch.zeros((B, 0, 3), dtype=torch.float32, device=self.device)
            verts, normals, colors = empty(), empty(), (empty() if self.has_colors else None)
        if fcap > 0:
            faces, _ = ops.tsdf_faces_raw(self.tsdf, self.weight, min_weight, edge, n_pts, fcap=fcap, points_fit=True)
        else:
            faces = torch.full((B, 0, 3), -1, dtype=torch.int32, device=self.device)
        return Meshes._from_padded(verts, faces, normals, colors, sizes[0], sizes[1])

    # ------------------------------------------------------------------ ray casting
    def _cast(self, intrinsics, poses, height, width, stride, step, near, far, min_weight):
        op = "TSDFVolume.raycast"
        for name, t in (("intrinsics", intrinsics), ("poses", poses)):
            if not torch.is_tensor(t):
                raise TypeError("{}: expected {} to be a tensor; got {}".format(op, name, type(t)))
        if poses.ndim != 4 or poses.shape[0] != self._B:
            raise ValueError("Batch size of the poses and of the volume must match: poses {} for a volume of {}.".format(
                tuple(poses.shape), self._B))
        if intrinsics.numel() != 16 * self._B:
            raise ValueError("Batch size of the intrinsics and of the volume must match: intrinsics {} for a volume of {}.".format(
                tuple(intrinsics.shape), self._B))
        step = 0.5 * self.trunc if step is None else step
        far = float("inf") if far is None else far
        state = (self.tsdf, self.weight, self.color, self.origin, self.voxel_size, intrinsics, poses, height, width, stride, step, near,
                 far, min_weight)
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (self.tsdf, self.color, poses)):
            return ops.tsdf_raycast(*state)
        return ops.tsdf_raycast_raw(*state)

    def raycast(self, intrinsics, poses, height: int, width: int, *, stride: int = 1, step: Optional[float] = None, near: float = 0.0,
                far: Optional[float] = None, min_weight: float = 1.0, return_normals: bool = False):
        r"""The volume seen from the cameras `intrinsics` (B, 1, 4, 4), `poses` (B, L, 4, 4) (camera-to-world) of height x width
        images, on the [::stride, ::stride] pixel grid: per pixel the ray is sampled every `step` (default trunc / 2) of space,
        at depths near <= z <= far; a sample is observed iff the 8 voxels around it have weight >= min_weight, its value is
        their trilinear interpolant; the first observed sample behind the surface (tsdf < 0) ends the ray, which hits iff the
        sample before it is observed and in front (a ray that comes out of unobserved space, or starts inside, misses); the hit
        is placed by linear interpolation between the two.  Returns a channels-last RGBDImages of the cast depth (z, not range;
        0 on a miss) and colour (zero for a volume without colours) with the given poses and the intrinsics of the strided grid
        (fx, fy, cx, cy divided by stride), so that its vertex maps are the hit points.  `return_normals=True` also returns the
        (B, L, Ho, Wo, 3) image of global normals (the gradient of the interpolant, pointing into free space; 0 on a miss).
        Differentiable w.r.t. tsdf, color and the poses (which sample ends a ray, whether it hits and the cells of its samples
        are constants of the graph; normals carry no gradient); not w.r.t. the intrinsics and the weights.  Poses that require
        a gradient stay attached to the returned frames, so their global vertex map carries the pose gradient too; poses that
        do not are detached copies, as before.  No host synchronisation."""
        depth, normal, rgb, _ = self._cast(intrinsics, poses, height, width, stride, step, near, far, min_weight)
        if rgb is None:
            rgb = torch.zeros(tuple(depth.shape) + (3,), dtype=torch.float32, device=depth.device)
        K = intrinsics.detach().to(torch.float32).reshape(self._B, 1, 4, 4).clone()
        K[..., 0, 0] /= stride
        K[..., 1, 1] /= stride
        K[..., 0, 2] /= stride
        K[..., 1, 2] /= stride
        attached = torch.is_grad_enabled() and poses.requires_grad
        frames = RGBDImages(rgb, depth.unsqueeze(-1), K, (poses if attached else poses.detach()).to(torch.float32))
        return (frames, normal) if return_normals else frames

    def raycast_pointcloud(self, intrinsics, poses, height: int, width: int, *, stride: int = 1, step: Optional[float] = None,
                           near: float = 0.0, far: Optional[float] = None, min_weight: float = 1.0) -> Pointclouds:
        r"""The hit pixels of `raycast` from ONE camera per batch element (poses (B, 1, 4, 4)) as a Pointclouds, in pixel order:
        global points (the global vertex map of the cast image), normals and, for a volume with colours, colours.
        Differentiable w.r.t. tsdf and color, through the depth, and w.r.t. poses that require a gradient, through the depth
        and through the vertex map.  One host synchronisation (the sizes)."""
        if torch.is_tensor(poses) and poses.ndim == 4 and poses.shape[1] != 1:
            raise ValueError("TSDFVolume.raycast_pointcloud: one camera per batch element (L = 1). Got poses {}.".format(tuple(poses.shape)))
        frames, normal = self.raycast(intrinsics, poses, height, width, stride=stride, step=step, near=near, far=far,
                                      min_weight=min_weight, return_normals=True)
        B = self._B
        mask = (frames.depth_image > 0).reshape(-1)  # the hits: z* > 0
        xs = [frames.global_vertex_map.reshape(-1, 3), normal.reshape(-1, 3)] + ([frames.rgb_image.reshape(-1, 3)] if self.has_colors else [])
        counts = mask.view(B, -1).sum(1)
        n = counts.tolist()  # the one host synchronisation
        if torch.is_grad_enabled() and any(x.requires_grad for x in xs):
            rows = ops.mask_select_multi(xs, mask, n=sum(n))
        else:
            rows, _ = ops.compact_multi_raw(xs, mask)
        at = [sum(n[:b]) for b in range(B + 1)]
        split = lambda x: [x[at[b]: at[b + 1]] for b in range(B)]
        return Pointclouds(points=split(rows[0]), normals=split(rows[1]), colors=split(rows[2]) if self.has_colors else None)
