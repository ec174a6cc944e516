"""The arena-backed sequence drivers: the map storage (`_MapArena`), the one frame loop over it (`run_frames`, which
`ICPSLAM._forward_streamed` hands the plain C calls) and the differentiable sequence as one autograd node, which hands it
their taped forms (`_PointFusionSeqFn`).  Every C call goes through `ops`."""
import os

import torch

from .. import ops
from ..structures.pointclouds import Pointclouds

_NO_READBACK = bool(os.environ.get("GS_NO_READBACK"))  # measurements only: never tighten the host's bound of the map size


class _MapArena:
    """Device-resident map storage for the streamed sequence driver: capacity-doubling
    (B, cap, C) arrays, per-sequence point counts that live on the device, O(1) append.  The host only tracks an
    upper bound of the counts; it is tightened by asynchronous read-backs (pinned memory + events) that never
    stall the frame loop."""

    def __init__(self, B: int, hw: int, device, with_features: bool = True):
        self.B, self.hw, self.device = B, hw, device
        self.cap = 1 << max(2 * hw - 1, 1).bit_length()
        mk = lambda c: torch.zeros((B, self.cap, c), dtype=torch.float32, device=device)
        self.points, self.normals, self.colors = mk(3), mk(3), mk(3)
        self.ccounts = mk(1) if with_features else None
        self.counts = torch.zeros(B, dtype=torch.int32, device=device)
        self.upper = 0          # host-side upper bound of max_b counts[b]
        self.appends = 0        # frames appended so far
        self._pinned = [torch.empty(B, dtype=torch.int32).pin_memory() for _ in range(4)]
        self._pending = []      # (appends at issue time, pinned buffer, event)

    @classmethod
    def for_one_step(cls, pointclouds: Pointclouds, B: int, hw: int, device, with_features: bool):
        """Arena holding a copy of `pointclouds` with room for exactly one more frame (the step-by-step API)."""
        self = cls.__new__(cls)
        self.B, self.hw, self.device = B, hw, device
        n_old = max(pointclouds._counts) if pointclouds.has_points else 0
        self.cap = n_old + hw
        mk = lambda c: torch.zeros((B, self.cap, c), dtype=torch.float32, device=device)
        self.points, self.normals, self.colors = mk(3), mk(3), mk(3)
        self.ccounts = mk(1) if with_features else None
        if pointclouds.has_points:
            self.points[:, :n_old] = pointclouds.points_padded
            self.normals[:, :n_old] = pointclouds.normals_padded
            self.colors[:, :n_old] = pointclouds.colors_padded
            if with_features:
                self.ccounts[:, :n_old] = pointclouds.features_padded
            self.counts = pointclouds._counts_i32().clone()
        else:
            self.counts = torch.zeros(B, dtype=torch.int32, device=device)
        self.upper, self.appends, self._pinned, self._pending = n_old, 0, [], []
        return self

    # The host may run at most this many frames ahead of the map counts it knows.  The row bound it hands to the kernels
    # and the capacity it reserves are `last known count + frames since x H W`: a host that enqueues four times faster than
    # the GPU executes (0.13 against 0.4-0.6 ms per frame on the round-3 boxes) would otherwise be ~150 frames ahead by
    # the end of a 200-frame sequence, none of its read-backs would have landed when it needs them, and the arena would be
    # grown -- allocated, zero-filled, copied -- as if every frame had appended H W points (46 M rows instead of 3.3 M:
    # the 200-frame forward ran at 1 600 frames/s where the same kernels with exact bounds run at 2 650, and FASTER under
    # rocprofv3, whose per-launch host cost happens to keep the host near the GPU: tools/gap_bisect.py).  Two frames of
    # queued work (~1 ms) keep the GPU fed on any host.
    MAX_FRAMES_AHEAD = 2

    def _tighten(self):
        while self._pending and (self._pending[0][2].query() or self.appends - self._pending[0][0] >= self.MAX_FRAMES_AHEAD):
            at, buf, ev = self._pending.pop(0)
            ev.synchronize()  # (returns at once when the query above succeeded)
            self._pinned.append(buf)
            self.upper = min(self.upper, int(buf.max()) + (self.appends - at) * self.hw)

    def reserve_frame(self) -> int:
        """Make room for one more frame's worth of rows; returns the row bound to hand to the kernels."""
        self._tighten()
        need = self.upper + self.hw
        if need > self.cap:
            # one sequence: power-of-two capacities keep the workspace ADDRESS (and with it the captured graph) for many
            # frames, and the kernels get `need`, not the capacity, as row bound.  Several sequences share the row
            # stride = capacity, which the kernels then scan: grow by 1.5x in 64 Ki-row steps instead, so that the
            # padding they read stays below half of the data
            new_cap = 1 << (need - 1).bit_length() if self.B == 1 else -(-max(need, self.cap + self.cap // 2) // 65536) * 65536
            for name in ("points", "normals", "colors", "ccounts"):
                old = getattr(self, name)
                if old is None:
                    continue
                new = torch.zeros((self.B, new_cap, old.shape[2]), dtype=torch.float32, device=self.device)
                new[:, : self.cap] = old
                setattr(self, name, new)
            self.cap = new_cap
        # one sequence: any row bound works as the "padded length" (rows beyond the count are zero); several
        # sequences share the row stride, which is the capacity
        return need if self.B == 1 else self.cap

    def rows(self, bound: int):
        """(points, normals, colors, ccounts) views of `bound` rows per sequence (contiguous)."""
        if bound == self.cap:
            return self.points, self.normals, self.colors, self.ccounts
        cut = lambda x: None if x is None else x[:, :bound]
        return cut(self.points), cut(self.normals), cut(self.colors), cut(self.ccounts)

    def appended(self):
        self.upper += self.hw
        self.appends += 1
        if self._pinned and not _NO_READBACK:
            buf = self._pinned.pop()
            buf.copy_(self.counts, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending.append((self.appends, buf, ev))

    def to_pointclouds(self) -> Pointclouds:
        n = self.counts.tolist()  # the one host synchronisation of a streamed sequence
        pick = lambda x: [x[b, : n[b]].clone() for b in range(self.B)]
        return Pointclouds(points=pick(self.points), normals=pick(self.normals), colors=pick(self.colors),
                           features=pick(self.ccounts) if self.ccounts is not None else None)


def run_frames(arena: _MapArena, rgb, depth, K, gt_poses, localize, update):
    """The frame loop over an arena: two actions per frame, no host synchronisation.  rgb (B,L,H,W,3), depth (B,L,H,W,1);
    gt_poses (B,L,4,4) or None (identity start).
      localize(depth_s, prev_pose, bound, out) -> pose (B,1,4,4) of a frame after the first against `arena.rows(bound)`; `out`
          is the frame's slice of the result where the pose can be written straight into it (one sequence), else None.
          localize = None: every frame takes its ground-truth pose.
      update(arena, depth_s, rgb_s, K, pose, bound, stats_row): the map update on `arena.rows(bound)`.
    -> (recovered poses (B,L,4,4), stats (L,4+B) int32)."""
    B, L = depth.shape[:2]
    dev = depth.device
    recovered = torch.empty((B, L, 4, 4), dtype=torch.float32, device=dev)
    stats = torch.zeros((L, 4 + B), dtype=torch.int32, device=dev)
    prev, bound = None, None
    for s in range(L):  # true serial dependence: pose s needs map s-1
        d_s, c_s = depth[:, s].contiguous(), rgb[:, s].contiguous()  # (B,H,W,C); views (no copy) for one contiguous sequence
        if s == 0 or localize is None:
            pose = (gt_poses[:, s:s + 1] if gt_poses is not None else
                    torch.eye(4, dtype=torch.float32, device=dev).view(1, 1, 4, 4).repeat(B, 1, 1, 1))
        else:
            # (one sequence: the pose can go straight into its row of the result -- a copy launch less per frame)
            pose = localize(d_s, prev, bound, recovered[:, s:s + 1] if B == 1 else None)
        bound = arena.reserve_frame()
        update(arena, d_s, c_s, K, pose, bound, stats[s])
        arena.appended()
        if pose.data_ptr() != recovered[:, s:s + 1].data_ptr():
            recovered[:, s] = pose[:, 0]
        prev = pose
    return recovered, stats


class _PointFusionSeqFn(torch.autograd.Function):
    """PointFusion over a whole batch of sequences as ONE autograd node: (rgb, depth, K, poses, localize_args = the tail of
    ops.slam_localize_* or None for ground-truth poses, update_args = (dist_th, dot_th, sigma)) -> (points, normals, colors,
    ccounts (B,N,C) each, recovered poses (B,L,4,4), stats).

    forward  = the arena-backed frame loop with the taped forms of its two calls per frame
               (gs_slam_localize_taped, gs_pointfusion_update_taped): no host synchronisation until the map is
               handed back, the map updated in place.
    backward = the frames in reverse on a copy of the final arena: per frame gs_pointfusion_update_backward (pulls the
               running adjoint of the whole map back through merge + append at the matched / appended rows only and
               restores the arena to the previous frame's), the adjoint of the frame's vertex / normal maps, then
               gs_slam_localize_backward (adds the ICP targets' adjoints into the running map adjoint) and the adjoint of
               the live maps under the previous pose.  What is a constant in the reference's graph is a constant here
               (correspondence tables, association indices, accept decisions).
    reference: torch autograd through slam/icpslam.py:125-137 with slam/pointfusion.py:107-112."""

    @staticmethod
    def forward(ctx, rgb, depth, K, poses, localize_args, update_args):
        c32 = lambda x: x.detach().float().contiguous()
        rgb, depth, K = c32(rgb), c32(depth), c32(K)
        B, L, H, W = depth.shape[:4]
        arena = _MapArena(B, H * W, depth.device, with_features=True)
        loc_tapes, fuse_tapes = [], []  # (tape, row bound) of the frames after the first (if they localise) / of every frame

        def localize(d_s, prev, bound, out):
            mp, mn, _, _ = arena.rows(bound)
            d_s = d_s.unsqueeze(1)
            _, _, gV, _ = ops.vertex_normal_maps_raw(d_s, K, prev, want_local=False, want_global=True)
            pose, tape = ops.slam_localize_taped_raw(gV, d_s, K, prev, mp, mn, arena.counts, *localize_args)
            loc_tapes.append((tape, bound))
            return pose

        def update(arena, d_s, c_s, K, pose, bound, stats_row):
            tape = ops.pointfusion_update_taped_raw(d_s, c_s, K, pose, *arena.rows(bound), arena.counts, *update_args, stats_row)
            fuse_tapes.append((tape, bound))

        recovered, stats = run_frames(arena, rgb, depth, K, c32(poses) if poses is not None else None,
                                      localize if localize_args is not None else None, update)
        n = arena.counts.tolist()  # the one host synchronisation of the sequence
        ctx.arena, ctx.loc_tapes, ctx.fuse_tapes, ctx.n_final = arena, loc_tapes, fuse_tapes, n
        ctx.localize_args, ctx.sigma = localize_args, update_args[2]
        ctx.has_poses = poses is not None
        ctx.save_for_backward(rgb, depth, K, recovered)
        cut = lambda x: x[:, : max(n)].clone()  # zero-padded to the largest map (rows beyond a sequence's count are zero)
        ctx.mark_non_differentiable(stats)
        return cut(arena.points), cut(arena.normals), cut(arena.colors), cut(arena.ccounts), recovered.clone(), stats

    @staticmethod
    def backward(ctx, g_p, g_n, g_c, g_f, g_poses, _g_stats):
        rgb, depth, K, recovered = ctx.saved_tensors
        arena, n_final = ctx.arena, ctx.n_final
        B, L, H, W = depth.shape[:4]
        dev = depth.device
        cap = arena.cap
        # work on copies: the arena is restored frame by frame, the running adjoint of the map is pulled back in place
        mp, mn, mc, mf = (x.clone() for x in (arena.points, arena.normals, arena.colors, arena.ccounts))
        counts = arena.counts.clone()

        def running(g, c):
            G = torch.zeros((B, cap, c), dtype=torch.float32, device=dev)
            if g is not None:
                for b in range(B):  # (rows beyond a sequence's count are padding of the output, not map points)
                    G[b, :n_final[b]] = g[b, :n_final[b]]
            return G

        Gp, Gn, Gc, Gf = running(g_p, 3), running(g_n, 3), running(g_c, 3), running(g_f, 1)
        gpose = g_poses.clone().float() if g_poses is not None else torch.zeros((B, L, 4, 4), dtype=torch.float32, device=dev)
        g_rgb, g_depth, g_K = torch.zeros_like(rgb), torch.zeros_like(depth), torch.zeros_like(K)
        g_poses_in = torch.zeros((B, L, 4, 4), dtype=torch.float32, device=dev) if ctx.has_poses else None
        mk = lambda c: torch.empty((B, H, W, c), dtype=torch.float32, device=dev)
        g_V, g_gV, g_gN = mk(3), mk(3), mk(3)
        g_live = torch.empty((B, 1, H, W, 3), dtype=torch.float32, device=dev)
        g_prev = torch.empty((B, 1, 4, 4), dtype=torch.float32, device=dev)
        # One sequence (B = 1): the per-frame slices of the adjoints are contiguous, so every kernel writes or ADDS straight
        # into them -- no per-frame temporaries, zero fills or `+=` launches (a dozen small torch kernels per frame, and
        # their host cost, in the first version of this loop).  A batch takes contiguous per-frame buffers and copies.
        one = B == 1
        if not one:
            t_rgb, t_depth, t_pose, t_pose2 = mk(3), torch.empty((B, 1, H, W, 1), dtype=torch.float32, device=dev), \
                torch.empty((B, 1, 4, 4), dtype=torch.float32, device=dev), torch.empty((B, 1, 4, 4), dtype=torch.float32, device=dev)
        stride = cap

        def restride(n):
            # A batch's arrays are (B, stride, C) and the kernels take ONE number for row bound and row stride.  The arena
            # may have grown during the forward pass; the tapes of earlier frames were laid out with the stride of their
            # time.  Walking back, the map only shrinks: repack the working arrays to the older, smaller stride once per
            # growth step (rows beyond it did not exist yet; their adjoints have been consumed by their own frames).
            nonlocal mp, mn, mc, mf, Gp, Gn, Gc, Gf, stride
            if one or n == stride:
                return
            mp, mn, mc, mf, Gp, Gn, Gc, Gf = (x[:, :n].contiguous() for x in (mp, mn, mc, mf, Gp, Gn, Gc, Gf))
            stride = n

        for s in reversed(range(L)):
            d_s, c_s = depth[:, s].contiguous(), rgb[:, s].contiguous()
            pose_s = recovered[:, s:s + 1].contiguous()
            ftape, bound = ctx.fuse_tapes[s]
            restride(bound)
            ops.pointfusion_update_backward_raw(d_s, c_s, K, pose_s, mp, mn, mc, mf, counts, bound, ctx.sigma, ftape, Gp, Gn, Gc, Gf,
                                                g_V, g_gV, g_gN, g_rgb[:, s] if one else t_rgb)
            if one:
                gd_s, gpose_s = g_depth[:, s], gpose[:, s]
            else:
                g_rgb[:, s] = t_rgb
                gd_s, gpose_s = t_depth.zero_(), t_pose.zero_()
            ops.vertex_normal_maps_backward_into(d_s.unsqueeze(1), K, pose_s, g_V.unsqueeze(1), None, g_gV.unsqueeze(1),
                                                 g_gN.unsqueeze(1), gd_s, g_K, gpose_s)
            if not one:
                gpose[:, s] += t_pose[:, 0]
            if s > 0 and ctx.localize_args is not None:
                tape, nmax = ctx.loc_tapes[s - 1]
                restride(nmax)
                prev = recovered[:, s - 1:s].contiguous()
                ds, numiters, _, dist_thresh, grad_params = ctx.localize_args
                ops.slam_localize_backward_raw(prev, mp, mn, nmax, H, W, ds, numiters, dist_thresh, grad_params, tape,
                                               gpose[:, s:s + 1], g_live, Gp, Gn, g_prev, 1)
                gprev_s = gpose[:, s - 1] if one else t_pose2.zero_()
                ops.vertex_normal_maps_backward_into(d_s.unsqueeze(1), K, prev, None, None, g_live, None, gd_s, g_K, gprev_s)
                if not one:
                    gpose[:, s - 1] += t_pose2[:, 0]
                gpose[:, s - 1] += g_prev.view(B, 4, 4)
            elif g_poses_in is not None:
                g_poses_in[:, s] += gpose[:, s]
            if not one:
                g_depth[:, s] += t_depth[:, 0]
        return g_rgb, g_depth, g_K, g_poses_in, None, None
