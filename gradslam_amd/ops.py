"""Tensor-level front of the C ABI: one Python function per kernel family, plus the
`torch.autograd.Function`s that keep the reference's gradients flowing through them.

Nothing here computes on the CPU.  Tensors must live on a HIP device (`require_hip`).
Shapes follow the reference: images channels-last (B,L,H,W,C), clouds padded (B,N,C), tables
(P,4) int64 rows [b,n,h,w].
"""
import math
from typing import Optional, Tuple

import torch

from . import _native as nv
from ._native import call, ptr, require_hip, stream, workspace, ws_bytes


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def deterministic() -> bool:
    """torch's switch for reproducible training: under torch.use_deterministic_algorithms(True) every backward below calls the
    `_det` entry of its kernel (no float atomics: the same gradient bits from run to run), otherwise the default one."""
    return torch.are_deterministic_algorithms_enabled()


def dev_int(value: int, device) -> torch.Tensor:
    """A device-resident int32 scalar (filled by a kernel: no host->device copy, no sync)."""
    return torch.full((1,), int(value), dtype=torch.int32, device=device)


# ---------------------------------------------------------------------------------------------- V
def vertex_normal_maps_raw(depth, K, poses, want_local=True, want_global=True):
    """depth (B,L,H,W,1), K (B,1,4,4), poses (B,L,4,4) or None -> (V, N, gV, gN); entries not
    requested are None.  One fused launch (reference structures/rgbdimages.py:643-762)."""
    require_hip(depth, K, poses, op="vertex_normal_maps")
    depth, K, poses = _f32c(depth), _f32c(K), _f32c(poses)
    B, L, H, W = depth.shape[:4]
    mk = lambda: torch.empty((B, L, H, W, 3), dtype=torch.float32, device=depth.device)
    V = mk() if want_local else None
    N = mk() if want_local else None
    gV = mk() if want_global else None
    gN = mk() if want_global else None
    call("gs_vertex_normal_maps", ptr(depth), ptr(K), ptr(poses), B, L, H, W, ptr(V), ptr(N), ptr(gV), ptr(gN), stream())
    return V, N, gV, gN


class _MapsFn(torch.autograd.Function):
    """(depth, K, poses) -> (V, N, gV, gN) with the hand-written adjoint."""

    @staticmethod
    def forward(ctx, depth, K, poses, want_local, want_global):
        V, N, gV, gN = vertex_normal_maps_raw(depth, K, poses, want_local, want_global)
        ctx.save_for_backward(depth, K, poses)
        ctx.has_poses = poses is not None
        dummy = depth.new_empty(0)
        outs = tuple(x if x is not None else dummy for x in (V, N, gV, gN))
        ctx.mark_non_differentiable(*[o for o, x in zip(outs, (V, N, gV, gN)) if x is None])
        return outs

    @staticmethod
    def backward(ctx, gV_l, gN_l, gV_g, gN_g):
        depth, K, poses = ctx.saved_tensors
        fix = lambda g: None if (g is None or g.numel() == 0) else g
        g_depth, g_K, g_P = vertex_normal_maps_backward_raw(depth, K, poses, fix(gV_l), fix(gN_l), fix(gV_g), fix(gN_g))
        return g_depth.view_as(depth), g_K.view_as(K), (g_P.view_as(poses) if g_P is not None else None), None, None


def vertex_normal_maps_backward_raw(depth, K, poses, gV_l=None, gN_l=None, gV_g=None, gN_g=None):
    """Adjoint of vertex_normal_maps_raw: given the adjoints of any of the four maps (None = zero) returns
    (g_depth, g_K, g_poses or None), freshly allocated and fully written."""
    depth_c, K_c, poses_c = _f32c(depth), _f32c(K), _f32c(poses)
    B, L, H, W = depth_c.shape[:4]
    gV_l, gN_l, gV_g, gN_g = _f32c(gV_l), _f32c(gN_l), _f32c(gV_g), _f32c(gN_g)
    g_depth = torch.zeros_like(depth_c)
    g_K = torch.zeros_like(K_c)
    g_P = torch.zeros_like(poses_c) if poses_c is not None else None
    _maps_backward(depth_c, K_c, poses_c, B, L, H, W, gV_l, gN_l, gV_g, gN_g, g_depth, g_K, g_P)
    return g_depth, g_K, g_P


def _maps_backward(depth_c, K_c, poses_c, B, L, H, W, gV_l, gN_l, gV_g, gN_g, g_depth, g_K, g_P):
    det = "_det" if deterministic() else ""
    ws = workspace(ws_bytes("gs_vertex_normal_maps_backward{}_ws_bytes".format(det), B, L, H, W), depth_c.device, "maps_bwd" + det)
    call("gs_vertex_normal_maps_backward" + det, ptr(depth_c), ptr(K_c), ptr(poses_c), B, L, H, W, ptr(gV_l), ptr(gN_l),
         ptr(gV_g), ptr(gN_g), ptr(g_depth), ptr(g_K), ptr(g_P), ptr(ws), ws.numel(), stream())


def vertex_normal_maps_backward_into(depth, K, poses, gV_l, gN_l, gV_g, gN_g, g_depth, g_K, g_poses):
    """vertex_normal_maps_backward_raw that ADDS into caller-held adjoints (contiguous float32, same shapes as depth / K /
    poses; the C kernels accumulate into all three): what a reverse pass over many frames wants -- no temporaries, no
    zero fills, no `+=` launches per frame."""
    depth_c, K_c, poses_c = _f32c(depth), _f32c(K), _f32c(poses)
    B, L, H, W = depth_c.shape[:4]
    for x in (g_depth, g_K, g_poses):
        if x is not None and not (x.is_contiguous() and x.dtype == torch.float32):
            raise ValueError("vertex_normal_maps_backward_into: the adjoint buffers must be contiguous float32")
    gV_l, gN_l, gV_g, gN_g = _f32c(gV_l), _f32c(gN_l), _f32c(gV_g), _f32c(gN_g)
    _maps_backward(depth_c, K_c, poses_c, B, L, H, W, gV_l, gN_l, gV_g, gN_g, g_depth, g_K, g_poses)


def vertex_normal_maps(depth, K, poses, want_local=True, want_global=True):
    """Autograd-aware entry: returns (V, N, gV, gN) (None where not requested)."""
    needs_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (depth, K, poses))
    if not needs_grad:
        return vertex_normal_maps_raw(depth, K, poses, want_local, want_global)
    outs = _MapsFn.apply(depth, K, poses, want_local, want_global)
    sel = (want_local, want_local, want_global, want_global)
    return tuple(o if s else None for o, s in zip(outs, sel))


# ---------------------------------------------------------------------------------------------- alpha
class _AlphaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, sigma, eps):
        p = _f32c(pts)
        out = torch.empty(p.shape[:-1], dtype=torch.float32, device=p.device)
        call("gs_get_alpha", ptr(p), p.numel() // 3, float(sigma), float(eps), ptr(out), stream())
        ctx.save_for_backward(p)
        ctx.sigma, ctx.eps = float(sigma), float(eps)
        return out

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        gp = torch.zeros_like(p)
        call("gs_get_alpha_backward", ptr(p), p.numel() // 3, ctx.sigma, ctx.eps, ptr(_f32c(g)), ptr(gp), stream())
        return gp, None, None


def get_alpha_lastdim(points: torch.Tensor, sigma: float, eps: float) -> torch.Tensor:
    """points (..., 3) -> alpha (...)  (reference slam/fusionutils.py:69-73)."""
    require_hip(points, op="get_alpha")
    return _AlphaFn.apply(points, sigma, eps)


# ---------------------------------------------------------------------------------------------- compaction
def compact_rows(src: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """src (n, C) float32 or (n, C) int64, mask (n,) bool/uint8 -> src[mask], order preserved.
    One host sync to learn the output length."""
    require_hip(src, mask, op="compact_rows")
    n = src.shape[0]
    src = src.contiguous()
    m8 = mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()
    words = (src.element_size() * (src.numel() // max(n, 1))) // 4 if n else 0
    out = torch.empty_like(src)
    cnt = torch.zeros(1, dtype=torch.int32, device=src.device)
    ws = workspace(ws_bytes("gs_compact_ws_bytes", n), src.device, "compact")
    call("gs_compact_rows", ptr(src), ptr(m8), n, words, ptr(out), ptr(cnt), ptr(ws), ws.numel(), stream())
    return out[: int(cnt.item())]


def compact_multi_raw(srcs, mask):
    """srcs: list of <=4 (n, C_a) float32 tensors sharing `mask` (n,) uint8/bool -> (list of (n, C_a)
    output buffers, count (1,) int32 device).  No sync; rows beyond count are garbage."""
    import ctypes

    require_hip(mask, *srcs, op="compact_multi")
    n = mask.shape[0]
    srcs = [_f32c(s) for s in srcs]
    m8 = mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()
    outs = [torch.empty_like(s) for s in srcs]
    k = len(srcs)
    a_src = (ctypes.c_void_p * k)(*[s.data_ptr() for s in srcs])
    a_out = (ctypes.c_void_p * k)(*[o.data_ptr() for o in outs])
    a_w = (ctypes.c_int * k)(*[s.numel() // max(n, 1) for s in srcs])
    cnt = torch.zeros(1, dtype=torch.int32, device=mask.device)
    ws = workspace(ws_bytes("gs_compact_ws_bytes", n), mask.device, "compact")
    call("gs_compact_multi", k, a_src, a_w, a_out, ptr(m8), n, ptr(cnt), ptr(ws), ws.numel(), stream())
    return outs, cnt


class _MaskSelectFn(torch.autograd.Function):
    """x[mask] on (n, C) rows with a scatter adjoint (the reference's boolean-mask indexing)."""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        ctx.shape = x.shape
        return compact_rows(x, mask)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        out = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device)
        out[mask.bool() if mask.dtype != torch.bool else mask] = g  # adjoint of a gather with unique targets
        return out, None


class _MultiMaskSelectFn(torch.autograd.Function):
    """[x[mask] for x in xs] for up to 4 (n, C_a) arrays sharing one mask: one compaction (one scan, one host
    sync for the length) forward, one expansion kernel backward."""

    @staticmethod
    def forward(ctx, mask, n, *xs):
        outs, cnt = compact_multi_raw(list(xs), mask)
        n = int(cnt.item()) if n is None else n
        ctx.save_for_backward(mask)
        ctx.shapes = [x.shape for x in xs]
        return tuple(o[:n] for o in outs)

    @staticmethod
    def backward(ctx, *gs):
        import ctypes

        (mask,) = ctx.saved_tensors
        n = mask.shape[0]
        gs = [_f32c(g) for g in gs]
        dev = mask.device
        outs = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in ctx.shapes]
        if n == 0:
            return (None, None, *outs)
        m8 = mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()
        k = len(gs)
        # an empty selection leaves nothing to read: give the kernel a valid (unused) pointer
        a_g = (ctypes.c_void_p * k)(*[(g if g.numel() else o).data_ptr() for g, o in zip(gs, outs)])
        a_out = (ctypes.c_void_p * k)(*[o.data_ptr() for o in outs])
        a_w = (ctypes.c_int * k)(*[o.numel() // n for o in outs])
        ws = workspace(ws_bytes("gs_compact_ws_bytes", n), dev, "compact")
        call("gs_expand_multi", k, a_g, a_w, a_out, ptr(m8), n, ptr(ws), ws.numel(), stream())
        return (None, None, *outs)


def mask_select_multi(xs, mask: torch.Tensor, n: Optional[int] = None):
    """[x[mask] for x in xs] (<= 4 arrays, (n, C_a) float32 each), differentiable, one scan and one sync -- none when the caller
    already knows n = mask.sum()."""
    return list(_MultiMaskSelectFn.apply(mask, n, *xs))


def select_rows_multi(xs, mask: torch.Tensor):
    """[x[mask] for x in xs] with or without autograd: one compaction, one host sync either way."""
    if torch.is_grad_enabled() and any(x.requires_grad for x in xs):
        return mask_select_multi(xs, mask)
    outs, cnt = compact_multi_raw(list(xs), mask)
    n = int(cnt.item())
    return [o[:n] for o in outs]


def mask_select(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    if torch.is_grad_enabled() and x.requires_grad:
        return _MaskSelectFn.apply(x, mask)
    return compact_rows(x, mask)


def frames_from_raw(depth_u16, rgb_u8, height: int, width: int, depth_scale: float, normalize_color: bool):
    """Raw sensor frames on the device -> float32 (depth (B,H,W,1), rgb (B,H,W,3)); either input may be None.
    depth_u16 (B,Hs,Ws) int16/uint16 storage, rgb_u8 (B,Hs,Ws,3) uint8 (reference datasets/tum.py:455-499)."""
    ref = depth_u16 if depth_u16 is not None else rgb_u8
    require_hip(*(x for x in (depth_u16, rgb_u8) if x is not None), op="frames_from_raw")
    B, Hs, Ws = ref.shape[:3]
    dev = ref.device
    if depth_u16 is not None and not (depth_u16.is_contiguous() and depth_u16.element_size() == 2):
        raise ValueError("frames_from_raw: depth must be a contiguous 16-bit integer tensor")
    if rgb_u8 is not None and not (rgb_u8.is_contiguous() and rgb_u8.dtype == torch.uint8 and rgb_u8.shape[-1] == 3):
        raise ValueError("frames_from_raw: rgb must be a contiguous uint8 (B,H,W,3) tensor")
    depth = torch.empty((B, height, width, 1), dtype=torch.float32, device=dev) if depth_u16 is not None else None
    rgb = torch.empty((B, height, width, 3), dtype=torch.float32, device=dev) if rgb_u8 is not None else None
    call("gs_frames_from_raw", ptr(depth_u16), ptr(rgb_u8), B, Hs, Ws, int(height), int(width), float(depth_scale),
         1 if normalize_color else 0, ptr(depth), ptr(rgb), stream())
    return depth, rgb


# ---------------------------------------------------------------------------------------------- D
def downsample_frame_raw(depth, gV, gN, rgb, ds: int):
    """One-frame maps (B,1,H,W,C) -> padded (B,cap,3) x3 + counts (B,) int32 device
    (reference odometry/icputils.py:651-669)."""
    require_hip(depth, gV, gN, rgb, op="downsample_frame")
    depth, gV, gN, rgb = _f32c(depth), _f32c(gV), _f32c(gN), _f32c(rgb)
    B, _, H, W = depth.shape[:4]
    cap = ((H + ds - 1) // ds) * ((W + ds - 1) // ds)
    dev = depth.device
    mk = lambda src: None if src is None else torch.zeros((B, cap, 3), dtype=torch.float32, device=dev)
    op, on, oc = mk(gV), mk(gN), mk(rgb)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = workspace(ws_bytes("gs_downsample_frame_ws_bytes", H, W, ds), dev, "compact")
    call("gs_downsample_frame", ptr(depth), ptr(gV), ptr(gN), ptr(rgb), B, H, W, ds, cap, ptr(op), ptr(on), ptr(oc),
         None, ptr(counts), ptr(ws), ws.numel(), stream())
    return op, on, oc, counts


# ---------------------------------------------------------------------------------------------- P / S
def project_active_raw(points_padded, counts_dev, poses_b44, K_b44, H: int, W: int, ds: int = 0):
    """-> (rows buffer (B*Nmax,4) int64, count (1,) int32 device).  Rows beyond count are garbage.
    reference slam/fusionutils.py:247-282 (+ odometry/icputils.py:596-597 when ds > 0)."""
    require_hip(points_padded, counts_dev, poses_b44, K_b44, op="project_active")
    pts, poses, K = _f32c(points_padded), _f32c(poses_b44), _f32c(K_b44)
    B, Nmax = pts.shape[:2]
    dev = pts.device
    rows = torch.empty((B * Nmax, 4), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = workspace(ws_bytes("gs_project_active_ws_bytes", B, Nmax), dev, "project")
    call("gs_project_active", ptr(pts), ptr(counts_dev), B, Nmax, ptr(poses), ptr(K), H, W, ds, ptr(rows), ptr(cnt),
         ptr(ws), ws.numel(), stream())
    return rows, cnt


def gather_table_rows_raw(rows, n_rows_dev, max_rows: int, attr_padded, cap: int):
    """Per-batch gather of attr[b, n] for table rows (sorted by b) -> padded (B,cap,C), counts (B,)."""
    require_hip(rows, attr_padded, op="gather_table_rows")
    attr = _f32c(attr_padded)
    B, Nmax, C = attr.shape
    dev = attr.device
    out = torch.zeros((B, max(cap, 1), C), dtype=torch.float32, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = workspace(ws_bytes("gs_gather_table_rows_ws_bytes", B), dev, "gather")
    call("gs_gather_table_rows", ptr(rows), ptr(n_rows_dev), max_rows, ptr(attr), B, Nmax, C, cap, ptr(out), ptr(counts),
         ptr(ws), ws.numel(), stream())
    return out, counts


def table_ds_mask(rows: torch.Tensor, ds: int) -> torch.Tensor:
    require_hip(rows, op="table_ds_mask")
    rows = rows.contiguous()
    mask = torch.zeros(rows.shape[0], dtype=torch.uint8, device=rows.device)
    call("gs_table_ds_mask", ptr(rows), rows.shape[0], ds, ptr(mask), stream())
    return mask


# ---------------------------------------------------------------------------------------------- K / J
def knn1_raw(src, tgt, ns_dev=None, nt_dev=None, brute_force: bool = False) -> torch.Tensor:
    """src (Ns,3), tgt (Nt,3) -> packed best (Ns,) int64 = dist_bits << 32 | idx.  The default kernel
    prunes target chunks with an exact AABB bound; brute_force=True evaluates every pair (verifier)."""
    require_hip(src, tgt, op="knn1")
    src, tgt = _f32c(src), _f32c(tgt)
    dev = src.device
    ns_dev = dev_int(src.shape[0], dev) if ns_dev is None else ns_dev
    nt_dev = dev_int(tgt.shape[0], dev) if nt_dev is None else nt_dev
    best = torch.empty(src.shape[0], dtype=torch.int64, device=dev)
    if brute_force:
        call("gs_knn1_bruteforce", ptr(src), ptr(ns_dev), src.shape[0], ptr(tgt), ptr(nt_dev), tgt.shape[0], ptr(best), stream())
    else:
        ws = workspace(ws_bytes("gs_knn1_ws_bytes", tgt.shape[0]), dev, "knn")
        call("gs_knn1", ptr(src), ptr(ns_dev), src.shape[0], ptr(tgt), ptr(nt_dev), tgt.shape[0], ptr(best), ptr(ws),
             ws.numel(), stream())
    return best


def knn1_unpack(best: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    dev = best.device
    n = best.shape[0]
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    call("gs_knn1_unpack", ptr(best), ptr(dev_int(n, dev)), n, ptr(d2), ptr(idx), stream())
    return d2, idx


def knn_points(src: torch.Tensor, tgt: torch.Tensor):
    """Drop-in for the call `knn_points(src (1,Ns,3), tgt (1,Nt,3))` of reference
    odometry/icputils.py:200-201: returns (dists (1,Ns,1) squared L2, idx (1,Ns,1) int64)."""
    d2, idx = knn1_unpack(knn1_raw(src[0].detach(), tgt[0].detach()))
    return d2.view(1, -1, 1), idx.view(1, -1, 1)


def _thresh(dist_thresh) -> float:
    # negative == None at the C ABI; a user-supplied negative threshold keeps nothing, like 0.0
    return -1.0 if dist_thresh is None else max(float(dist_thresh), 0.0)


def icp_linearize_raw(src, tgt, nrm, best, dist_thresh) -> torch.Tensor:
    """-> 44 floats: H (36) | g (6) | e | count."""
    src, tgt, nrm = _f32c(src), _f32c(tgt), _f32c(nrm)
    dev = src.device
    out = torch.empty(44, dtype=torch.float32, device=dev)
    ws = workspace(ws_bytes("gs_icp_linearize_ws_bytes", src.shape[0]), dev, "linearize")
    call("gs_icp_linearize", ptr(src), ptr(dev_int(src.shape[0], dev)), src.shape[0], ptr(tgt), ptr(nrm), ptr(best),
         _thresh(dist_thresh), ptr(out), ptr(ws), ws.numel(), stream())
    return out


class _LinearizeFn(torch.autograd.Function):
    """(src, tgt, nrm | best) -> (H (6,6), g (6,1), e ()) with the scatter adjoint of A.5."""

    @staticmethod
    def forward(ctx, src, tgt, nrm, best, dist_thresh):
        out = icp_linearize_raw(src, tgt, nrm, best, dist_thresh)
        ctx.save_for_backward(src, tgt, nrm, best)
        ctx.dist_thresh = dist_thresh
        return out[:36].view(6, 6).clone(), out[36:42].view(6, 1).clone(), out[42].clone()

    @staticmethod
    def backward(ctx, gH, gg, ge):
        src, tgt, nrm, best = ctx.saved_tensors
        src_c, tgt_c, nrm_c = _f32c(src), _f32c(tgt), _f32c(nrm)
        dev = src.device
        z = lambda t, n: torch.zeros(n, dtype=torch.float32, device=dev) if t is None else _f32c(t).reshape(-1)
        gout = torch.cat([z(gH, 36), z(gg, 6), z(ge, 1)])
        g_src = torch.zeros_like(src_c)
        g_tgt = torch.zeros_like(tgt_c)
        g_nrm = torch.zeros_like(nrm_c)
        ns, nt = src_c.shape[0], tgt_c.shape[0]
        if deterministic():
            ws = workspace(ws_bytes("gs_icp_linearize_backward_det_ws_bytes", ns, nt), dev, "linearize_bwd_det")
            d_ns, d_nt = dev_int(ns, dev), dev_int(nt, dev)  # (held: two temporaries could share one freed block)
            call("gs_icp_linearize_backward_det", ptr(src_c), ptr(d_ns), ns, ptr(tgt_c), ptr(nrm_c), ptr(d_nt), nt, ptr(best), _thresh(ctx.dist_thresh), ptr(gout), ptr(g_src), ptr(g_tgt), ptr(g_nrm), ptr(ws), ws.numel(), stream())
        else:
            call("gs_icp_linearize_backward", ptr(src_c), ptr(dev_int(ns, dev)), ns, ptr(tgt_c), ptr(nrm_c), ptr(best),
                 _thresh(ctx.dist_thresh), ptr(gout), ptr(g_src), ptr(g_tgt), ptr(g_nrm), stream())
        return g_src, g_tgt, g_nrm, None, None


def icp_linearize(src, tgt, nrm, best, dist_thresh):
    return _LinearizeFn.apply(src, tgt, nrm, best, dist_thresh)


def icp_rows_raw(src, tgt, nrm, best, dist_thresh):
    """-> A (Ns,6), b (Ns,), keep (Ns,) uint8 (rows failing the distance filter are zero)."""
    src, tgt, nrm = _f32c(src), _f32c(tgt), _f32c(nrm)
    dev = src.device
    n = src.shape[0]
    A = torch.empty((n, 6), dtype=torch.float32, device=dev)
    b = torch.empty(n, dtype=torch.float32, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    call("gs_icp_rows", ptr(src), ptr(dev_int(n, dev)), n, ptr(tgt), ptr(nrm), ptr(best), _thresh(dist_thresh), ptr(A),
         ptr(b), ptr(keep), stream())
    return A, b, keep


class _TransformFn(torch.autograd.Function):
    """(pts (N,3), T (4,4)) -> R pts + t (reference geometry/geometryutils.py:780-792)."""

    @staticmethod
    def forward(ctx, pts, T):
        p, Tc = _f32c(pts), _f32c(T)
        out = torch.empty_like(p)
        call("gs_transform_points", ptr(p), ptr(dev_int(p.shape[0], p.device)), p.shape[0], ptr(Tc), ptr(out), stream())
        ctx.save_for_backward(p, Tc)
        return out

    @staticmethod
    def backward(ctx, g):
        p, T = ctx.saved_tensors
        g = _f32c(g)
        # adjoint w.r.t. the points is the transform by R^T (no translation): same kernel, T' = [R^T 0]
        Tt = torch.zeros_like(T)
        Tt[:3, :3] = T[:3, :3].t()
        Tt[3, 3] = 1.0
        gp = torch.empty_like(p)
        call("gs_transform_points", ptr(g), ptr(dev_int(p.shape[0], p.device)), p.shape[0], ptr(Tt.contiguous()), ptr(gp), stream())
        gT = torch.zeros_like(T)
        gT[:3, :3] = g.t() @ p  # 3xN @ Nx3: a library GEMM, O(N) once per call
        gT[:3, 3] = g.sum(0)
        return gp, gT


def transform_points(pts: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    require_hip(pts, T, op="transform_points")
    return _TransformFn.apply(pts, T)


# ---------------------------------------------------------------------------------------------- X
def icp_device_loop(src, tgt, nrm, init_T, numiters, damp, dist_thresh, grad_params=None, want_trace=False,
                    want_best=False):
    """Whole (grad)ICP loop on the device, no host sync (reference odometry/icputils.py:310-367,
    :479-545).  Returns (T (4,4), best_last or None, trace (numiters,48) or None)."""
    require_hip(src, tgt, nrm, init_T, op="icp")
    src, tgt, nrm, init_T = _f32c(src.detach()), _f32c(tgt.detach()), _f32c(nrm.detach()), _f32c(init_T.detach())
    dev = src.device
    ns, nt = src.shape[0], tgt.shape[0]
    if ns == 0 or nt == 0:
        raise ValueError("ICP needs non-empty source and target clouds (got {} and {} points)".format(ns, nt))
    T = torch.empty((4, 4), dtype=torch.float32, device=dev)
    best = torch.empty(ns, dtype=torch.int64, device=dev) if want_best else None
    trace = torch.zeros((max(numiters, 1), 48), dtype=torch.float32, device=dev) if want_trace else None
    ws = workspace(ws_bytes("gs_icp_ws_bytes", ns, nt), dev, "icp")
    d_ns, d_nt = dev_int(ns, dev), dev_int(nt, dev)
    if grad_params is None:
        call("gs_icp_point_to_plane", ptr(src), ptr(d_ns), ns, ptr(tgt), ptr(nrm), ptr(d_nt), nt, ptr(init_T),
             int(numiters), float(damp), _thresh(dist_thresh), None, ptr(T), ptr(best), ptr(trace), ptr(ws), ws.numel(), stream())
    else:
        lmax, Bp, B2, nu = grad_params
        call("gs_icp_point_to_plane_grad", ptr(src), ptr(d_ns), ns, ptr(tgt), ptr(nrm), ptr(d_nt), nt, ptr(init_T),
             int(numiters), float(damp), _thresh(dist_thresh), float(lmax), float(Bp), float(B2), float(nu), None, ptr(T),
             ptr(best), ptr(trace), ptr(ws), ws.numel(), stream())
    return T, best, trace


def _grad_lm(grad_params):
    """grad_params (lambda_max, B, B2, nu) of gradICP, or None for plain ICP -> (grad_lm, lmax, Bp, B2, nu) as the C calls
    take them (plain ICP ignores the four floats)."""
    lmax, Bp, B2, nu = grad_params if grad_params is not None else (2.0, 1.0, 1.0, 200.0)
    return (1 if grad_params is not None else 0), float(lmax), float(Bp), float(B2), float(nu)


class _IcpLoopFn(torch.autograd.Function):
    """Differentiable point_to_plane_ICP / gradICP as ONE node: the taped device loop forward, the
    device-side reverse pass over the tape backward (no host sync in either direction)."""

    @staticmethod
    def forward(ctx, src, tgt, nrm, init_T, numiters, damp, dist_thresh, grad_params):
        src, tgt, nrm, init_T = _f32c(src.detach()), _f32c(tgt.detach()), _f32c(nrm.detach()), _f32c(init_T.detach())
        dev = src.device
        ns, nt = src.shape[0], tgt.shape[0]
        if ns == 0 or nt == 0:
            raise ValueError("ICP needs non-empty source and target clouds (got {} and {} points)".format(ns, nt))
        grad_lm, lmax, Bp, B2, nu = _grad_lm(grad_params)
        T = torch.empty((4, 4), dtype=torch.float32, device=dev)
        best = torch.empty(ns, dtype=torch.int64, device=dev)
        tape = torch.empty(ws_bytes("gs_icp_tape_bytes", ns, int(numiters), grad_lm), dtype=torch.uint8, device=dev)
        ws = workspace(ws_bytes("gs_icp_ws_bytes", ns, nt), dev, "icp")
        d_ns, d_nt = dev_int(ns, dev), dev_int(nt, dev)
        call("gs_icp_point_to_plane_taped", ptr(src), ptr(d_ns), ns, ptr(tgt), ptr(nrm), ptr(d_nt), nt, ptr(init_T),
             int(numiters), float(damp), _thresh(dist_thresh), grad_lm, lmax, Bp, B2, nu, None,
             ptr(T), ptr(best), ptr(tape), tape.numel(), ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(src, tgt, nrm, init_T, tape, d_ns, d_nt)
        ctx.cfg = (int(numiters), _thresh(dist_thresh), grad_lm, lmax, Bp, B2, nu)
        ctx.mark_non_differentiable(best)
        return T, best

    @staticmethod
    def backward(ctx, gT, _gbest):
        src, tgt, nrm, init_T, tape, d_ns, d_nt = ctx.saved_tensors
        numiters, thresh, grad_lm, lmax, Bp, B2, nu = ctx.cfg
        dev = src.device
        ns, nt = src.shape[0], tgt.shape[0]
        gT = _f32c(gT)
        need_tgt, need_nrm = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        g_src = torch.empty_like(src)
        g_tgt = torch.empty_like(tgt) if need_tgt else None
        g_nrm = torch.empty_like(nrm) if need_nrm else None
        g_init = torch.empty((4, 4), dtype=torch.float32, device=dev)
        if deterministic():
            entry = "gs_icp_point_to_plane_backward_det"
            ws = workspace(ws_bytes("gs_icp_backward_det_ws_bytes", ns, nt, numiters, grad_lm), dev, "icp_bwd_det")
        else:
            entry = "gs_icp_point_to_plane_backward"
            ws = workspace(ws_bytes("gs_icp_backward_ws_bytes", ns), dev, "icp_bwd")
        call(entry, ptr(src), ptr(d_ns), ns, ptr(tgt), ptr(nrm), ptr(d_nt), nt, ptr(init_T), numiters, thresh,
             grad_lm, lmax, Bp, B2, nu, ptr(tape), tape.numel(), ptr(gT), ptr(g_src), ptr(g_tgt), ptr(g_nrm), ptr(g_init),
             ptr(ws), ws.numel(), stream())
        return g_src, g_tgt, g_nrm, g_init, None, None, None, None


def icp_loop_autograd(src, tgt, nrm, init_T, numiters, damp, dist_thresh, grad_params=None):
    """(T (4,4) with grad_fn, packed NN of the last iteration's first solve)."""
    require_hip(src, tgt, nrm, init_T, op="icp")
    return _IcpLoopFn.apply(src, tgt, nrm, init_T, numiters, damp, dist_thresh, grad_params)


def slam_localize_raw(depth, K, prev_poses, map_points, map_normals, map_counts_i32, ds, numiters, damp, dist_thresh,
                      grad_params=None, out=None, want_maps=True):
    """One fused, sync-free ICPSLAM._localize (reference slam/icpslam.py:238-247).
    depth (B,1,H,W,1), K (B,1,4,4), prev_poses (B,1,4,4), map padded (B,Nmax,3) x2 + counts (B,) int32.
    Returns (poses (B,1,4,4), V, N): the local maps are handed back so the caller can cache them (want_maps=False: not
    computed, None returned).  `out`: a contiguous float32 (B,1,4,4) tensor the poses are written to (a sequence driver's
    slice of its pose array: no copy launch)."""
    require_hip(depth, K, prev_poses, map_points, map_normals, map_counts_i32, op="slam_localize")
    depth, K, prev = _f32c(depth.detach()), _f32c(K.detach()), _f32c(prev_poses.detach())
    mp, mn = _f32c(map_points.detach()), _f32c(map_normals.detach())
    B, _, H, W = depth.shape[:4]
    Nmax = mp.shape[1]
    dev = depth.device
    mk = lambda: torch.empty((B, 1, H, W, 3), dtype=torch.float32, device=dev)
    V, N, gV = (mk() if want_maps else None), (mk() if want_maps else None), mk()
    if out is None:
        out = torch.empty((B, 1, 4, 4), dtype=torch.float32, device=dev)
    elif not (out.is_contiguous() and out.dtype == torch.float32 and out.numel() == 16 * B and out.device == dev):
        raise ValueError("slam_localize: `out` must be a contiguous float32 (B,1,4,4) tensor on the inputs' device")
    ws = workspace(ws_bytes("gs_slam_localize_ws_bytes", B, H, W, int(ds), Nmax), dev, "localize")
    grad_lm, lmax, Bp, B2, nu = _grad_lm(grad_params)
    call("gs_slam_localize", ptr(depth), ptr(K), ptr(prev), B, H, W, int(ds), ptr(mp), ptr(mn), ptr(map_counts_i32), Nmax,
         grad_lm, int(numiters), float(damp), _thresh(dist_thresh), lmax, Bp, B2, nu, ptr(V), ptr(N), ptr(gV), None, ptr(out),
         ptr(ws), ws.numel(), stream())
    return out, V, N


def slam_localize_taped_raw(gV, depth, K, prev_poses, map_points, map_normals, map_counts_i32, ds, numiters, damp, dist_thresh,
                            grad_params=None):
    """slam_localize_raw that also fills the tape of its reverse pass -> (poses (B,1,4,4), tape).  gV (B,1,H,W,3) is the live
    frame's global vertex map under the previous pose: an input here, so that its adjoint chains into the maps' own."""
    require_hip(gV, depth, K, prev_poses, map_points, map_normals, map_counts_i32, op="slam_localize")
    gV, depth, K, prev = _f32c(gV.detach()), _f32c(depth.detach()), _f32c(K.detach()), _f32c(prev_poses.detach())
    mp, mn = _f32c(map_points.detach()), _f32c(map_normals.detach())
    B, _, H, W = depth.shape[:4]
    Nmax = mp.shape[1]
    dev = depth.device
    grad_lm, lmax, Bp, B2, nu = _grad_lm(grad_params)
    out = torch.empty((B, 1, 4, 4), dtype=torch.float32, device=dev)
    tape = torch.empty(ws_bytes("gs_slam_localize_tape_bytes", B, H, W, int(ds), Nmax, int(numiters), grad_lm),
                       dtype=torch.uint8, device=dev)
    ws = workspace(ws_bytes("gs_slam_localize_ws_bytes", B, H, W, int(ds), Nmax), dev, "localize")
    call("gs_slam_localize_taped", ptr(depth), ptr(gV), ptr(K), ptr(prev), B, H, W, int(ds), ptr(mp), ptr(mn),
         ptr(map_counts_i32), Nmax, grad_lm, int(numiters), float(damp), _thresh(dist_thresh), lmax, Bp, B2, nu, ptr(out),
         ptr(tape), tape.numel(), ptr(ws), ws.numel(), stream())
    return out, tape


def slam_localize_backward_raw(prev_poses, map_points, map_normals, nmax, H, W, ds, numiters, dist_thresh, grad_params, tape,
                               g_poses, g_gV, g_map_points, g_map_normals, g_prev, accumulate):
    """Reverse pass of slam_localize_taped_raw (same prev_poses and map; `nmax` its row bound, the arrays may hold more rows
    by now) into the caller's contiguous float32 buffers: g_gV (B,1,H,W,3) and g_prev (B,1,4,4) are written, g_map_points /
    g_map_normals (None = not wanted) written (accumulate = 0) or added into (1: the running adjoint of a whole map)."""
    B, dev = prev_poses.shape[0], prev_poses.device
    ds, numiters = int(ds), int(numiters)
    grad_lm, lmax, Bp, B2, nu = _grad_lm(grad_params)
    g_poses = _f32c(g_poses)
    if deterministic():
        det, size = "_det", ws_bytes("gs_slam_localize_backward_det_ws_bytes", B, H, W, ds, nmax, numiters, grad_lm)
    else:
        det, size = "", ws_bytes("gs_slam_localize_backward_ws_bytes", B, H, W, ds, nmax)
    ws = workspace(size, dev, "localize_bwd" + det)
    call("gs_slam_localize_backward" + det, ptr(prev_poses), B, H, W, ds, ptr(map_points), ptr(map_normals), nmax, grad_lm,
         numiters, _thresh(dist_thresh), lmax, Bp, B2, nu, ptr(tape), tape.numel(), ptr(g_poses), ptr(g_gV), ptr(g_map_points),
         ptr(g_map_normals), ptr(g_prev), int(accumulate), ptr(ws), ws.numel(), stream())


class _LocalizeFn(torch.autograd.Function):
    """Differentiable ICPSLAM._localize as ONE node (slam_localize_taped_raw / slam_localize_backward_raw): gradients reach
    the live frame's global vertex map, the map points / normals that served as ICP targets and the previous
    pose; nothing synchronises with the host in either direction."""

    @staticmethod
    def forward(ctx, gV, depth, K, prev_poses, mp, mn, counts_i32, ds, numiters, damp, dist_thresh, grad_params):
        prev, mp, mn = _f32c(prev_poses.detach()), _f32c(mp.detach()), _f32c(mn.detach())
        out, tape = slam_localize_taped_raw(gV, depth, K, prev, mp, mn, counts_i32, ds, numiters, damp, dist_thresh, grad_params)
        ctx.save_for_backward(prev, mp, mn, tape)
        ctx.cfg = (depth.shape[2], depth.shape[3], ds, numiters, dist_thresh, grad_params)
        return out

    @staticmethod
    def backward(ctx, g_out):
        prev, mp, mn, tape = ctx.saved_tensors
        H, W = ctx.cfg[:2]
        B, dev = prev.shape[0], prev.device
        g_gV = torch.empty((B, 1, H, W, 3), dtype=torch.float32, device=dev)
        g_mp = torch.empty_like(mp) if ctx.needs_input_grad[4] else None
        g_mn = torch.empty_like(mn) if ctx.needs_input_grad[5] else None
        g_prev = torch.empty((B, 1, 4, 4), dtype=torch.float32, device=dev)
        slam_localize_backward_raw(prev, mp, mn, mp.shape[1], *ctx.cfg, tape, g_out, g_gV, g_mp, g_mn, g_prev, 0)
        return g_gV, None, None, g_prev, g_mp, g_mn, None, None, None, None, None, None


def slam_localize_autograd(gV, depth, K, prev_poses, map_points, map_normals, map_counts_i32, ds, numiters, damp, dist_thresh,
                           grad_params=None):
    """Differentiable fused localisation -> poses (B,1,4,4) with grad_fn."""
    return _LocalizeFn.apply(gV, depth, K, prev_poses, map_points, map_normals, map_counts_i32, ds, numiters, damp, dist_thresh,
                             grad_params)


def _pointfusion_update_args(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts, map_counts_i32, nmax=None):
    """The checks and the C argument prefix that gs_pointfusion_update, its taped form and its reverse pass share
    -> (B, H, W, nmax, held, prefix).  nmax: the row bound handed to the kernels (default: the rows the map arrays hold);
    held: the contiguous K and poses behind the prefix's pointers, for the caller to keep until its call is made."""
    require_hip(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts, map_counts_i32, op="pointfusion_update")
    for name, x in (("map_points", map_points), ("map_normals", map_normals), ("map_colors", map_colors),
                    ("map_ccounts", map_ccounts), ("depth", depth), ("rgb", rgb)):
        if not (x.is_contiguous() and x.dtype == torch.float32):
            raise ValueError("pointfusion_update: {} must be contiguous float32 (it is updated / read in place)".format(name))
    B, H, W = depth.shape[:3]
    nmax = map_points.shape[1] if nmax is None else int(nmax)
    held = K, poses = _f32c(K), _f32c(poses)
    return B, H, W, nmax, held, (ptr(depth), ptr(rgb), ptr(K), ptr(poses), B, H, W, ptr(map_points), ptr(map_normals),
                                 ptr(map_colors), ptr(map_ccounts), ptr(map_counts_i32), nmax)


def pointfusion_update_raw(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts, map_counts_i32, dist_th,
                           dot_th, sigma, stats=None):
    """One fused, sync-free PointFusion map update on arena arrays (reference slam/fusionutils.py:761-789 with
    inplace=True).  depth (B,H,W[,1]), rgb (B,H,W,3), K / poses (B,[1,]4,4); map_* (B,Nmax,C) float32 contiguous,
    rows beyond map_counts zero; the caller guarantees counts + H*W <= Nmax.  Everything is updated in place,
    including map_counts_i32 (B,) int32 on the device; `stats` (4+B,) int32 receives the step's counters."""
    B, H, W, Nmax, held, prefix = _pointfusion_update_args(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts,
                                                           map_counts_i32)
    ws = workspace(ws_bytes("gs_pointfusion_update_ws_bytes", B, H, W, Nmax), depth.device, "fusion_step")
    call("gs_pointfusion_update", *prefix, float(dist_th), float(dot_th), float(sigma), ptr(stats), ptr(ws), ws.numel(), stream())


def pointfusion_update_taped_raw(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts, map_counts_i32, dist_th,
                                 dot_th, sigma, stats=None):
    """pointfusion_update_raw that also fills the frame's tape for pointfusion_update_backward_raw -> tape."""
    B, H, W, Nmax, held, prefix = _pointfusion_update_args(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts,
                                                           map_counts_i32)
    tape = torch.empty(ws_bytes("gs_pointfusion_update_tape_bytes", B, H, W), dtype=torch.uint8, device=depth.device)
    ws = workspace(ws_bytes("gs_pointfusion_update_ws_bytes", B, H, W, Nmax), depth.device, "fusion_step")
    call("gs_pointfusion_update_taped", *prefix, float(dist_th), float(dot_th), float(sigma), ptr(stats), ptr(tape), tape.numel(),
         ptr(ws), ws.numel(), stream())
    return tape


def pointfusion_update_backward_raw(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts, map_counts_i32, nmax,
                                    sigma, tape, G_points, G_normals, G_colors, G_ccounts, g_V, g_gV, g_gN, g_rgb):
    """One frame back over the tape of pointfusion_update_taped_raw (`nmax`: that call's row bound; the arrays may hold more
    rows by now).  G_* (B,rows,C), the running adjoint of the WHOLE map, is pulled back in place at the matched / appended rows;
    the map and counts are restored to the previous frame's; g_V, g_gV, g_gN, g_rgb (B,H,W,3) receive the frame's adjoints."""
    B, H, W, nmax, held, prefix = _pointfusion_update_args(depth, rgb, K, poses, map_points, map_normals, map_colors, map_ccounts,
                                                           map_counts_i32, nmax)
    ws = workspace(ws_bytes("gs_pointfusion_update_backward_ws_bytes", B, H, W), depth.device, "fusion_bwd")
    call("gs_pointfusion_update_backward", *prefix, float(sigma), ptr(tape), tape.numel(), ptr(G_points), ptr(G_normals),
         ptr(G_colors), ptr(G_ccounts), ptr(g_V), ptr(g_gV), ptr(g_gN), ptr(g_rgb), ptr(ws), ws.numel(), stream())


def aggregate_update_raw(depth, rgb, K, poses, map_points, map_normals, map_colors, map_counts_i32, stats=None):
    """One fused, sync-free ICPSLAM map update on arena arrays (reference slam/fusionutils.py:725-758 with
    inplace=True): every valid live-frame pixel is appended, counts advance on the device."""
    require_hip(depth, rgb, K, poses, map_points, map_normals, map_colors, map_counts_i32, op="aggregate_update")
    for name, x in (("map_points", map_points), ("map_normals", map_normals), ("map_colors", map_colors), ("depth", depth), ("rgb", rgb)):
        if not (x.is_contiguous() and x.dtype == torch.float32):
            raise ValueError("aggregate_update: {} must be contiguous float32 (it is updated / read in place)".format(name))
    B, H, W = depth.shape[:3]
    K, poses = _f32c(K), _f32c(poses)
    ws = workspace(ws_bytes("gs_aggregate_update_ws_bytes", B, H, W), depth.device, "aggregate_step")
    call("gs_aggregate_update", ptr(depth), ptr(rgb), ptr(K), ptr(poses), B, H, W, ptr(map_points), ptr(map_normals),
         ptr(map_colors), ptr(map_counts_i32), map_points.shape[1], ptr(stats), ptr(ws), ws.numel(), stream())


# ---------------------------------------------------------------------------------------------- C / U / F / A
def fusion_similar_raw(rows, n_rows_dev, max_rows, gV, gN, map_points, map_normals, dist_th, dot_th):
    """-> keep (max_rows,) uint8, max_dot (1,) float32 device."""
    gV, gN, mp, mn = _f32c(gV), _f32c(gN), _f32c(map_points), _f32c(map_normals)
    H, W = gV.shape[2:4]
    dev = gV.device
    keep = torch.zeros(max(max_rows, 1), dtype=torch.uint8, device=dev)
    max_dot = torch.zeros(1, dtype=torch.float32, device=dev)
    call("gs_fusion_similar", ptr(rows), ptr(n_rows_dev), max_rows, ptr(gV), ptr(gN), H, W, ptr(mp), ptr(mn),
         mp.shape[1], float(dist_th), float(dot_th), ptr(keep), ptr(max_dot), stream())
    return keep, max_dot


def fusion_unique_raw(rows, keep, n_rows_dev, max_rows, gV, map_points, map_ccounts):
    """-> (rows buffer (B*H*W,4) int64, count (1,) int32 device)."""
    gV, mp, cc = _f32c(gV), _f32c(map_points), _f32c(map_ccounts)
    B, _, H, W = gV.shape[:4]
    dev = gV.device
    out = torch.empty((B * H * W, 4), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = workspace(ws_bytes("gs_fusion_unique_ws_bytes", B, H, W), dev, "unique")
    call("gs_fusion_unique", ptr(rows), ptr(keep), ptr(n_rows_dev), max_rows, ptr(gV), B, H, W, ptr(mp), ptr(cc),
         mp.shape[1], ptr(out), ptr(cnt), ptr(ws), ws.numel(), stream())
    return out, cnt


def fusion_merge_raw(rows, n_rows_dev, max_rows, gV, gN, rgb, alpha, counts_dev, mp, mn, mc, cc):
    """-> new (points, normals, colors, ccounts), each a fresh (B,Nmax,C) tensor."""
    B, _, H, W = gV.shape[:4]
    Nmax = mp.shape[1]
    dev = gV.device
    op, on, oc, occ = (torch.empty_like(x) for x in (mp, mn, mc, cc))
    ws = workspace(ws_bytes("gs_fusion_merge_ws_bytes", B, Nmax), dev, "merge")
    call("gs_fusion_merge", ptr(rows), ptr(n_rows_dev), max_rows, ptr(gV), ptr(gN), ptr(rgb), ptr(alpha), B, H, W, Nmax,
         ptr(counts_dev), ptr(mp), ptr(mn), ptr(mc), ptr(cc), ptr(op), ptr(on), ptr(oc), ptr(occ), ptr(ws), ws.numel(),
         stream())
    return op, on, oc, occ


class _MergeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, counts_dev, gV, gN, rgb, alpha, mp, mn, mc, cc):
        gV, gN, rgb, alpha, mp, mn, mc, cc = (_f32c(x) for x in (gV, gN, rgb, alpha, mp, mn, mc, cc))
        n_dev = dev_int(rows.shape[0], rows.device)
        outs = fusion_merge_raw(rows, n_dev, rows.shape[0], gV, gN, rgb, alpha, counts_dev, mp, mn, mc, cc)
        ctx.save_for_backward(rows, counts_dev, gV, gN, rgb, alpha, mp, mn, mc, cc)
        return outs

    @staticmethod
    def backward(ctx, gop, gon, goc, gocc):
        rows, counts_dev, gV, gN, rgb, alpha, mp, mn, mc, cc = ctx.saved_tensors
        B, _, H, W = gV.shape[:4]
        Nmax = mp.shape[1]
        dev = gV.device
        gop, gon, goc, gocc = (None if g is None else _f32c(g) for g in (gop, gon, goc, gocc))
        gip, ginn, gic, gicc = (torch.empty_like(x) for x in (mp, mn, mc, cc))
        ggv, ggn, grgb, galpha = (torch.zeros_like(x) for x in (gV, gN, rgb, alpha))
        ws = workspace(ws_bytes("gs_fusion_merge_ws_bytes", B, Nmax), dev, "merge")
        call("gs_fusion_merge_backward", ptr(rows), ptr(dev_int(rows.shape[0], dev)), rows.shape[0], ptr(gV), ptr(gN),
             ptr(rgb), ptr(alpha), B, H, W, Nmax, ptr(counts_dev), ptr(mp), ptr(mn), ptr(mc), ptr(cc), ptr(gop), ptr(gon),
             ptr(goc), ptr(gocc), ptr(gip), ptr(ginn), ptr(gic), ptr(gicc), ptr(ggv), ptr(ggn), ptr(grgb), ptr(galpha),
             ptr(ws), ws.numel(), stream())
        return None, None, ggv, ggn, grgb, galpha, gip, ginn, gic, gicc


def fusion_merge(rows, counts_dev, gV, gN, rgb, alpha, mp, mn, mc, cc):
    """Autograd-aware merge of the unique rows into the padded map arrays."""
    return _MergeFn.apply(rows, counts_dev, gV, gN, rgb, alpha, mp, mn, mc, cc)


def fusion_new_mask_raw(depth, rows, n_rows_dev, max_rows):
    """depth (B,1,H,W,1) -> mask (B,H,W) uint8: valid depth and not matched."""
    depth = _f32c(depth)
    B, _, H, W = depth.shape[:4]
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=depth.device)
    call("gs_fusion_new_mask", ptr(depth), ptr(rows), ptr(n_rows_dev), max_rows, B, H, W, ptr(mask), stream())
    return mask


# ---------------------------------------------------------------------------------------------- argument checkers the modules share
def _as_float(value) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        return float("nan")


def _number(value, name, op):
    x = _as_float(value)
    if math.isnan(x):
        raise ValueError("{}: {} should be a number. Got {!r}.".format(op, name, value))
    return x


def _positive(value, name, op):
    x = _as_float(value)
    x32 = float(torch.tensor(x, dtype=torch.float32)) if math.isfinite(x) else x  # what the kernels compute with
    if not (math.isfinite(x32) and x32 > 0.0):
        raise ValueError("{}: {} should be a finite positive number. Got {!r}.".format(op, name, value))
    return x


def _counts(c, B, name, op):
    if c.dtype != torch.int32 or c.numel() != B:
        raise ValueError("{}: {} should be {} int32 values. Got {} of {}.".format(op, name, B, c.numel(), c.dtype))
    return c.contiguous()


def _padded_pair(x, y, x_counts, y_counts, names, op):
    """Two padded clouds (B, N, 3) with int32 device counts, called names[0] / names[1] in the messages -> (x, y, counts of x,
    counts of y), contiguous (fp32 for the clouds); `x is y` stays so."""
    require_hip(x, y, x_counts, y_counts, op=op)
    same = x is y
    x = _f32c(x)
    y = x if same else _f32c(y)
    for name, t in zip(names, (x, y)):
        if t.ndim != 3 or t.shape[-1] != 3 or t.shape[1] == 0:
            raise ValueError("{}: {} should have shape (B, N, 3) with N > 0. Got {}.".format(op, name, tuple(t.shape)))
    B = x.shape[0]
    if y.shape[0] != B or B == 0:
        raise ValueError("{}: {} and {} should share a batch size B > 0. Got {} and {}.".format(op, *names, x.shape[0], y.shape[0]))
    return x, y, _counts(x_counts, B, names[0] + "_counts", op), _counts(y_counts, B, names[1] + "_counts", op)


# ---------------------------------------------------------------------------------------------- R
def _render_args(points_padded, normals_padded, colors_padded, counts_i32, poses_b44, K_b44, H, W, op):
    require_hip(points_padded, normals_padded, colors_padded, counts_i32, poses_b44, K_b44, op=op)
    pts, nrm, col = _f32c(points_padded), _f32c(normals_padded), _f32c(colors_padded)
    poses, K = _f32c(poses_b44), _f32c(K_b44)
    if pts.ndim != 3 or pts.shape[-1] != 3:
        raise ValueError("{}: points_padded should have shape (B, N, 3). Got {}.".format(op, tuple(pts.shape)))
    B = pts.shape[0]
    for name, x in (("normals_padded", nrm), ("colors_padded", col)):
        if x is not None and x.shape != pts.shape:
            raise ValueError("{}: {} should have the shape of points_padded {}. Got {}.".format(op, name, tuple(pts.shape), tuple(x.shape)))
    for name, x in (("poses", poses), ("intrinsics", K)):
        if x.numel() != 16 * B or x.shape[-2:] != (4, 4):
            raise ValueError("{}: {} should hold one 4x4 matrix per batch element (B = {}). Got {}.".format(op, name, B, tuple(x.shape)))
    counts = _counts(counts_i32, B, "counts", op)
    if int(H) <= 0 or int(W) <= 0 or pts.shape[1] == 0:
        raise ValueError("{}: needs a non-empty map array and a positive image size. Got N = {}, H = {}, W = {}.".format(
            op, pts.shape[1], H, W))
    return pts, nrm, col, counts, poses, K


def render_map_raw(points_padded, normals_padded, colors_padded, counts_i32, poses_b44, K_b44, H: int, W: int):
    """The map seen from one camera per batch element: z-buffered (index (B,H,W) int32, depth (B,H,W), points, normals,
    colors (B,H,W,3)).  A pixel shows the map row with the smallest camera-frame z among the rows find_active_map_points
    puts on it (ties: the smallest row), or index -1 / zeros; normals / colors are None when the map has none.  Three
    launches, no [b,n,h,w] table (the chain it replaces: project_active_raw rows, a scatter-min key per pixel, gathers)."""
    pts, nrm, col, counts, poses, K = _render_args(points_padded, normals_padded, colors_padded, counts_i32, poses_b44, K_b44, H, W,
                                                   "render_map")
    B, Nmax = pts.shape[:2]
    H, W = int(H), int(W)
    dev = pts.device
    index = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    img = lambda have: torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if have else None
    op, on, oc = img(True), img(nrm is not None), img(col is not None)
    ws = workspace(ws_bytes("gs_render_map_ws_bytes", B, H, W), dev, "render")
    call("gs_render_map", ptr(pts), ptr(nrm), ptr(col), ptr(counts), B, Nmax, ptr(poses), ptr(K), H, W, ptr(index), ptr(depth),
         ptr(op), ptr(on), ptr(oc), ptr(ws), ws.numel(), stream())
    return index, depth, op, on, oc


def render_map_backward_raw(points_padded, counts_i32, poses_b44, index, g_depth=None, g_points=None, g_normals=None,
                            g_colors=None, want=(True, True, True, True)):
    """Adjoint of render_map_raw for the winners in `index` (constants): -> (g_map_points, g_map_normals, g_map_colors
    (B,N,3), g_poses (B,4,4)), each fully written, or None where `want` says it is not needed.  No atomics: bit-reproducible."""
    require_hip(points_padded, counts_i32, poses_b44, index, g_depth, g_points, g_normals, g_colors, op="render_map_backward")
    pts, poses = _f32c(points_padded), _f32c(poses_b44)
    B, Nmax = pts.shape[:2]
    H, W = index.shape[1:3]
    dev = pts.device
    index = index.contiguous()
    gd, gp, gn, gc = (_f32c(g) for g in (g_depth, g_points, g_normals, g_colors))
    row = lambda w: torch.empty((B, Nmax, 3), dtype=torch.float32, device=dev) if w else None
    o_p, o_n, o_c = row(want[0]), row(want[1]), row(want[2])
    o_T = torch.empty((B, 4, 4), dtype=torch.float32, device=dev) if want[3] else None
    ws = workspace(ws_bytes("gs_render_map_backward_ws_bytes", B, H, W), dev, "render_bwd")
    call("gs_render_map_backward", ptr(pts), ptr(counts_i32), B, Nmax, ptr(poses), H, W, ptr(index), ptr(gd), ptr(gp), ptr(gn),
         ptr(gc), ptr(o_p), ptr(o_n), ptr(o_c), ptr(o_T), ptr(ws), ws.numel(), stream())
    return o_p, o_n, o_c, o_T


class _RenderFn(torch.autograd.Function):
    """(map points, normals, colors, poses) -> (index, depth, points, normals, colors) with the hand-written adjoint.
    `index` is not differentiable; neither is the pixel a row lands on (a constant of the graph), so the intrinsics get None."""

    @staticmethod
    def forward(ctx, points, normals, colors, counts_i32, poses, K, H, W):
        index, depth, op, on, oc = render_map_raw(points, normals, colors, counts_i32, poses, K, H, W)
        ctx.save_for_backward(points, counts_i32, poses, index)
        ctx.mark_non_differentiable(index)
        return index, depth, op, on, oc

    @staticmethod
    def backward(ctx, _g_index, g_depth, g_op, g_on, g_oc):
        points, counts_i32, poses, index = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[i] for i in (0, 1, 2, 4))
        g_p, g_n, g_c, g_T = render_map_backward_raw(points, counts_i32, poses, index, g_depth, g_op, g_on, g_oc, want)
        return (None if g_p is None else g_p.view_as(points), g_n, g_c, None, None if g_T is None else g_T.view_as(poses), None,
                None, None)


def render_map(points_padded, normals_padded, colors_padded, counts_i32, poses_b44, K_b44, H: int, W: int):
    """Autograd-aware render_map_raw: gradients reach the map's points / normals / colors and the poses."""
    return _RenderFn.apply(points_padded, normals_padded, colors_padded, counts_i32, poses_b44, K_b44, int(H), int(W))


# ---------------------------------------------------------------------------------------------- M
KEY_NONE = -1  # a packed key without a neighbour (all ones), as int64


def chamfer_raw(a, b, a_counts, b_counts, tau2: float = float("inf"), reorder: bool = True, out=None):
    """Two-sided exact nearest neighbours of padded clouds a (B,Na,3), b (B,Nb,3) with int32 device counts ->
    (stats (B,2,4) float64, keys_ab (B,Na) int64, keys_ba (B,Nb) int64).  stats[b, d] = [sum d2, sum d, #(d2 < tau2), max d2]
    of direction d (0: a -> b, 1: b -> a); keys are dist2_bits << 32 | index, KEY_NONE beyond the counts and where the other
    cloud is empty.  reorder scans each target in cell-grid order (same bits, another cost).  `out`: (keys_ab, keys_ba)
    buffers to write into (rows beyond the counts are left as they are)."""
    a, b, ca, cb = _padded_pair(a, b, a_counts, b_counts, ("a", "b"), "chamfer")
    B, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    dev = a.device
    stats = torch.empty((B, 2, 4), dtype=torch.float64, device=dev)
    if out is None:
        keys_ab = torch.full((B, Na), KEY_NONE, dtype=torch.int64, device=dev)
        keys_ba = torch.full((B, Nb), KEY_NONE, dtype=torch.int64, device=dev)
    else:
        keys_ab, keys_ba = out
    ws = workspace(ws_bytes("gs_chamfer_ws_bytes", B, Na, Nb), dev, "chamfer")
    call("gs_chamfer", ptr(a), ptr(ca), Na, ptr(b), ptr(cb), Nb, B, float(tau2), int(bool(reorder)), ptr(stats), ptr(keys_ab),
         ptr(keys_ba), ptr(ws), ws.numel(), stream())
    return stats, keys_ab, keys_ba


def chamfer_backward_raw(a, b, a_counts, b_counts, keys_ab, keys_ba, g2, g1, out=None):
    """Adjoint of chamfer_raw's sum d2 / sum d w.r.t. both clouds: g2, g1 (B,2) -> (g_a (B,Na,3), g_b (B,Nb,3)); the keys are
    constants.  The deterministic fold under torch.use_deterministic_algorithms, float atomics otherwise.  `out`: (g_a, g_b)
    buffers to write into (rows beyond the counts are left as they are; fresh buffers hold zeros there)."""
    a, b, ca, cb = _padded_pair(a, b, a_counts, b_counts, ("a", "b"), "chamfer_backward")
    require_hip(keys_ab, keys_ba, g2, g1, op="chamfer_backward")
    B, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    dev = a.device
    g2, g1 = _f32c(g2).reshape(B, 2), _f32c(g1).reshape(B, 2)
    keys_ab, keys_ba = keys_ab.contiguous(), keys_ba.contiguous()
    g_a, g_b = (torch.zeros_like(a), torch.zeros_like(b)) if out is None else out
    det = "_det" if deterministic() else ""
    nbytes = ws_bytes("gs_chamfer_backward{}_ws_bytes".format(det), B, Na, Nb)
    ws = workspace(nbytes, dev, "chamfer_bwd") if nbytes else None
    call("gs_chamfer_backward" + det, ptr(a), ptr(ca), Na, ptr(b), ptr(cb), Nb, B, ptr(keys_ab), ptr(keys_ba), ptr(g2), ptr(g1),
         ptr(g_a), ptr(g_b), ptr(ws), 0 if ws is None else ws.numel(), stream())
    return g_a, g_b


class _ChamferFn(torch.autograd.Function):
    """(a, b | counts) -> (sum d2 (B,2), sum d (B,2) in fp32; stats, keys_ab, keys_ba: constants).  The nearest neighbours are
    constants of the graph, as in every chamfer loss: the gradient is that of the distances to them."""

    @staticmethod
    def forward(ctx, a, b, a_counts, b_counts, tau2, reorder):
        stats, keys_ab, keys_ba = chamfer_raw(a, b, a_counts, b_counts, tau2, reorder)
        ctx.save_for_backward(a, b, a_counts, b_counts, keys_ab, keys_ba)
        ctx.mark_non_differentiable(stats, keys_ab, keys_ba)
        return stats[..., 0].float(), stats[..., 1].float(), stats, keys_ab, keys_ba

    @staticmethod
    def backward(ctx, g2, g1, _gs, _gk0, _gk1):
        a, b, a_counts, b_counts, keys_ab, keys_ba = ctx.saved_tensors
        zero = lambda g: torch.zeros((a.shape[0], 2), dtype=torch.float32, device=a.device) if g is None else g
        g_a, g_b = chamfer_backward_raw(a, b, a_counts, b_counts, keys_ab, keys_ba, zero(g2), zero(g1))
        return (g_a.view_as(a).to(a.dtype) if ctx.needs_input_grad[0] else None,
                g_b.view_as(b).to(b.dtype) if ctx.needs_input_grad[1] else None, None, None, None, None)


def chamfer(a, b, a_counts, b_counts, tau2: float = float("inf"), reorder: bool = True):
    """Autograd-aware chamfer_raw: gradients of sum d2 / sum d reach both clouds' points."""
    return _ChamferFn.apply(a, b, a_counts, b_counts, float(tau2), bool(reorder))


# ---------------------------------------------------------------------------------------------- V
def _voxel_origin(origin, op):
    vals = [0.0, 0.0, 0.0] if origin is None else [float(t) for t in (origin.tolist() if torch.is_tensor(origin) else origin)]
    if len(vals) != 3 or not all(math.isfinite(t) for t in vals):
        raise ValueError("{}: origin should be three finite numbers. Got {!r}.".format(op, origin))
    return (nv.c_f * 3)(*vals)


def _voxel_rows(x, counts, op):
    require_hip(x, counts, op=op)
    x = _f32c(x)
    if x.ndim != 3 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("{}: expected a padded (B, N, C) tensor with B > 0 and N > 0. Got {}.".format(op, tuple(x.shape)))
    return x, _counts(counts, x.shape[0], "counts", op)


def voxel_assign(points_padded, counts_i32, voxel_size, origin=None):
    """The voxel of every row of a padded batch (B,N,3) with int32 device counts, on the grid of edge `voxel_size` through
    `origin` (default 0): k = floor((p - origin) / voxel_size) in fp32.  Returns (voxel_of (B,N), n_voxels (B,), n_dropped (B,),
    voxel_count (B,N), voxel_first (B,N)), all int32: voxels are numbered in order of first appearance; voxel_of is -1 for
    padding rows and for dropped ones (non-finite, or |k| >= 2^20: counted in n_dropped); voxel_count / voxel_first hold 0 / -1
    beyond n_voxels.  No gradient: the assignment is a constant of the graph.  Nothing synchronises the host."""
    v, o = _positive(voxel_size, "voxel_size", "voxel_assign"), _voxel_origin(origin, "voxel_assign")
    with torch.no_grad():
        pts, counts = _voxel_rows(points_padded.detach(), counts_i32, "voxel_assign")
        if pts.shape[-1] != 3:
            raise ValueError("voxel_assign: points should have shape (B, N, 3). Got {}.".format(tuple(pts.shape)))
        B, N = pts.shape[0], pts.shape[1]
        dev = pts.device
        voxel_of, voxel_count, voxel_first = (torch.empty((B, N), dtype=torch.int32, device=dev) for _ in range(3))
        n_voxels, n_dropped = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2))
        ws = workspace(ws_bytes("gs_voxel_assign_ws_bytes", B, N), dev, "voxel_assign")
        call("gs_voxel_assign", ptr(pts), ptr(counts), N, B, v, o, ptr(voxel_of), ptr(n_voxels), ptr(n_dropped), ptr(voxel_count),
             ptr(voxel_first), ptr(ws), ws.numel(), stream())
    return voxel_of, n_voxels, n_dropped, voxel_count, voxel_first


VOXEL_SUM, VOXEL_MEAN = 0, 1  # gs_voxel_reduce's modes
VOXEL_NO_PREAGG = 2  # measurement switch of tools/voxel_timing.py (same bits, no pre-aggregation); not part of the stable interface


def _voxel_index_args(x, voxel_of, voxel_count, M_max, op):
    B, N = x.shape[0], x.shape[1]
    require_hip(voxel_of, voxel_count, op=op)
    for name, t in (("voxel_of", voxel_of), ("voxel_count", voxel_count)):
        if t.dtype != torch.int32 or tuple(t.shape) != (B, N):
            raise ValueError("{}: {} should be int32 of shape {}. Got {} of shape {}.".format(op, name, (B, N), t.dtype, tuple(t.shape)))
    if not 1 <= int(M_max) <= N:
        raise ValueError("{}: M_max should lie in 1 .. N = {}. Got {}.".format(op, N, M_max))
    if not 1 <= x.shape[2] <= 64:
        raise ValueError("{}: between 1 and 64 components per row are supported. Got {}.".format(op, x.shape[2]))
    return voxel_of.contiguous(), voxel_count.contiguous()


def voxel_reduce_raw(x, counts_i32, voxel_of, n_voxels, voxel_count, M_max, mode=VOXEL_MEAN):
    """x (B,N,C) -> (B,M_max,C): per voxel the sum of its members by the fold of gs_fixed128.hpp, rounded once to fp32 (mode 0),
    or that value divided by the member count (mode 1); rows beyond n_voxels are zero.  Same bits whatever the order of the
    rows.  The sum is exact while all terms of the call (every batch element, every channel) lie within 102 - ceil(log2 N)
    binary places of the call's largest finite |x|; what lies below that is truncated toward zero, term by term.  A NaN or
    infinite member gives its sum what a float sum gives and does not count towards the largest."""
    x, counts = _voxel_rows(x, counts_i32, "voxel_reduce")
    voxel_of, voxel_count = _voxel_index_args(x, voxel_of, voxel_count, M_max, "voxel_reduce")
    require_hip(n_voxels, op="voxel_reduce")
    B, N, C = x.shape
    n_voxels = _counts(n_voxels, B, "n_voxels", "voxel_reduce")
    out = torch.empty((B, int(M_max), C), dtype=torch.float32, device=x.device)
    ws = workspace(ws_bytes("gs_voxel_reduce_ws_bytes", B, int(M_max), C), x.device, "voxel_reduce")
    call("gs_voxel_reduce", ptr(x), ptr(counts), N, C, B, ptr(voxel_of), ptr(n_voxels), ptr(voxel_count), int(M_max),
         int(mode), ptr(out), ptr(ws), ws.numel(), stream())
    return out


def voxel_reduce_backward_raw(g_out, counts_i32, voxel_of, voxel_count, N, mode=VOXEL_MEAN):
    """Adjoint of voxel_reduce_raw: g_out (B,M_max,C) -> g_x (B,N,C), a gather (zero rows for padding and dropped points)."""
    g_out, counts = _voxel_rows(g_out, counts_i32, "voxel_reduce_backward")
    B, M_max, C = g_out.shape
    g_x = torch.empty((B, int(N), C), dtype=torch.float32, device=g_out.device)
    voxel_of, voxel_count = _voxel_index_args(g_x, voxel_of, voxel_count, M_max, "voxel_reduce_backward")
    call("gs_voxel_reduce_backward", ptr(g_out), ptr(counts), int(N), C, B, ptr(voxel_of), ptr(voxel_count), M_max, int(mode),
         ptr(g_x), stream())
    return g_x


class _VoxelReduceFn(torch.autograd.Function):
    """(x | counts, voxel_of, n_voxels, voxel_count: constants) -> per-voxel sum or mean.  The voxel of a point is a constant of
    the graph, like a nearest-neighbour index: the gradient is that of the sum / mean over fixed members."""

    @staticmethod
    def forward(ctx, x, counts, voxel_of, n_voxels, voxel_count, M_max, mode):
        out = voxel_reduce_raw(x, counts, voxel_of, n_voxels, voxel_count, M_max, mode)
        ctx.save_for_backward(counts, voxel_of, voxel_count)
        ctx.shape, ctx.dtype, ctx.mode = tuple(x.shape), x.dtype, mode
        return out

    @staticmethod
    def backward(ctx, g_out):
        counts, voxel_of, voxel_count = ctx.saved_tensors
        g_x = voxel_reduce_backward_raw(g_out, counts, voxel_of, voxel_count, ctx.shape[1], ctx.mode & VOXEL_MEAN)
        return g_x.view(ctx.shape).to(ctx.dtype), None, None, None, None, None, None


def voxel_reduce(x, counts_i32, voxel_of, n_voxels, voxel_count, M_max, mean=True):
    """Autograd-aware voxel_reduce_raw over the assignment of `voxel_assign`: (B,N,C) -> (B,M_max,C), gradients reach x.
    (Exact under voxel_reduce_raw's condition: all terms of the call within 102 - ceil(log2 N) binary places of its largest.)"""
    return _VoxelReduceFn.apply(x, counts_i32, voxel_of, n_voxels, voxel_count, int(M_max), VOXEL_MEAN if mean else VOXEL_SUM)


# ---------------------------------------------------------------------------------------------- N
KNN_KMAX = 32


def _knn_args(src, tgt, src_counts, tgt_counts, K, op):
    checked = _padded_pair(src, tgt, src_counts, tgt_counts, ("src", "tgt"), op)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= KNN_KMAX:
        raise ValueError("{}: K should be an int in [1, {}]. Got {!r}.".format(op, KNN_KMAX, K))
    return checked


def knn_raw(src, tgt, src_counts, tgt_counts, K: int, out=None) -> torch.Tensor:
    """Exact K nearest neighbours of every row of src (B,Ns,3) in tgt (B,Nt,3), padded clouds with int32 device counts ->
    keys (B,Ns,K) int64, every element written: slot k of a row below its count holds the k-th smallest (d2, j) packed as
    dist2_bits << 32 | j (d2 in fp32 without FMA, the lowest row wins ties); KEY_NONE beyond min(K, tgt_counts) and in the
    rows beyond src_counts.  `src is tgt` is the self-query.  `out`: a (B,Ns,K) int64 buffer to write into."""
    src, tgt, cs, ct = _knn_args(src, tgt, src_counts, tgt_counts, K, "knn")
    B, Ns, Nt = src.shape[0], src.shape[1], tgt.shape[1]
    keys = torch.empty((B, Ns, K), dtype=torch.int64, device=src.device) if out is None else out
    ws = workspace(ws_bytes("gs_knn_ws_bytes", B, Ns, Nt, K), src.device, "knn")
    call("gs_knn", ptr(src), ptr(cs), Ns, ptr(tgt), ptr(ct), Nt, B, K, ptr(keys), ptr(ws), ws.numel(), stream())
    return keys


def knn_unpack(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """keys int64 -> (d2 fp32, idx int64); KEY_NONE slots give d2 = 0, idx = -1."""
    none = keys == KEY_NONE
    d2 = (keys >> 32).to(torch.int32).view(torch.float32).masked_fill(none, 0.0)
    idx = (keys & 0xFFFFFFFF).masked_fill(none, -1)
    return d2, idx


def knn_backward_raw(src, tgt, src_counts, tgt_counts, keys, g_d2):
    """Adjoint of knn's distances: g_d2 (B,Ns,K) -> (g_src (B,Ns,3), g_tgt (B,Nt,3)), both fully written; the keys are constants.
    g_src is the fp32 sum in slot order, g_tgt the fold of gs_fixed128.hpp rounded once: one path, the same bits from run to
    run.  The fold is exact while all terms of the call lie within 102 - lg binary places of the call's largest (2^lg: the
    most terms one sum can have); what lies below that is truncated toward zero, term by term."""
    require_hip(keys, g_d2, op="knn_backward")
    if keys.ndim != 3 or keys.dtype != torch.int64:
        raise ValueError("knn_backward: keys should be (B, Ns, K) int64. Got {} of {}.".format(tuple(keys.shape), keys.dtype))
    K = int(keys.shape[-1])
    src, tgt, cs, ct = _knn_args(src, tgt, src_counts, tgt_counts, K, "knn_backward")
    B, Ns, Nt = src.shape[0], src.shape[1], tgt.shape[1]
    if tuple(keys.shape) != (B, Ns, K) or tuple(g_d2.shape) != (B, Ns, K):
        raise ValueError("knn_backward: keys and g_d2 should have shape {}. Got {} and {}.".format(
            (B, Ns, K), tuple(keys.shape), tuple(g_d2.shape)))
    keys, g_d2 = keys.contiguous(), _f32c(g_d2)
    g_src = torch.empty((B, Ns, 3), dtype=torch.float32, device=src.device)
    g_tgt = torch.empty((B, Nt, 3), dtype=torch.float32, device=src.device)
    ws = workspace(ws_bytes("gs_knn_backward_ws_bytes", B, Ns, Nt, K), src.device, "knn_bwd")
    call("gs_knn_backward", ptr(src), ptr(cs), Ns, ptr(tgt), ptr(ct), Nt, B, K, ptr(keys), ptr(g_d2), ptr(g_src), ptr(g_tgt),
         ptr(ws), ws.numel(), stream())
    return g_src, g_tgt


class _KnnFn(torch.autograd.Function):
    """(src, tgt | counts, K) -> (d2 (B,Ns,K) fp32, idx (B,Ns,K) int64: a constant).  The neighbours are constants of the graph,
    as in _ChamferFn: the gradient is that of the distances to them."""

    @staticmethod
    def forward(ctx, src, tgt, src_counts, tgt_counts, K, same):
        keys = knn_raw(src, src if same else tgt, src_counts, tgt_counts, K)
        d2, idx = knn_unpack(keys)
        ctx.save_for_backward(src, tgt, src_counts, tgt_counts, keys)
        ctx.same = same
        ctx.mark_non_differentiable(idx)
        return d2, idx

    @staticmethod
    def backward(ctx, g_d2, _g_idx):
        src, tgt, src_counts, tgt_counts, keys = ctx.saved_tensors
        g_src, g_tgt = knn_backward_raw(src, src if ctx.same else tgt, src_counts, tgt_counts, keys, g_d2)
        if ctx.same:  # one cloud: both roles' adjoints, added once
            return (g_src + g_tgt).view_as(src).to(src.dtype), None, None, None, None, None
        return (g_src.view_as(src).to(src.dtype) if ctx.needs_input_grad[0] else None,
                g_tgt.view_as(tgt).to(tgt.dtype) if ctx.needs_input_grad[1] else None, None, None, None, None)


def knn(src, tgt, src_counts, tgt_counts, K: int):
    """Autograd-aware knn_raw -> (d2 (B,Ns,K) fp32, idx (B,Ns,K) int64).  KEY_NONE slots give d2 = 0, idx = -1.  Gradients of
    d2 reach both clouds' points (for `src is tgt`, the cloud receives the sum of both roles)."""
    _knn_args(src, tgt, src_counts, tgt_counts, K, "knn")
    return _KnnFn.apply(src, tgt, src_counts, tgt_counts, K, src is tgt)


def knn_normals_raw(src, tgt, src_counts, tgt_counts, keys, mode: int = 0, orient=None, want_variation: bool = False):
    """Normals of the rows of src from the covariance of their neighbours in tgt (keys of knn_raw) -> (normals (B,Ns,3),
    variation (B,Ns) or None).  mode 0: unoriented; 1: orient (B,3) viewpoints, normals face them; 2: orient (B,Ns,3) reference
    normals, n . ref >= 0.  Rows with fewer than three neighbours and rows beyond the count: zeros.  Not differentiable."""
    require_hip(keys, orient, op="knn_normals")
    if keys.ndim != 3 or keys.dtype != torch.int64:
        raise ValueError("knn_normals: keys should be (B, Ns, K) int64. Got {} of {}.".format(tuple(keys.shape), keys.dtype))
    K = int(keys.shape[-1])
    src, tgt, cs, ct = _knn_args(src, tgt, src_counts, tgt_counts, K, "knn_normals")
    B, Ns, Nt = src.shape[0], src.shape[1], tgt.shape[1]
    if tuple(keys.shape) != (B, Ns, K):
        raise ValueError("knn_normals: keys should have shape {}. Got {}.".format((B, Ns, K), tuple(keys.shape)))
    if mode not in (0, 1, 2):
        raise ValueError("knn_normals: mode should be 0, 1 or 2. Got {!r}.".format(mode))
    if mode:
        want = (B, 3) if mode == 1 else (B, Ns, 3)
        if orient is None or tuple(orient.shape) != want:
            raise ValueError("knn_normals: mode {} needs orient of shape {}. Got {}.".format(
                mode, want, None if orient is None else tuple(orient.shape)))
        orient = _f32c(orient)
    else:
        orient = None
    keys = keys.contiguous()
    normals = torch.empty((B, Ns, 3), dtype=torch.float32, device=src.device)
    variation = torch.empty((B, Ns), dtype=torch.float32, device=src.device) if want_variation else None
    call("gs_knn_normals", ptr(src), ptr(cs), Ns, ptr(tgt), ptr(ct), Nt, B, K, ptr(keys), int(mode), ptr(orient), ptr(normals),
         ptr(variation), stream())
    return normals, variation


# ---------------------------------------------------------------------------------------------- T
TSDF_NMAX = 1 << 29  # voxels per batch element: edge ids 3 j + a are int32
TSDF_CHUNK = 32      # frames per integration launch


def _tsdf_on_device(op, *tensors):
    for t in tensors:
        if t is not None and not torch.is_tensor(t):
            raise TypeError("{}: expected a tensor; got {}".format(op, type(t)))
        if t is not None and not t.is_cuda:
            raise ValueError("{}: tensor is on {}; TSDF volumes only live on a HIP device (no CPU fallback is provided).".format(
                op, t.device))
    require_hip(*tensors, op=op)


def _tsdf_dims(dims, op):
    try:
        d = tuple(dims)
        ok = len(d) == 3 and all(isinstance(n, int) and not isinstance(n, bool) and n > 0 for n in d)
    except TypeError:
        d, ok = dims, False
    if not ok:
        raise ValueError("{}: dims should be three positive integers (nx, ny, nz). Got {!r}.".format(op, dims))
    if d[0] * d[1] * d[2] > TSDF_NMAX:
        raise ValueError("{}: at most 2^29 voxels per batch element are supported. Got dims {} = {} voxels.".format(
            op, d, d[0] * d[1] * d[2]))
    return d


def tsdf_origin(origin, B: int, device, op: str = "tsdf_origin") -> torch.Tensor:
    """The (B,3) fp32 device tensor the kernels read: `origin` given as three numbers or B rows of three (host values, checked
    to be finite, then uploaded), or a (B,3) / (3,) device tensor that is taken as it is (no host synchronisation)."""
    if torch.is_tensor(origin) and origin.is_cuda:
        o = _f32c(origin.detach())
        if o.shape == (3,):
            o = o.expand(B, 3).contiguous()
        if tuple(o.shape) != (B, 3):
            raise ValueError("{}: origin should have shape (3,) or ({}, 3). Got {}.".format(op, B, tuple(origin.shape)))
        return o
    try:
        o = torch.as_tensor(origin, dtype=torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("{}: origin should be three finite numbers, or one such row per batch element. Got {!r}.".format(op, origin))
    if o.shape == (3,):
        o = o.expand(B, 3)
    if tuple(o.shape) != (B, 3) or not bool(torch.isfinite(o).all()):
        raise ValueError("{}: origin should be finite, of shape (3,) or ({}, 3). Got {!r}.".format(op, B, origin))
    return o.contiguous().to(device)


def _tsdf_volume(tsdf, weight, op):
    """Checks the shapes of a volume's tsdf and weight (device tensors) -> (B, (nx, ny, nz))."""
    if tsdf.ndim != 4 or tsdf.shape[0] == 0 or tsdf.shape[0] > 65535:
        raise ValueError("{}: tsdf should have shape (B, nz, ny, nx) with 1 <= B <= 65535. Got {}.".format(op, tuple(tsdf.shape)))
    B, nz, ny, nx = (int(n) for n in tsdf.shape)
    dims = _tsdf_dims((nx, ny, nz), op)
    if weight.shape != tsdf.shape:
        raise ValueError("{}: weight should have the shape of tsdf {}. Got {}.".format(op, tuple(tsdf.shape), tuple(weight.shape)))
    return B, dims


def _tsdf_state(tsdf, weight, color, origin, voxel_size, op):
    """Checks one volume's tensors -> (tsdf, weight, color, origin (B,3), (nx, ny, nz), voxel_size)."""
    _tsdf_on_device(op, tsdf, weight, color)
    B, dims = _tsdf_volume(tsdf, weight, op)
    nx, ny, nz = dims
    if color is not None and tuple(color.shape) != (B, nz, ny, nx, 3):
        raise ValueError("{}: color should have shape {}. Got {}.".format(op, (B, nz, ny, nx, 3), tuple(color.shape)))
    v = _positive(voxel_size, "voxel_size", op)
    origin = tsdf_origin(origin, B, tsdf.device, op)
    _tsdf_on_device(op, origin)
    return _f32c(tsdf), _f32c(weight), _f32c(color), origin, dims, v


def _tsdf_frames(depth, rgb, K, poses, B, want_rgb, op):
    if poses is None:
        raise ValueError("{}: the frames need poses (camera-to-world, (B, L, 4, 4)).".format(op))
    _tsdf_on_device(op, depth, rgb, K, poses)
    if depth.ndim == 5 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if depth.ndim != 4 or depth.shape[0] != B or 0 in depth.shape:
        raise ValueError("{}: depth should have shape ({}, L, H, W[, 1]) with L, H, W > 0. Got {}.".format(op, B, tuple(depth.shape)))
    L, H, W = (int(n) for n in depth.shape[1:])
    if want_rgb and (rgb is None or tuple(rgb.shape) != (B, L, H, W, 3)):
        raise ValueError("{}: a volume with colours needs rgb of shape {}. Got {}.".format(
            op, (B, L, H, W, 3), None if rgb is None else tuple(rgb.shape)))
    if K.numel() != 16 * B or K.shape[-2:] != (4, 4):
        raise ValueError("{}: intrinsics should hold one 4x4 matrix per batch element (B = {}). Got {}.".format(op, B, tuple(K.shape)))
    if tuple(poses.shape) != (B, L, 4, 4):
        raise ValueError("{}: poses should have shape {}. Got {}.".format(op, (B, L, 4, 4), tuple(poses.shape)))
    return _f32c(depth), (_f32c(rgb) if want_rgb else None), _f32c(K), _f32c(poses), L, H, W


def tsdf_integrate_raw(depth, rgb, K, poses, tsdf, weight, color, origin, voxel_size, trunc, max_weight, inplace: bool = False):
    """Fuse the frames depth (B,L,H,W[,1]) / rgb (B,L,H,W,3) with intrinsics K (B,1,4,4) and camera-to-world poses (B,L,4,4) into
    the volume tsdf / weight (B,nz,ny,nx), color (B,nz,ny,nx,3) or None -> the new (tsdf, weight, color).  Per voxel the frames
    are applied in order (the rule: include/gradslam_hip.h, T); one launch per 32 frames; the result is what L single-frame calls
    give, bit for bit.  `inplace` writes into the given tensors (which must then be contiguous fp32).  origin: see tsdf_origin."""
    op = "tsdf_integrate"
    if poses is None:
        raise ValueError("{}: the frames need poses (camera-to-world, (B, L, 4, 4)).".format(op))
    t_in, w_in, c_in, origin, (nx, ny, nz), v = _tsdf_state(tsdf, weight, color, origin, voxel_size, op)
    B = t_in.shape[0]
    depth, rgb, K, poses, L, H, W = _tsdf_frames(depth, rgb, K, poses, B, c_in is not None, op)
    trunc, max_weight = _positive(trunc, "trunc", op), _positive(max_weight, "max_weight", op)
    if inplace:
        if any(a is not b for a, b in ((t_in, tsdf), (w_in, weight), (c_in, color))):
            raise ValueError("{}: inplace needs contiguous float32 state tensors.".format(op))
        t_out, w_out, c_out = t_in, w_in, c_in
    else:
        t_out, w_out = torch.empty_like(t_in), torch.empty_like(w_in)
        c_out = None if c_in is None else torch.empty_like(c_in)
    call("gs_tsdf_integrate", ptr(depth), ptr(rgb), ptr(K), ptr(poses), B, L, H, W, nx, ny, nz, v, ptr(origin), trunc, max_weight,
         ptr(t_in), ptr(w_in), ptr(c_in), ptr(t_out), ptr(w_out), ptr(c_out), stream())
    return t_out, w_out, c_out


def _tsdf_integrate_backward(op, with_poses, want_state, want_frames, depth, K, poses, weight, origin, voxel_size, trunc, max_weight,
                             g_tsdf, g_color):
    """The body of tsdf_integrate_backward_raw (op "tsdf_integrate_backward": gs_<op> with its own size query and workspace) and
    of tsdf_integrate_backward_poses_raw -> (g_tsdf_in, g_color_in, g_depth, g_rgb, g_poses or None)."""
    g_t, w_in, g_c, origin, (nx, ny, nz), v = _tsdf_state(g_tsdf, weight, g_color, origin, voxel_size, op)
    B = g_t.shape[0]
    depth, _, K, poses, L, H, W = _tsdf_frames(depth, None, K, poses, B, False, op)
    trunc, max_weight = _positive(trunc, "trunc", op), _positive(max_weight, "max_weight", op)
    dev = g_t.device
    o_t = torch.empty_like(g_t) if want_state else None
    o_c = torch.empty_like(g_c) if want_state and g_c is not None else None
    g_depth = torch.empty((B, L, H, W), dtype=torch.float32, device=dev) if want_frames else None
    g_rgb = torch.empty((B, L, H, W, 3), dtype=torch.float32, device=dev) if want_frames and g_c is not None else None
    g_poses = torch.empty((B, L, 4, 4), dtype=torch.float32, device=dev) if with_poses else None
    size_args = (B, L, H, W, nx, ny, nz, int(g_c is not None)) if with_poses else (B, L, H, W)
    ws = workspace(ws_bytes("gs_{}_ws_bytes".format(op), *size_args), dev, "tsdf_bwd_poses" if with_poses else "tsdf_bwd")
    call("gs_" + op, ptr(depth), ptr(K), ptr(poses), B, L, H, W, nx, ny, nz, v, ptr(origin), trunc, max_weight, ptr(w_in), ptr(g_t),
         ptr(g_c), ptr(o_t), ptr(o_c), ptr(g_depth), ptr(g_rgb), *((ptr(g_poses),) if with_poses else ()), ptr(ws), ws.numel(), stream())
    return o_t, o_c, g_depth, g_rgb, g_poses


def tsdf_integrate_backward_raw(depth, K, poses, weight, origin, voxel_size, trunc, max_weight, g_tsdf, g_color=None):
    """Adjoint of tsdf_integrate_raw: the adjoints g_tsdf (B,nz,ny,nx) / g_color (B,nz,ny,nx,3 or None) of the new state ->
    (g_tsdf_in, g_color_in, g_depth (B,L,H,W), g_rgb (B,L,H,W,3)); `weight` is the weight BEFORE the integration.  The pixel sums
    are the fold of gs_fixed128.hpp, rounded once: the same bits from run to run (one path, with or without
    torch.use_deterministic_algorithms); exact while all terms of the call lie within 102 - lg binary places of the call's
    largest (2^lg: the most terms one sum can have), truncated toward zero below that."""
    return _tsdf_integrate_backward("tsdf_integrate_backward", False, True, True, depth, K, poses, weight, origin, voxel_size, trunc,
                                    max_weight, g_tsdf, g_color)[:4]


def tsdf_integrate_backward_poses_raw(depth, K, poses, weight, origin, voxel_size, trunc, max_weight, g_tsdf, g_color=None,
                                      want_state: bool = True, want_frames: bool = True):
    """tsdf_integrate_backward_raw with the adjoint of the poses: -> (g_tsdf_in, g_color_in, g_depth, g_rgb, g_poses (B,L,4,4)).
    The first four are tsdf_integrate_backward_raw's, bit for bit; `want_state=False` / `want_frames=False` leave (g_tsdf_in,
    g_color_in) / (g_depth, g_rgb) out (None) and drop their share of the work.  g_poses is the adjoint of the unconstrained
    matrix entries (render_map's convention; row 3 is zero): the update depends on a pose through the camera-frame depth of the
    voxel centres alone, with the pixel of a voxel, the three skips, the t = 1 branch and the weight cap held constant.  Fixed
    order fp32 sums, no atomics: the same bits from run to run.  Intrinsics, weights and origin receive no gradient."""
    return _tsdf_integrate_backward("tsdf_integrate_backward_poses", True, want_state, want_frames, depth, K, poses, weight, origin,
                                    voxel_size, trunc, max_weight, g_tsdf, g_color)


class _TsdfIntegrateFn(torch.autograd.Function):
    """(depth, rgb, tsdf, color, poses | weight, K, origin: constants) -> (tsdf', color', weight').  The pixel of a voxel, the three
    skips, the t = 1 branch and the weight cap are constants of the graph; weight, intrinsics and origin receive None.  The poses
    receive their adjoint when they require one (tsdf_integrate_backward_poses_raw); otherwise the reverse pass is
    tsdf_integrate_backward_raw's, as it was."""

    @staticmethod
    def forward(ctx, depth, rgb, tsdf, color, weight, K, poses, origin, voxel_size, trunc, max_weight):
        t, w, c = tsdf_integrate_raw(depth, rgb, K, poses, tsdf, weight, color, origin, voxel_size, trunc, max_weight)
        ctx.save_for_backward(depth, K, poses, weight, origin)
        ctx.cfg = (voxel_size, trunc, max_weight)
        ctx.depth_shape, ctx.has_color = tuple(depth.shape), color is not None
        ctx.mark_non_differentiable(w)
        return t, c, w

    @staticmethod
    def backward(ctx, g_t, g_c, _g_w):
        depth, K, poses, weight, origin = ctx.saved_tensors
        if g_t is None:
            g_t = torch.zeros_like(weight)
        if ctx.has_color and g_c is None:
            g_c = torch.zeros(tuple(weight.shape) + (3,), dtype=torch.float32, device=weight.device)
        need = ctx.needs_input_grad
        g_c = g_c if ctx.has_color else None
        g_poses = None
        if need[6]:
            o_t, o_c, g_depth, g_rgb, g_poses = tsdf_integrate_backward_poses_raw(
                depth, K, poses, weight, origin, *ctx.cfg, g_t, g_c, want_state=need[2] or need[3], want_frames=need[0] or need[1])
            g_poses = g_poses.view(poses.shape).to(poses.dtype)
        else:
            o_t, o_c, g_depth, g_rgb = tsdf_integrate_backward_raw(depth, K, poses, weight, origin, *ctx.cfg, g_t, g_c)
        return (g_depth.view(ctx.depth_shape) if need[0] else None, g_rgb if need[1] else None, o_t if need[2] else None,
                o_c if need[3] else None, None, None, g_poses, None, None, None, None)


def tsdf_integrate(depth, rgb, K, poses, tsdf, weight, color, origin, voxel_size, trunc, max_weight):
    """Autograd-aware tsdf_integrate_raw -> (tsdf, weight, color): gradients reach the old tsdf / color, depth, rgb and the poses
    (the adjoint of the unconstrained matrix entries; computed only when the poses require it).  Intrinsics, weights and origin
    are not differentiable."""
    origin = tsdf_origin(origin, tsdf.shape[0], tsdf.device, "tsdf_integrate") if torch.is_tensor(tsdf) and tsdf.ndim == 4 else origin
    t, c, w = _TsdfIntegrateFn.apply(depth, rgb, tsdf, color, weight, K, poses, origin, voxel_size, trunc, max_weight)
    return t, w, c


def tsdf_extract_raw(tsdf, weight, color, origin, voxel_size, min_weight: float = 1.0, cap: int = 0):
    """The surface points of a volume: one per grid edge whose ends are observed (weight >= min_weight) and differ in the sign of
    tsdf -> (points, normals, colors (B,cap,3), edge (B,cap) int32, n_points (B,) int32).  Rows come in ascending edge id
    e = 3 j + axis; the first min(n_points, cap) rows are written (the others hold zeros, edge -1), n_points is the full count.
    cap = 0 only counts (the arrays are None): size with it first.  colors is None for a volume without colours."""
    op = "tsdf_extract"
    t, w, c, origin, (nx, ny, nz), v = _tsdf_state(tsdf, weight, color, origin, voxel_size, op)
    mw = _number(min_weight, "min_weight", op)
    cap = int(cap)
    if cap < 0 or cap > 3 * TSDF_NMAX:
        raise ValueError("{}: cap should lie in 0 .. 3 * 2^29. Got {}.".format(op, cap))
    B, dev = t.shape[0], t.device
    n_points = torch.empty((B,), dtype=torch.int32, device=dev)
    rows = lambda have: torch.zeros((B, cap, 3), dtype=torch.float32, device=dev) if (have and cap) else None
    points, normals, colors = rows(True), rows(True), rows(c is not None)
    edge = torch.full((B, cap), -1, dtype=torch.int32, device=dev) if cap else None
    ws = workspace(ws_bytes("gs_tsdf_extract_ws_bytes", B, nx, ny, nz), dev, "tsdf_extract")
    call("gs_tsdf_extract", ptr(t), ptr(w), ptr(c), B, nx, ny, nz, v, ptr(origin), mw, cap, ptr(points), ptr(normals), ptr(colors),
         ptr(edge), ptr(n_points), ptr(ws), ws.numel(), stream())
    return points, normals, colors, edge, n_points


def tsdf_extract_backward_raw(tsdf, color, voxel_size, edge, n_points, g_points=None, g_colors=None):
    """Adjoint of tsdf_extract_raw for the rows in edge / n_points (constants): -> (g_tsdf, g_color or None), written in full.
    No float atomics, a fixed order of addition: bit-reproducible."""
    op = "tsdf_extract_backward"
    _tsdf_on_device(op, tsdf, color, edge, n_points, g_points, g_colors)
    if tsdf.ndim != 4:
        raise ValueError("{}: tsdf should have shape (B, nz, ny, nx). Got {}.".format(op, tuple(tsdf.shape)))
    B, nz, ny, nx = (int(n) for n in tsdf.shape)
    _tsdf_dims((nx, ny, nz), op)
    v = _positive(voxel_size, "voxel_size", op)
    if edge.dtype != torch.int32 or edge.ndim != 2 or edge.shape[0] != B or edge.shape[1] == 0:
        raise ValueError("{}: edge should be int32 of shape ({}, cap) with cap > 0. Got {} of {}.".format(op, B, tuple(edge.shape), edge.dtype))
    cap = int(edge.shape[1])
    n_points = _counts(n_points, B, "n_points", op)
    for name, g in (("g_points", g_points), ("g_colors", g_colors)):
        if g is not None and tuple(g.shape) != (B, cap, 3):
            raise ValueError("{}: {} should have shape {}. Got {}.".format(op, name, (B, cap, 3), tuple(g.shape)))
    t, c = _f32c(tsdf), _f32c(color)
    g_tsdf = torch.empty_like(t)
    g_color = None if c is None else torch.empty_like(c)
    call("gs_tsdf_extract_backward", ptr(t), ptr(c), B, nx, ny, nz, v, ptr(edge.contiguous()), ptr(n_points), cap,
         ptr(_f32c(g_points)), ptr(_f32c(g_colors)), ptr(g_tsdf), ptr(g_color), stream())
    return g_tsdf, g_color


class _TsdfExtractFn(torch.autograd.Function):
    """(tsdf, color | weight, origin: constants) -> (points, normals, colors, edge, n_points).  Which edges cross is a constant of
    the graph; normals carry no gradient (like knn_normals)."""

    @staticmethod
    def forward(ctx, tsdf, color, weight, origin, voxel_size, min_weight, cap):
        points, normals, colors, edge, n_points = tsdf_extract_raw(tsdf, weight, color, origin, voxel_size, min_weight, cap)
        ctx.save_for_backward(tsdf, color, edge, n_points)
        ctx.voxel_size = voxel_size
        ctx.mark_non_differentiable(normals, edge, n_points)
        return points, normals, colors, edge, n_points

    @staticmethod
    def backward(ctx, g_points, _g_normals, g_colors, _g_edge, _g_n):
        tsdf, color, edge, n_points = ctx.saved_tensors
        g_tsdf, g_color = tsdf_extract_backward_raw(tsdf, color, ctx.voxel_size, edge, n_points, g_points, g_colors)
        return (g_tsdf if ctx.needs_input_grad[0] else None, g_color if ctx.needs_input_grad[1] else None, None, None, None, None, None)


def tsdf_extract(tsdf, weight, color, origin, voxel_size, min_weight: float = 1.0, cap: int = 0):
    """Autograd-aware tsdf_extract_raw (cap > 0): gradients of points and colors reach tsdf and color."""
    if int(cap) <= 0:
        raise ValueError("tsdf_extract: cap should be positive (size it with tsdf_extract_raw(..., cap=0)). Got {}.".format(cap))
    if torch.is_tensor(tsdf) and tsdf.ndim == 4:
        origin = tsdf_origin(origin, tsdf.shape[0], tsdf.device, "tsdf_extract")
    return _TsdfExtractFn.apply(tsdf, color, weight, origin, voxel_size, min_weight, int(cap))


MESH_NMAX = 1 << 28  # voxels per batch element of a meshed volume: face counts are int32, 5 per cube


def tsdf_faces_raw(tsdf, weight, min_weight, edge, n_points, fcap: int = 0, points_fit: bool = False):
    """The triangles of a volume's surface over the rows of tsdf_extract_raw (marching cubes; the case table is generated by
    tools/gen_mc_table.py) -> (faces (B,fcap,3) int32, n_faces (B,) int32).  A cube of 8 voxels emits iff all its corners are
    observed (weight >= min_weight); faces come in ascending cube id, then table order, counter-clockwise seen from free space,
    and index the rows of `edge` (B,vcap) / `n_points` (B,) -- the edge list and count tsdf_extract_raw returned for the same
    volume and min_weight.  The first min(n_faces, fcap) rows are written, the others hold -1; n_faces is the full count.
    fcap = 0 only counts (faces is None; edge and n_points may be None): size with it first.  A truncated edge list
    (vcap < n_points) is refused: the counts are read back for that (one host synchronisation) unless the caller, who sized
    vcap from them, passes points_fit=True.  Integers only: no autograd node."""
    op = "tsdf_faces"
    _tsdf_on_device(op, tsdf, weight, edge, n_points)
    B, (nx, ny, nz) = _tsdf_volume(tsdf, weight, op)
    if nx * ny * nz > MESH_NMAX:
        raise ValueError("{}: at most 2^28 voxels per batch element can be meshed. Got dims {} = {} voxels.".format(
            op, (nx, ny, nz), nx * ny * nz))
    mw = _number(min_weight, "min_weight", op)
    fcap = int(fcap)
    if fcap < 0 or fcap > 5 * MESH_NMAX:
        raise ValueError("{}: fcap should lie in 0 .. 5 * 2^28. Got {}.".format(op, fcap))
    vcap = 0
    if fcap:
        if edge is None or n_points is None:
            raise ValueError("{}: fcap = {} rows need the edge list and n_points of tsdf_extract_raw.".format(op, fcap))
        if edge.dtype != torch.int32 or edge.ndim != 2 or edge.shape[0] != B:
            raise ValueError("{}: edge should be int32 of shape ({}, vcap). Got {} of {}.".format(op, B, tuple(edge.shape), edge.dtype))
        n_points = _counts(n_points, B, "n_points", op)
        vcap = int(edge.shape[1])
        if not points_fit and int(n_points.max()) > vcap:
            raise ValueError("{}: the edge list is truncated: it holds {} rows per batch element, n_points is up to {}.".format(
                op, vcap, int(n_points.max())))
        edge = edge.contiguous()
    t, w = _f32c(tsdf.detach()), _f32c(weight.detach())
    dev = t.device
    n_faces = torch.empty((B,), dtype=torch.int32, device=dev)
    faces = torch.empty((B, fcap, 3), dtype=torch.int32, device=dev) if fcap else None
    ws = workspace(ws_bytes("gs_tsdf_faces_ws_bytes", B, nx, ny, nz), dev, "tsdf_faces")
    call("gs_tsdf_faces", ptr(t), ptr(w), B, nx, ny, nz, mw, ptr(edge) if (fcap and vcap) else None, ptr(n_points) if fcap else None, vcap,
         fcap, ptr(faces), ptr(n_faces), ptr(ws), ws.numel(), stream())
    return faces, n_faces


def _tsdf_cast(K, poses, B, dims, v, height, width, stride, step, min_weight, op):
    """Checks the cameras and the sampling of a cast -> (K, poses, L, height, width, stride, step, min_weight)."""
    if poses is None:
        raise ValueError("{}: the cameras need poses (camera-to-world, (B, L, 4, 4)).".format(op))
    _tsdf_on_device(op, K, poses)
    if K.numel() != 16 * B or K.shape[-2:] != (4, 4):
        raise ValueError("{}: intrinsics should hold one 4x4 matrix per batch element (B = {}). Got {}.".format(op, B, tuple(K.shape)))
    if poses.ndim != 4 or poses.shape[0] != B or poses.shape[1] == 0 or poses.shape[1] > 65535 or poses.shape[2:] != (4, 4):
        raise ValueError("{}: poses should have shape ({}, L, 4, 4) with 1 <= L <= 65535. Got {}.".format(op, B, tuple(poses.shape)))
    for name, n in (("height", height), ("width", width), ("stride", stride)):
        if not isinstance(n, int) or isinstance(n, bool) or n < 1:
            raise ValueError("{}: {} should be a positive integer. Got {!r}.".format(op, name, n))
    if height * width > 2 ** 31 - 1:
        raise ValueError("{}: at most 2^31 - 1 pixels per image are supported. Got {} x {}.".format(op, height, width))
    if -(-height // (16 * stride)) * -(-width // (16 * stride)) > 2 ** 22:
        raise ValueError("{}: at most 2^22 tiles of 16 x 16 output pixels per image are supported. Got {} x {} at stride {}.".format(
            op, height, width, stride))
    step = _positive(step, "step", op)
    if sum(dims) * v / step > 2 ** 20:
        raise ValueError("{}: (nx + ny + nz) voxel_size / step should be at most 2^20 samples per ray. Got {:g}.".format(
            op, sum(dims) * v / step))
    return _f32c(K), _f32c(poses), int(poses.shape[1]), height, width, stride, step, _number(min_weight, "min_weight", op)


def tsdf_raycast_raw(tsdf, weight, color, origin, voxel_size, K, poses, height: int, width: int, stride: int, step: float,
                     near: float = 0.0, far: float = float("inf"), min_weight: float = 1.0):
    """Cast the volume into the cameras K (B,1,4,4), poses (B,L,4,4) of height x width images, on the [::stride, ::stride] pixel
    grid -> (depth (B,L,Ho,Wo), normal (B,L,Ho,Wo,3), rgb (B,L,Ho,Wo,3) or None without colours, k_end (B,L,Ho,Wo) int32).  The
    rule (ray, sample, march, hit) is stated in include/gradslam_hip.h, T; `stride` and `step` are required here
    (TSDFVolume.raycast defaults them to 1 and trunc / 2).  Misses hold zeros; k_end is the tape of tsdf_raycast_backward_raw.  One launch, no host synchronisation."""
    op = "tsdf_raycast"
    t, w, c, origin, dims, v = _tsdf_state(tsdf, weight, color, origin, voxel_size, op)
    B, dev = t.shape[0], t.device
    K, poses, L, height, width, stride, step, mw = _tsdf_cast(K, poses, B, dims, v, height, width, stride, step, min_weight, op)
    near, far = _number(near, "near", op), _number(far, "far", op)
    if near < 0.0:
        raise ValueError("{}: near should not be negative. Got {!r}.".format(op, near))
    Ho, Wo = -(-height // stride), -(-width // stride)
    depth = torch.empty((B, L, Ho, Wo), dtype=torch.float32, device=dev)
    normal = torch.empty((B, L, Ho, Wo, 3), dtype=torch.float32, device=dev)
    rgb = None if c is None else torch.empty((B, L, Ho, Wo, 3), dtype=torch.float32, device=dev)
    k_end = torch.empty((B, L, Ho, Wo), dtype=torch.int32, device=dev)
    call("gs_tsdf_raycast", ptr(t), ptr(w), ptr(c), B, *dims, v, ptr(origin), ptr(K), ptr(poses), L, height, width, stride, step, near,
         far, mw, ptr(depth), ptr(normal), ptr(rgb), ptr(k_end), stream())
    return depth, normal, rgb, k_end


def _tsdf_raycast_backward(op, with_poses, want_volume, tsdf, weight, color, origin, voxel_size, K, poses, height, width, stride, step,
                           min_weight, k_end, g_depth, g_rgb):
    """The body of tsdf_raycast_backward_raw (op "tsdf_raycast_backward": gs_<op> with its own size query and workspace) and of
    tsdf_raycast_backward_poses_raw -> (g_tsdf, g_color, g_poses or None)."""
    t, w, c, origin, dims, v = _tsdf_state(tsdf, weight, color, origin, voxel_size, op)
    B, dev = t.shape[0], t.device
    K, poses, L, height, width, stride, step, mw = _tsdf_cast(K, poses, B, dims, v, height, width, stride, step, min_weight, op)
    Ho, Wo = -(-height // stride), -(-width // stride)
    _tsdf_on_device(op, k_end, g_depth, g_rgb)
    if k_end.dtype != torch.int32 or tuple(k_end.shape) != (B, L, Ho, Wo):
        raise ValueError("{}: k_end should be int32 of shape {}. Got {} of {}.".format(op, (B, L, Ho, Wo), tuple(k_end.shape), k_end.dtype))
    if g_depth is not None and g_depth.ndim == 5 and g_depth.shape[-1] == 1:
        g_depth = g_depth[..., 0]
    if g_depth is not None and tuple(g_depth.shape) != (B, L, Ho, Wo):
        raise ValueError("{}: g_depth should have shape {}. Got {}.".format(op, (B, L, Ho, Wo), tuple(g_depth.shape)))
    if g_rgb is not None and (c is None or tuple(g_rgb.shape) != (B, L, Ho, Wo, 3)):
        raise ValueError("{}: g_rgb needs a volume with colours and the shape {}. Got {}.".format(op, (B, L, Ho, Wo, 3), tuple(g_rgb.shape)))
    k_end, g_depth, g_rgb = k_end.contiguous(), _f32c(g_depth), _f32c(g_rgb)
    g_tsdf = torch.empty_like(t) if want_volume else None
    g_color = torch.empty_like(c) if want_volume and c is not None else None
    g_poses = torch.empty((B, L, 4, 4), dtype=torch.float32, device=dev) if with_poses else None
    size_args = (B, *dims, int(c is not None)) + ((L, height, width, stride) if with_poses else ())
    ws = workspace(ws_bytes("gs_{}_ws_bytes".format(op), *size_args), dev, "tsdf_cast_bwd_poses" if with_poses else "tsdf_cast_bwd")
    call("gs_" + op, ptr(t), ptr(w), ptr(c), B, *dims, v, ptr(origin), ptr(K), ptr(poses), L, height, width, stride, step, mw, ptr(k_end),
         ptr(g_depth), ptr(g_rgb), ptr(g_tsdf), ptr(g_color), *((ptr(g_poses),) if with_poses else ()), ptr(ws), ws.numel(), stream())
    return g_tsdf, g_color, g_poses


def tsdf_raycast_backward_raw(tsdf, weight, color, origin, voxel_size, K, poses, height: int, width: int, stride, step, min_weight,
                              k_end, g_depth=None, g_rgb=None):
    """Adjoint of tsdf_raycast_raw for the tape k_end (a constant): g_depth (B,L,Ho,Wo), g_rgb (B,L,Ho,Wo,3) (None: zero) ->
    (g_tsdf, g_color or None), written in full.  Every voxel's sum over its pixels is the fold of gs_fixed128.hpp, rounded once:
    the same bits from run to run (one path, with or without torch.use_deterministic_algorithms); exact while all terms of the
    call lie within 102 - lg binary places of the call's largest (2^lg: the most terms one sum can have), truncated toward zero
    below that.  Poses, intrinsics and weights get no gradient."""
    return _tsdf_raycast_backward("tsdf_raycast_backward", False, True, tsdf, weight, color, origin, voxel_size, K, poses, height, width,
                                  stride, step, min_weight, k_end, g_depth, g_rgb)[:2]


def tsdf_raycast_backward_poses_raw(tsdf, weight, color, origin, voxel_size, K, poses, height: int, width: int, stride, step, min_weight,
                                    k_end, g_depth=None, g_rgb=None, want_volume: bool = True):
    """tsdf_raycast_backward_raw with the adjoint of the poses: -> (g_tsdf, g_color or None, g_poses (B,L,4,4)).  The first two are
    tsdf_raycast_backward_raw's, bit for bit; `want_volume=False` leaves them out (None) and drops their share of the work.
    g_poses is the adjoint of the unconstrained matrix entries (render_map's convention; row 3 is zero; zeros for a camera
    without hits), with which sample ends a ray, whether it hits and the cells of its three positions held constant.  Fixed
    order fp32 sums, no atomics: the same bits from run to run.  Intrinsics, weights, origin and the normal image receive no
    gradient."""
    return _tsdf_raycast_backward("tsdf_raycast_backward_poses", True, want_volume, tsdf, weight, color, origin, voxel_size, K, poses,
                                  height, width, stride, step, min_weight, k_end, g_depth, g_rgb)


class _TsdfRaycastFn(torch.autograd.Function):
    """(tsdf, color, poses | weight, origin, K: constants) -> (depth, normal, rgb, k_end).  Which sample ends a ray and whether it
    hits are constants of the graph; normals carry no gradient; intrinsics, weights and origin receive None.  The poses receive
    their adjoint when they require one (tsdf_raycast_backward_poses_raw); otherwise the reverse pass is
    tsdf_raycast_backward_raw's, as it was."""

    @staticmethod
    def forward(ctx, tsdf, color, weight, origin, voxel_size, K, poses, height, width, stride, step, near, far, min_weight):
        depth, normal, rgb, k_end = tsdf_raycast_raw(tsdf, weight, color, origin, voxel_size, K, poses, height, width, stride, step, near,
                                                     far, min_weight)
        ctx.save_for_backward(tsdf, color, weight, origin, K, poses, k_end)
        ctx.cfg = (voxel_size, height, width, stride, step, min_weight)
        ctx.mark_non_differentiable(normal, k_end)
        return depth, normal, rgb, k_end

    @staticmethod
    def backward(ctx, g_depth, _g_normal, g_rgb, _g_k):
        tsdf, color, weight, origin, K, poses, k_end = ctx.saved_tensors
        voxel_size, height, width, stride, step, min_weight = ctx.cfg
        need = ctx.needs_input_grad
        g_rgb = g_rgb if color is not None else None
        g_poses = None
        if need[6]:
            g_tsdf, g_color, g_poses = tsdf_raycast_backward_poses_raw(tsdf, weight, color, origin, voxel_size, K, poses, height, width,
                                                                       stride, step, min_weight, k_end, g_depth, g_rgb,
                                                                       want_volume=need[0] or need[1])
            g_poses = g_poses.view(poses.shape).to(poses.dtype)
        else:
            g_tsdf, g_color = tsdf_raycast_backward_raw(tsdf, weight, color, origin, voxel_size, K, poses, height, width, stride, step,
                                                        min_weight, k_end, g_depth, g_rgb)
        return (g_tsdf if need[0] else None, g_color if need[1] else None, None, None, None, None, g_poses) + (None,) * 7


def tsdf_raycast(tsdf, weight, color, origin, voxel_size, K, poses, height: int, width: int, stride: int, step: float,
                 near: float = 0.0, far: float = float("inf"), min_weight: float = 1.0):
    """Autograd-aware tsdf_raycast_raw, one node: gradients of depth and rgb reach tsdf, color and the poses (the adjoint of the
    unconstrained matrix entries; computed only when the poses require it).  Intrinsics, weights, origin and the normal image are
    not differentiable."""
    if torch.is_tensor(tsdf) and tsdf.ndim == 4:
        origin = tsdf_origin(origin, tsdf.shape[0], tsdf.device, "tsdf_raycast")
    return _TsdfRaycastFn.apply(tsdf, color, weight, origin, voxel_size, K, poses, height, width, stride, step, near, far, min_weight)


# ------------------------------------------------------------------ dense RGB-D odometry (csrc/rgbd.hip)
def _rgbd_frame(depth, rgb, which, op, B=None, H=None, W=None, attached=False):
    """depth (B,H,W) or (B,H,W,1), rgb (B,H,W,3) -> contiguous fp32 (B,H,W), (B,H,W,3); detached unless `attached`."""
    for name, t in (("depth", depth), ("rgb", rgb)):
        if not torch.is_tensor(t):
            raise TypeError("{}: expected {}_{} to be a tensor; got {}".format(op, which, name, type(t)))
    if depth.ndim == 4 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if depth.ndim != 3:
        raise ValueError("{}: {}_depth should have shape (B, H, W) or (B, H, W, 1). Got {}.".format(op, which, tuple(depth.shape)))
    if tuple(rgb.shape) != tuple(depth.shape) + (3,):
        raise ValueError("{}: {}_rgb should have shape {}. Got {}.".format(op, which, tuple(depth.shape) + (3,), tuple(rgb.shape)))
    if B is not None and tuple(depth.shape) != (B, H, W):
        raise ValueError("{}: both frames should have the same batch size and image size ({} != {}).".format(
            op, tuple(depth.shape), (B, H, W)))
    if attached:
        return depth.float().contiguous(), rgb.float().contiguous()
    return _f32c(depth.detach()), _f32c(rgb.detach())


def _rgbd_K(K, B, op):
    if not torch.is_tensor(K):
        raise TypeError("{}: expected intrinsics to be a tensor; got {}".format(op, type(K)))
    if K.numel() != B * 16:
        raise ValueError("{}: intrinsics should have shape ({}, 4, 4) or ({}, 1, 4, 4). Got {}.".format(op, B, B, tuple(K.shape)))
    return _f32c(K.detach().reshape(B, 4, 4))


def _rgbd_T(T, B, name, op, attached=False):
    if not torch.is_tensor(T):
        raise TypeError("{}: expected {} to be a tensor; got {}".format(op, name, type(T)))
    if T.numel() != B * 16 or tuple(T.shape[-2:]) != (4, 4):
        raise ValueError("{}: {} should have shape ({}, 4, 4) or ({}, 1, 4, 4). Got {}.".format(op, name, B, B, tuple(T.shape)))
    if attached:
        return T.reshape(B, 16).float().contiguous()
    return _f32c(T.detach().reshape(B, 16))


def _gn_levels(levels, op):
    """The level count of the two image-aligned odometries (rgbd_*, sdf_*): an integer in [1, 8]."""
    if not isinstance(levels, int) or isinstance(levels, bool) or levels < 1 or levels > 8:
        raise ValueError("{}: levels should be an integer in [1, 8]. Got {!r}.".format(op, levels))


def _gn_loop(numiters, levels, damp, op):
    """The loop's parameters, checked -> (numiters as `levels` counts, finest first (an int: that count at every level), damp)."""
    damp = _number(damp, "damp", op)
    if not (0.0 <= damp < math.inf):
        raise ValueError("{}: damp should be finite and not negative. Got {!r}.".format(op, damp))
    if isinstance(numiters, int) and not isinstance(numiters, bool):
        numiters = (numiters,) * levels
    numiters = tuple(numiters)
    if len(numiters) != levels or any(not isinstance(n, int) or isinstance(n, bool) or n < 0 for n in numiters):
        raise ValueError("{}: numiters should be {} non-negative integers (finest level first). Got {!r}.".format(op, levels, numiters))
    return numiters, damp


def _gn_outputs(B, numiters, dev):
    """What a loop's C call fills and takes: (out_T (B,4,4), info (B,levels,4), the levels' counts as a C int array)."""
    out_T = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    info = torch.empty((B, len(numiters), 4), dtype=torch.float32, device=dev)
    return out_T, info, (nv.c_i * len(numiters))(*numiters)


def _rgbd_params(levels, lambda_geo, depth_diff_max, rgb_scale, H, W, op):
    _gn_levels(levels, op)
    if (H >> (levels - 1)) < 4 or (W >> (levels - 1)) < 4:
        raise ValueError("{}: the coarsest of {} levels of a {} x {} image would be smaller than 4 x 4.".format(op, levels, H, W))
    lam, ddm, scale = (_number(x, n, op) for x, n in ((lambda_geo, "lambda_geo"), (depth_diff_max, "depth_diff_max"),
                                                           (rgb_scale, "rgb_scale")))
    if not 0.0 <= lam <= 1.0:
        raise ValueError("{}: lambda_geo should be in [0, 1]. Got {!r}.".format(op, lambda_geo))
    if not (0.0 < ddm < math.inf):
        raise ValueError("{}: depth_diff_max should be finite and positive. Got {!r}.".format(op, depth_diff_max))
    if not math.isfinite(scale):
        raise ValueError("{}: rgb_scale should be finite. Got {!r}.".format(op, rgb_scale))
    return lam, ddm, scale


def rgbd_level_sizes(H: int, W: int, levels: int):
    """[(H_l, W_l)] of the pyramid: every level halves the one before, rounding down."""
    return [(H >> l, W >> l) for l in range(levels)]


def rgbd_pyramid_raw(depth, rgb, levels: int, depth_diff_max: float = 0.07, rgb_scale: float = 1.0 / 255.0):
    """The (intensity, depth) pyramid of one frame, the rule of include/gradslam_hip.h: a list of `levels` tensors (B, H_l, W_l, 2),
    views of one allocation.  Depth 0 = not valid."""
    op = "rgbd_pyramid"
    depth, rgb = _rgbd_frame(depth, rgb, "frame", op)
    B, H, W = depth.shape
    _, ddm, scale = _rgbd_params(levels, 0.5, depth_diff_max, rgb_scale, H, W, op)
    require_hip(depth, rgb, op=op)
    sizes = rgbd_level_sizes(H, W, levels)
    out = torch.empty(2 * B * sum(h * w for h, w in sizes), dtype=torch.float32, device=depth.device)
    call("gs_rgbd_pyramid", ptr(depth), ptr(rgb), B, H, W, levels, ddm, scale, ptr(out), stream())
    pyr, o = [], 0
    for h, w in sizes:
        pyr.append(out[o:o + 2 * B * h * w].view(B, h, w, 2))
        o += 2 * B * h * w
    return pyr


def _rgbd_seam_args(op, tgt_depth, tgt_rgb, src_depth, src_rgb, intrinsics, T, lambda_geo, depth_diff_max, rgb_scale, *g_sums):
    """What rgbd_rows_raw and rgbd_rows_bwd_raw hand their entry points: the checked frames, K, T (and rgbd_rows_bwd_raw's g_sums)
    on the current HIP device -> (frames, g_sums as given to the device, the argument list up to the scalar parameters)."""
    td, tc = _rgbd_frame(tgt_depth, tgt_rgb, "target", op)
    B, H, W = td.shape
    sd, sc = _rgbd_frame(src_depth, src_rgb, "source", op, B, H, W)
    K, T = _rgbd_K(intrinsics, B, op), _rgbd_T(T, B, "T", op)
    lam, ddm, scale = _rgbd_params(1, lambda_geo, depth_diff_max, rgb_scale, H, W, op)
    if any(not torch.is_tensor(g) or tuple(g.shape) != (B, 29) for g in g_sums):
        raise ValueError("{}: g_sums should be a tensor of shape ({}, 29).".format(op, B))
    g_sums = [_f32c(g.detach()) for g in g_sums]
    require_hip(td, tc, sd, sc, K, T, *g_sums, op=op)
    return (td, tc, sd, sc), g_sums, (ptr(td), ptr(tc), ptr(sd), ptr(sc), B, H, W, ptr(K), ptr(T), lam, ddm, scale)


def rgbd_rows_raw(tgt_depth, tgt_rgb, src_depth, src_rgb, intrinsics, T, lambda_geo: float = 0.968, depth_diff_max: float = 0.07,
                  rgb_scale: float = 1.0 / 255.0):
    """One level-0 linearisation of the RGB-D alignment at T (B,4,4) (source camera -> target camera) -> (valid (B,H,W) int32,
    rows (B,H,W,14) = J_I | r_I | J_D | r_D, sums (B,29) = H upper triangle | g | err | cnt).  The seam the tests check."""
    (td, _, _, _), _, args = _rgbd_seam_args("rgbd_rows", tgt_depth, tgt_rgb, src_depth, src_rgb, intrinsics, T, lambda_geo,
                                             depth_diff_max, rgb_scale)
    (B, H, W), dev = td.shape, td.device
    valid = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    rows = torch.empty((B, H, W, 14), dtype=torch.float32, device=dev)
    sums = torch.empty((B, 29), dtype=torch.float32, device=dev)
    ws = workspace(ws_bytes("gs_rgbd_odometry_ws_bytes", B, H, W, 1), dev, "rgbd")
    call("gs_rgbd_rows", *args, ptr(valid), ptr(rows), ptr(sums), ptr(ws), ws.numel(), stream())
    return valid, rows, sums


def rgbd_rows_bwd_raw(tgt_depth, tgt_rgb, src_depth, src_rgb, intrinsics, T, g_sums, lambda_geo: float = 0.968,
                      depth_diff_max: float = 0.07, rgb_scale: float = 1.0 / 255.0):
    """The reverse of rgbd_rows_raw, the decisions held constant: g_sums (B,29), the adjoint of `sums` as rgbd_rows_raw returns them
    (err's is honoured, cnt's ignored) -> (g_tgt_depth (B,H,W), g_tgt_rgb (B,H,W,3), g_src_depth, g_src_rgb, g_T (B,3,4), rows 0..2
    of T's).  The seam the tests check."""
    frames, (g_sums,), args = _rgbd_seam_args("rgbd_rows_bwd", tgt_depth, tgt_rgb, src_depth, src_rgb, intrinsics, T, lambda_geo,
                                              depth_diff_max, rgb_scale, g_sums)
    (B, H, W), dev = frames[0].shape, frames[0].device
    grads = [torch.empty_like(t) for t in frames] + [torch.empty((B, 3, 4), dtype=torch.float32, device=dev)]
    ws = workspace(ws_bytes("gs_rgbd_odometry_bwd_ws_size", B, H, W, 1, 1), dev, "rgbd")
    call("gs_rgbd_rows_bwd", *args, ptr(g_sums), *(ptr(g) for g in grads), ptr(ws), ws.numel(), stream())
    return tuple(grads)


def _rgbd_odometry_call(td, tc, sd, sc, init, K, numiters, levels, lam, ddm, damp, scale, taped):
    """gs_rgbd_odometry, or with `taped` gs_rgbd_odometry_taped (the same launches, the same bits) -> (T, info, tape or None)."""
    (B, H, W), dev = td.shape, td.device
    out_T, info, counts = _gn_outputs(B, numiters, dev)
    ws = workspace(ws_bytes("gs_rgbd_odometry_ws_bytes", B, H, W, levels), dev, "rgbd")
    tape, extra = None, ()
    if taped:
        tape = torch.empty(ws_bytes("gs_rgbd_odometry_tape_size", B, levels, sum(numiters)) // 4, dtype=torch.float32, device=dev)
        extra = (ptr(tape),)
    call("gs_rgbd_odometry_taped" if taped else "gs_rgbd_odometry", ptr(td), ptr(tc), ptr(sd), ptr(sc), B, H, W, ptr(K), ptr(init), levels,
         counts, lam, ddm, damp, scale, ptr(out_T), ptr(info), ptr(ws), ws.numel(), stream(), *extra)
    return out_T, info, tape


class _RgbdOdometryFn(torch.autograd.Function):
    """rgbd_odometry as one autograd node: the taped forward (the plain call's bits) and gs_rgbd_odometry_bwd.  td, tc, sd, sc, K
    are contiguous fp32; init (B,16) contiguous fp32 or None."""

    @staticmethod
    def forward(ctx, td, tc, sd, sc, init, K, numiters, levels, lam, ddm, damp, scale):
        out_T, info, tape = _rgbd_odometry_call(td, tc, sd, sc, init, K, numiters, levels, lam, ddm, damp, scale, taped=True)
        ctx.save_for_backward(td, tc, sd, sc, K, tape)
        ctx.params = (numiters, levels, lam, ddm, damp, scale, init is not None)
        ctx.mark_non_differentiable(info)
        return out_T, info

    @staticmethod
    def backward(ctx, grad_T, _grad_info):
        td, tc, sd, sc, K, tape = ctx.saved_tensors
        numiters, levels, lam, ddm, damp, scale, has_init = ctx.params
        (B, H, W), dev = td.shape, td.device
        grad_T = _f32c(grad_T)
        need = list(ctx.needs_input_grad[:5])
        need[4] = need[4] and has_init
        grads = [torch.empty_like(t) if n else None for t, n in zip((td, tc, sd, sc), need)]
        grads.append(torch.empty((B, 16), dtype=torch.float32, device=dev) if need[4] else None)
        ws = workspace(ws_bytes("gs_rgbd_odometry_bwd_ws_size", B, H, W, levels, sum(numiters)), dev, "rgbd")
        counts = (nv.c_i * levels)(*numiters)
        call("gs_rgbd_odometry_bwd", ptr(td), ptr(tc), ptr(sd), ptr(sc), B, H, W, ptr(K), levels, counts, lam, ddm, damp, scale, ptr(tape),
             ptr(grad_T), *(ptr(g) for g in grads), ptr(ws), ws.numel(), stream())
        return (*grads, None, None, None, None, None, None, None)


def rgbd_odometry(tgt_depth, tgt_rgb, src_depth, src_rgb, intrinsics, init=None, numiters=(10, 5, 3), levels: int = 3,
                  lambda_geo: float = 0.968, depth_diff_max: float = 0.07, damp: float = 1e-8, rgb_scale: float = 1.0 / 255.0,
                  differentiable: bool = False):
    """Dense RGB-D odometry, coarse to fine (the rule of include/gradslam_hip.h): frames as depth (B,H,W[,1]) and rgb (B,H,W,3) with
    shared intrinsics -> (T (B,4,4) taking source-camera to target-camera coordinates, info (B,levels,4) = cnt, err, status bits,
    iterations per level).  `numiters`: iterations per level, finest first (an int: that count at every level).  No host
    synchronisation.  `differentiable=False` (the default): no gradients, the inputs are detached.  `differentiable=True`: when grad
    mode is on and one of the two depths, the two colours or `init` requires a gradient, T carries the graph -- one autograd
    node, the taped forward (the same bits) and a reverse pass on the device that holds every decision of the forward constant
    (validity, cells, the pyramid's selection, which steps were applied); of `init` rows 0..2 are differentiable; the scalar
    parameters and info are not, nor are the intrinsics (with `differentiable=True` intrinsics that require a gradient are refused)."""
    op = "rgbd_odometry"
    attached = bool(differentiable) and torch.is_grad_enabled() and any(
        torch.is_tensor(t) and t.requires_grad for t in (tgt_depth, tgt_rgb, src_depth, src_rgb, init))
    if differentiable and torch.is_grad_enabled() and torch.is_tensor(intrinsics) and intrinsics.requires_grad:
        raise NotImplementedError("{}: gradients with respect to the intrinsics are not implemented; detach them.".format(op))
    td, tc = _rgbd_frame(tgt_depth, tgt_rgb, "target", op, attached=attached)
    B, H, W = td.shape
    sd, sc = _rgbd_frame(src_depth, src_rgb, "source", op, B, H, W, attached=attached)
    K = _rgbd_K(intrinsics, B, op)
    init = None if init is None else _rgbd_T(init, B, "init", op, attached=attached)
    lam, ddm, scale = _rgbd_params(levels, lambda_geo, depth_diff_max, rgb_scale, H, W, op)
    numiters, damp = _gn_loop(numiters, levels, damp, op)
    require_hip(td, tc, sd, sc, K, init, op=op)
    if attached:
        return _RgbdOdometryFn.apply(td, tc, sd, sc, init, K, numiters, levels, lam, ddm, damp, scale)
    return _rgbd_odometry_call(td, tc, sd, sc, init, K, numiters, levels, lam, ddm, damp, scale, taped=False)[:2]


# ------------------------------------------------------------------ SDF odometry (csrc/sdf.hip)
def _sdf_args(op, depth, intrinsics, poses, tsdf, weight, origin, voxel_size, trunc, min_weight, stride, levels, attached=False,
              **transforms):
    """The checked inputs of sdf_rows_raw / sdf_odometry (the caller requires the HIP device, after its own checks): depth (B,H,W[,1]), intrinsics, poses and the
    named transforms (B,4,4) or (B,1,4,4), the volume's tsdf / weight (B,nz,ny,nx) and origin -> (tensors to keep alive, named
    transforms as (B,16) or None, (B, H, W), the C argument lists up to `stride`).  `attached`: depth, poses, the named
    transforms and tsdf keep their graphs (contiguous fp32 all the same), for the autograd node."""
    for name, t in (("depth", depth), ("intrinsics", intrinsics), ("poses", poses), ("tsdf", tsdf), ("weight", weight)):
        if not torch.is_tensor(t):
            raise TypeError("{}: expected {} to be a tensor; got {}".format(op, name, type(t)))
    if depth.ndim == 4 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if depth.ndim != 3 or 0 in depth.shape:
        raise ValueError("{}: depth should have shape (B, H, W) or (B, H, W, 1). Got {}.".format(op, tuple(depth.shape)))
    B, H, W = (int(n) for n in depth.shape)
    K = _rgbd_K(intrinsics, B, op)
    poses = _rgbd_T(poses, B, "poses", op, attached=attached)
    named = {n: (None if t is None else _rgbd_T(t, B, n, op, attached=attached)) for n, t in transforms.items()}
    if tsdf.ndim != 4 or tsdf.shape[0] != B:
        raise ValueError("{}: tsdf should have shape ({}, nz, ny, nx), the frames' batch size. Got {}.".format(op, B, tuple(tsdf.shape)))
    _, dims = _tsdf_volume(tsdf, weight, op)
    v, tr, mw = _positive(voxel_size, "voxel_size", op), _positive(trunc, "trunc", op), _number(min_weight, "min_weight", op)
    if not isinstance(stride, int) or isinstance(stride, bool) or stride < 1:
        raise ValueError("{}: stride should be a positive integer. Got {!r}.".format(op, stride))
    _gn_levels(levels, op)
    s = stride << (levels - 1)
    if -(-H // s) < 4 or -(-W // s) < 4:
        raise ValueError("{}: the coarsest of {} grids of a {} x {} image at stride {} would be smaller than 4 x 4.".format(
            op, levels, H, W, stride))
    if attached:
        depth, tsdf, weight = depth.float().contiguous(), tsdf.float().contiguous(), _f32c(weight.detach())
    else:
        depth, tsdf, weight = _f32c(depth.detach()), _f32c(tsdf.detach()), _f32c(weight.detach())
    origin = tsdf_origin(origin, B, tsdf.device, op)
    keep = (depth, K, poses, tsdf, weight, origin)
    return keep, named, (B, H, W), (ptr(depth), B, H, W, ptr(K), ptr(poses)), (ptr(tsdf), ptr(weight), *dims, ptr(origin), v, tr, mw, stride)


def sdf_rows_raw(depth, intrinsics, poses, D, tsdf, weight, origin, voxel_size, trunc, min_weight: float = 1.0, stride: int = 1):
    """One level-0 linearisation of the SDF alignment at the world-frame delta D (B,4,4) -> (valid (B,Hs,Ws) int32, rows
    (B,Hs,Ws,7) = J | r, sums (B,29) = H upper triangle | g | err | cnt) on the [::stride, ::stride] pixel grid.  The seam the
    tests check."""
    op = "sdf_rows"
    keep, named, (B, H, W), frame, volume = _sdf_args(op, depth, intrinsics, poses, tsdf, weight, origin, voxel_size, trunc, min_weight,
                                                      stride, 1, D=D)
    if named["D"] is None:
        raise TypeError("{}: expected D to be a tensor; got {}".format(op, type(D)))
    require_hip(*keep, named["D"], op=op)
    dev, Hs, Ws = keep[0].device, -(-H // stride), -(-W // stride)
    valid = torch.empty((B, Hs, Ws), dtype=torch.int32, device=dev)
    rows = torch.empty((B, Hs, Ws, 7), dtype=torch.float32, device=dev)
    sums = torch.empty((B, 29), dtype=torch.float32, device=dev)
    ws = workspace(ws_bytes("gs_sdf_odometry_ws_size", B, H, W, stride), dev, "sdf")
    call("gs_sdf_rows", *frame, ptr(named["D"]), *volume, ptr(valid), ptr(rows), ptr(sums), ptr(ws), ws.numel(), stream())
    return valid, rows, sums


def sdf_rows_bwd_raw(depth, intrinsics, poses, D, g_sums, tsdf, weight, origin, voxel_size, trunc, min_weight: float = 1.0,
                     stride: int = 1, want_tsdf: bool = True):
    """The reverse of sdf_rows_raw, the decisions held constant: g_sums (B,29), the adjoint of `sums` as sdf_rows_raw returns them
    (err's is honoured, cnt's ignored) -> (g_depth (B,H,W), g_poses (B,3,4), g_D (B,3,4): rows 0..2 of the poses' and of D's,
    g_tsdf (B,nz,ny,nx), or None with `want_tsdf=False`: no fold, no fold memory).  The seam the tests check."""
    op = "sdf_rows_bwd"
    keep, named, (B, H, W), frame, volume = _sdf_args(op, depth, intrinsics, poses, tsdf, weight, origin, voxel_size, trunc, min_weight,
                                                      stride, 1, D=D)
    if named["D"] is None:
        raise TypeError("{}: expected D to be a tensor; got {}".format(op, type(D)))
    if not torch.is_tensor(g_sums) or tuple(g_sums.shape) != (B, 29):
        raise ValueError("{}: g_sums should be a tensor of shape ({}, 29).".format(op, B))
    g_sums = _f32c(g_sums.detach())
    require_hip(*keep, named["D"], g_sums, op=op)
    dev, dims = keep[0].device, volume[2:5]
    g_depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    g_poses, g_D = (torch.empty((B, 3, 4), dtype=torch.float32, device=dev) for _ in range(2))
    g_tsdf = torch.empty_like(keep[3]) if want_tsdf else None
    room = torch.empty(ws_bytes("gs_sdf_odometry_bwd_room", B, H, W, stride, 1, 1, *dims, int(bool(want_tsdf))), dtype=torch.uint8, device=dev)
    call("gs_sdf_rows_bwd", *frame, ptr(named["D"]), *volume, ptr(g_sums), ptr(g_depth), ptr(g_poses), ptr(g_D), ptr(g_tsdf), ptr(room),
         room.numel(), stream())
    return g_depth, g_poses, g_D, g_tsdf


class _SdfOdometryFn(torch.autograd.Function):
    """sdf_odometry as one autograd node: the taped forward (the plain call's bits) and gs_sdf_odometry_bwd.  depth (B,H,W), poses
    (B,16), tsdf, weight, K, origin are contiguous fp32; init (B,16) contiguous fp32 or None.  The tape is allocated here and kept
    until the reverse pass; the reverse pass's room -- 20 bytes per voxel when tsdf takes a gradient -- only while it runs."""

    @staticmethod
    def forward(ctx, depth, poses, init, tsdf, weight, K, origin, dims, v, tr, mw, stride, levels, numiters, damp):
        (B, H, W), dev = depth.shape, depth.device
        out_T, info, counts = _gn_outputs(B, numiters, dev)
        tape = torch.empty(ws_bytes("gs_sdf_odometry_tape_bytes_for", B, H, W, stride, levels, sum(numiters)), dtype=torch.uint8, device=dev)
        call("gs_sdf_odometry_taped", ptr(depth), B, H, W, ptr(K), ptr(poses), ptr(init), ptr(tsdf), ptr(weight), *dims, ptr(origin), v, tr,
             mw, stride, levels, counts, damp, ptr(out_T), ptr(info), ptr(tape), tape.numel(), stream())
        ctx.save_for_backward(depth, poses, tsdf, weight, K, origin, tape)
        ctx.params = (dims, v, tr, mw, stride, levels, numiters, damp, init is not None)
        ctx.mark_non_differentiable(info)
        return out_T, info

    @staticmethod
    def backward(ctx, grad_T, _grad_info):
        depth, poses, tsdf, weight, K, origin, tape = ctx.saved_tensors
        dims, v, tr, mw, stride, levels, numiters, damp, has_init = ctx.params
        (B, H, W), dev = depth.shape, depth.device
        grad_T = _f32c(grad_T)
        need = list(ctx.needs_input_grad[:4])
        need[2] = need[2] and has_init
        g_depth = torch.empty_like(depth) if need[0] else None
        g_poses, g_init = (torch.empty((B, 16), dtype=torch.float32, device=dev) if n else None for n in need[1:3])
        g_tsdf = torch.empty_like(tsdf) if need[3] else None
        room = torch.empty(ws_bytes("gs_sdf_odometry_bwd_room", B, H, W, stride, levels, sum(numiters), *dims, int(need[3])),
                           dtype=torch.uint8, device=dev)
        counts = (nv.c_i * levels)(*numiters)
        call("gs_sdf_odometry_bwd", ptr(depth), B, H, W, ptr(K), ptr(poses), ptr(tsdf), ptr(weight), *dims, ptr(origin), v, tr, mw, stride,
             levels, counts, damp, ptr(tape), tape.numel(), ptr(grad_T), ptr(g_depth), ptr(g_poses), ptr(g_init), ptr(g_tsdf), ptr(room),
             room.numel(), stream())
        return (g_depth, g_poses, g_init, g_tsdf) + (None,) * 11


def sdf_odometry(depth, intrinsics, poses, tsdf, weight, origin, voxel_size, trunc, init=None, numiters=(10, 5, 3), levels: int = 3,
                 stride: int = 1, min_weight: float = 1.0, damp: float = 1e-8, differentiable: bool = False):
    """SDF odometry (the rule of include/gradslam_hip.h): the frame depth (B,H,W[,1]) carrying the camera-to-world poses (B,4,4)
    is aligned directly against the volume tsdf / weight (B,nz,ny,nx) at `origin` -- no ray cast, no cloud -> (T (B,4,4), the
    WORLD-frame delta: the new pose is compose_transformations(T, poses), the ICP providers' convention; info (B,levels,4) = cnt,
    err, status bits, iterations per level).  Level l uses the pixel grid [::stride 2^l, ::stride 2^l]; `numiters`: iterations per
    level, finest first (an int: that count at every level).  No host synchronisation.  `differentiable=False` (the default): no
    gradients: under autograd, a depth, poses, init or tsdf that requires one is refused rather than cut silently.
    `differentiable=True`: when grad mode is on and one of them requires a gradient, T carries the graph -- one autograd node, the
    taped forward (the same bits) and a reverse pass on the device that holds every decision of the forward constant (the gates,
    the cells, which steps were applied); of poses and `init` rows 0..2 are differentiable; weight, origin, the scalar parameters
    and info are not, nor are the intrinsics (with `differentiable=True` intrinsics that require a gradient are refused)."""
    op = "sdf_odometry"
    wants = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (depth, poses, init, tsdf))
    if wants and not differentiable:
        raise NotImplementedError("{}: gradients are not implemented (the reverse pass is not built); detach the inputs or call "
                                  "under torch.no_grad().".format(op))
    if differentiable and torch.is_grad_enabled() and torch.is_tensor(intrinsics) and intrinsics.requires_grad:
        raise NotImplementedError("{}: gradients with respect to the intrinsics are not implemented; detach them.".format(op))
    keep, named, (B, H, W), frame, volume = _sdf_args(op, depth, intrinsics, poses, tsdf, weight, origin, voxel_size, trunc, min_weight,
                                                      stride, levels, attached=wants, init=init)
    numiters, damp = _gn_loop(numiters, levels, damp, op)
    require_hip(*keep, named["init"], op=op)
    if wants:
        depth, K, poses, tsdf, weight, origin = keep
        return _SdfOdometryFn.apply(depth, poses, named["init"], tsdf, weight, K, origin, tuple(volume[2:5]), *volume[6:10], levels,
                                    numiters, damp)
    dev = keep[0].device
    out_T, info, counts = _gn_outputs(B, numiters, dev)
    ws = workspace(ws_bytes("gs_sdf_odometry_ws_size", B, H, W, stride), dev, "sdf")
    call("gs_sdf_odometry", *frame, ptr(named["init"]), *volume, levels, counts, damp, ptr(out_T), ptr(info), ptr(ws), ws.numel(), stream())
    return out_T, info
