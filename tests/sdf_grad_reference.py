"""The reference of the SDF odometry's reverse pass (tests/test_sdf_odometry_grads.py): the rule of include/gradslam_hip.h as a
torch transcription, written ONCE for a dtype, one batch element at a time, so that torch autograd differentiates it.  The
operations are those of tests/test_sdf_odometry.py's ref_rows / ref_step, in their order.

* The DECISIONS -- which pixels pass the depth gate, the cell each point falls in, the weight and free-space gates, whether a step
  is applied -- are computed on detached values and enter the differentiable part as index sets: autograd sees them as
  constants, which is the rule of the reverse pass.  A `Decisions` object (tests/rgbd_grad_reference.py's) records them in the
  order they are taken and can replay them at other inputs (central differences of the function autograd differentiates).
* The 6 x 6 system is solved in float64 for either dtype, as the device does (the damping is added in the dtype): the step, the
  exponential and the constants are tests/rgbd_grad_reference.py's -- the two loops share them on the device too (gs_gn_step.hpp).
* With dtype = float64 autograd of this is the reference.  With float32 it measures what fp32 alone costs -- in AUTOGRAD'S order
  of operations, not the device's: the forward operations are the device's, the reverse ones are whatever torch emits.

A volume is a dict: tsdf (nz,ny,nx) tensor of the dtype (the differentiable part), weight (nz,ny,nx) numpy fp32, origin (3,) numpy
fp32, v and trunc (Python floats, the fp32 values the device gets).
"""
import numpy as np
import torch

from tests.rgbd_grad_reference import DAMP, Decisions, c32, leaves, se3_exp, step  # noqa: F401  (re-exported)


def _point(d, w, h, K, P, D):
    fx, fy, cx, cy = K
    px, py = d * ((w - cx) / fx), d * ((h - cy) / fy)
    pw = [((P[i, 0] * px + P[i, 1] * py) + P[i, 2] * d) + P[i, 3] for i in range(3)]
    return [((D[i, 0] * pw[0] + D[i, 1] * pw[1]) + D[i, 2] * pw[2]) + D[i, 3] for i in range(3)]


def _corner(A, ix, iy, iz, c):
    return A[iz + (c >> 2), iy + ((c >> 1) & 1), ix + (c & 1)]


def linearize(depth, K, P, D, vol, dt, dec, stride=1, minw=1.0):
    """One linearisation on the [::stride, ::stride] grid -> (rows (n, 7) = J | r of the n valid pixels, (hs, ws, ix, iy, iz):
    their full-resolution pixels and the cells they fall in).  depth (H,W), P and D (3,4): tensors of dtype dt."""
    H, W = depth.shape
    nz, ny, nx = vol["tsdf"].shape
    Kt = [torch.tensor(float(k), dtype=dt) for k in K]
    v, trunc = c32(vol["v"], dt), c32(vol["trunc"], dt)
    o = [c32(x, dt) for x in vol["origin"]]
    weight = torch.from_numpy(np.ascontiguousarray(vol["weight"]))

    def decide():
        d = depth[::stride, ::stride]
        h, w = torch.meshgrid(torch.arange(0, H, stride).to(dt), torch.arange(0, W, stride).to(dt), indexing="ij")
        live = (d > 0) & torch.isfinite(d)
        q = _point(torch.where(live, d, torch.ones_like(d)), w, h, Kt, P, D)
        fi = [torch.floor((q[k] - o[k]) / v - 0.5) for k in range(3)]
        inside = live
        for k, n in enumerate((nx, ny, nz)):
            inside = inside & (fi[k] >= 0) & (fi[k] + 1 <= n - 1)
        ix, iy, iz = (torch.where(inside, fi[k], torch.zeros_like(fi[k])).long() for k in range(3))
        ok = inside
        for c in range(8):
            ok = ok & (_corner(weight, ix, iy, iz, c) >= np.float32(minw)) & (_corner(vol["tsdf"], ix, iy, iz, c) < 1.0)
        i, j = torch.nonzero(ok, as_tuple=True)
        return i * stride, j * stride, ix[i, j], iy[i, j], iz[i, j]

    hs, ws, ix, iy, iz = dec.take(decide)
    q = _point(depth[hs, ws], ws.to(dt), hs.to(dt), Kt, P, D)
    cell = (ix, iy, iz)
    ax, ay, az = ((q[k] - o[k]) / v - 0.5 - cell[k].to(dt) for k in range(3))
    f = [_corner(vol["tsdf"], ix, iy, iz, c) for c in range(8)]
    lerp = lambda p_, q_, s: p_ + s * (q_ - p_)
    fh = lerp(lerp(lerp(f[0], f[1], ax), lerp(f[2], f[3], ax), ay), lerp(lerp(f[4], f[5], ax), lerp(f[6], f[7], ax), ay), az)
    gx = lerp(lerp(f[1] - f[0], f[3] - f[2], ay), lerp(f[5] - f[4], f[7] - f[6], ay), az)
    gy = lerp(lerp(f[2] - f[0], f[3] - f[1], ax), lerp(f[6] - f[4], f[7] - f[5], ax), az)
    gz = lerp(lerp(f[4] - f[0], f[5] - f[1], ax), lerp(f[6] - f[2], f[7] - f[3], ax), ay)
    kappa = trunc / v
    r = trunc * fh
    n0, n1, n2 = kappa * gx, kappa * gy, kappa * gz
    cols = [n0, n1, n2, q[1] * n2 - q[2] * n1, q[2] * n0 - q[0] * n2, q[0] * n1 - q[1] * n0, r]
    return torch.stack(cols, -1), (hs, ws, ix, iy, iz)


def sums29(rows, dt):
    """H upper triangle | g = MINUS the sum | err | cnt."""
    J, r = rows[:, :6], rows[:, 6]
    out = [(J[:, m] * J[:, n]).sum() for m in range(6) for n in range(m, 6)]
    out += [-(J[:, m] * r).sum() for m in range(6)]
    out += [(r * r).sum(), torch.tensor(float(rows.shape[0]), dtype=dt)]
    return torch.stack(out)


def odometry(depth, K, P, vol, stride, levels, numiters, dt, init=None, dec=None):
    """One batch element, the whole loop: depth (H,W), P (3,4), init (3,4) or None, vol["tsdf"]: tensors of dtype dt -> D (3,4)."""
    dec = dec or Decisions()
    D = torch.eye(4, dtype=dt)[:3] if init is None else init
    for l in range(levels - 1, -1, -1):
        for _ in range(numiters[l]):
            rows, _ = linearize(depth, K, P, D, vol, dt, dec, stride=stride << l)
            D = step(sums29(rows, dt), D, dt, dec)
    return D


def seam(depth, K, P, D, vol, dt, stride=1, dec=None):
    """One level-0 linearisation at D (3,4) -> (the 29 sums, the valid pixels and their cells)."""
    dec = dec or Decisions()
    rows, where = linearize(depth, K, P, D, vol, dt, dec, stride=stride)
    return sums29(rows, dt), where
