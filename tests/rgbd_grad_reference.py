"""The reference of the RGB-D odometry's reverse pass (tests/test_rgbd_odometry_grads.py): the rule of include/gradslam_hip.h as a
torch transcription, written ONCE for a dtype, one batch element at a time, so that torch autograd differentiates it.

* The DECISIONS -- which source pixels are valid and the cell each falls in, which depths a pyramid block takes, the level-0 depth
  clean-up, whether a step is applied -- are computed on detached values and enter the differentiable part as index sets and
  masks: autograd sees them as constants, which is the rule of the reverse pass.  A `Decisions` object records them in the
  order they are taken and can replay them at other inputs (central differences of the function autograd differentiates).
* The 6 x 6 system is solved in float64 for either dtype, as the device does (the damping is added in the dtype).
* With dtype = float64 autograd of this is the reference.  With float32 it measures what fp32 alone costs -- in AUTOGRAD'S order
  of operations, not the device's: the forward operations are the device's, the reverse ones are whatever torch emits.
"""
import numpy as np
import torch

LAM, DDM, DAMP, SCALE = 0.968, 0.07, 1e-8, 1.0 / 255.0


class Decisions:
    """Record (default) or replay the decisions of one run, in order."""

    def __init__(self):
        self.items, self.pos, self.replaying = [], 0, False

    def replay(self):
        d = Decisions()
        d.items, d.replaying = self.items, True
        return d

    def take(self, compute):
        if self.replaying:
            self.pos += 1
            return self.items[self.pos - 1]
        with torch.no_grad():
            item = compute()
        self.items.append(item)
        return item


def c32(x, dt):
    """The fp32 constant the device uses, in dt."""
    return torch.tensor(float(np.float32(x)), dtype=dt)


def level0(depth, rgb, dt, dec, scale=SCALE):
    keep = dec.take(lambda: (depth > 0) & torch.isfinite(depth))
    I = c32(scale, dt) * ((c32(0.299, dt) * rgb[..., 0] + c32(0.587, dt) * rgb[..., 1]) + c32(0.114, dt) * rgb[..., 2])
    return I, torch.where(keep, depth, torch.zeros((), dtype=dt))


def down(I, D, dt, dec, ddm=DDM):
    H2, W2 = I.shape[0] // 2, I.shape[1] // 2
    blk = lambda A: [A[0:2 * H2:2, 0:2 * W2:2], A[0:2 * H2:2, 1:2 * W2:2], A[1:2 * H2:2, 0:2 * W2:2], A[1:2 * H2:2, 1:2 * W2:2]]
    i, d = blk(I), blk(D)
    Io = (((i[0] + i[1]) + i[2]) + i[3]) * 0.25

    def decide():
        dmin = torch.full((H2, W2), float("inf"), dtype=dt)
        for k in range(4):
            dmin = torch.where((d[k] > 0) & (d[k] < dmin), d[k], dmin)
        return [(d[k] > 0) & (d[k] - dmin <= c32(ddm, dt)) for k in range(4)]

    take = dec.take(decide)
    s, n = torch.zeros((H2, W2), dtype=dt), torch.zeros((H2, W2), dtype=dt)
    for k in range(4):
        s = torch.where(take[k], s + d[k], s)
        n = n + take[k].to(dt)
    return Io, torch.where(n > 0, s / torch.clamp(n, min=1), torch.zeros((), dtype=dt))


def pyramid(depth, rgb, levels, dt, dec):
    pyr = [level0(depth, rgb, dt, dec)]
    for _ in range(1, levels):
        pyr.append(down(pyr[-1][0], pyr[-1][1], dt, dec))
    return pyr


def level_K(K, level, dt):
    fx, fy, cx, cy = (torch.tensor(k, dtype=dt) for k in K)
    for _ in range(level):
        fx, fy = fx * 0.5, fy * 0.5
        cx, cy = (cx + 0.5) * 0.5 - 0.5, (cy + 0.5) * 0.5 - 0.5
    return fx, fy, cx, cy


def _warp(d, u, v, K, T):
    fx, fy, cx, cy = K
    px, py = d * ((u - cx) / fx), d * ((v - cy) / fy)
    qx, qy, qz = (((T[i, 0] * px + T[i, 1] * py) + T[i, 2] * d) + T[i, 3] for i in range(3))
    iz = 1.0 / qz
    return qx, qy, qz, iz, (fx * qx) * iz + cx, (fy * qy) * iz + cy


def _sample(F00, F10, F01, F11, a, b):
    X0, X1 = F10 - F00, F11 - F01
    top, bot = F00 + a * X0, F01 + a * X1
    return top + b * (bot - top), X0 + b * (X1 - X0), bot - top


def linearize(tI, tD, sI, sD, K, T, dt, dec, lam=LAM, ddm=DDM):
    """One linearisation -> (rows (n, 14) of the n valid pixels, (vs, us, i, j): where they are and their cells)."""
    H, W = sD.shape
    cut = c32(ddm, dt)

    def decide():
        v, u = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
        ok = sD > 0
        _, _, qz, _, x, y = _warp(sD, u, v, K, T)
        xf, yf = torch.floor(x), torch.floor(y)
        ok = ok & (qz > 0) & (xf >= 0) & (xf <= W - 2) & (yf >= 0) & (yf <= H - 2)
        i, j = torch.where(ok, xf, torch.zeros_like(xf)).long(), torch.where(ok, yf, torch.zeros_like(yf)).long()
        D = [tD[j, i], tD[j, i + 1], tD[j + 1, i], tD[j + 1, i + 1]]
        ok = ok & (D[0] > 0) & (D[1] > 0) & (D[2] > 0) & (D[3] > 0)
        Dh, _, _ = _sample(*D, x - xf, y - yf)
        ok = ok & ((Dh - qz).abs() <= cut)
        vs, us = torch.nonzero(ok, as_tuple=True)
        return vs, us, i[vs, us], j[vs, us]

    vs, us, i, j = dec.take(decide)
    qx, qy, qz, iz, x, y = _warp(sD[vs, us], us.to(dt), vs.to(dt), K, T)
    a, b = x - i.to(dt), y - j.to(dt)
    corners = lambda F: (F[j, i], F[j, i + 1], F[j + 1, i], F[j + 1, i + 1])
    Ih, Ix, Iy = _sample(*corners(tI), a, b)
    Dh, Dx, Dy = _sample(*corners(tD), a, b)
    ri, rd = Ih - sI[vs, us], Dh - qz
    lam32 = c32(lam, dt)
    wI, wD = torch.sqrt(1.0 - lam32), torch.sqrt(lam32)
    fx, fy = K[0], K[1]
    gx, gy = fx * iz, fy * iz
    i0, i1 = Ix * gx, Iy * gy
    i2 = -((i0 * qx + i1 * qy) * iz)
    d0, d1 = Dx * gx, Dy * gy
    d2 = -((d0 * qx + d1 * qy) * iz) - 1.0
    cols = [wI * i0, wI * i1, wI * i2, wI * (qy * i2 - qz * i1), wI * (qz * i0 - qx * i2), wI * (qx * i1 - qy * i0), wI * ri,
            wD * d0, wD * d1, wD * d2, wD * (qy * d2 - qz * d1), wD * (qz * d0 - qx * d2), wD * (qx * d1 - qy * d0), wD * rd]
    return torch.stack(cols, -1), (vs, us, i, j)


def sums29(rows, dt):
    """H upper triangle | g = MINUS the sum | err | cnt."""
    JI, rI, JD, rD = rows[:, :6], rows[:, 6], rows[:, 7:13], rows[:, 13]
    out = [(JI[:, m] * JI[:, n] + JD[:, m] * JD[:, n]).sum() for m in range(6) for n in range(m, 6)]
    out += [-(JI[:, m] * rI + JD[:, m] * rD).sum() for m in range(6)]
    out += [(rI * rI + rD * rD).sum(), torch.tensor(float(rows.shape[0]), dtype=dt)]
    return torch.stack(out)


def se3_exp(xi, dt):
    """geometry.se3utils.se3_exp / the device's se3_exp_dev (xi = [v; omega]; the small-angle branch uses V = I + w^)."""
    v, w = xi[:3], xi[3:]
    z = torch.zeros((), dtype=dt)
    Wh = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    I3 = torch.eye(3, dtype=dt)
    if float((w * w).detach().sum().sqrt()) < 1e-6:  # (a decision on a detached value)
        R = I3 + Wh
        V = R
    else:
        th = (w * w).sum().sqrt()
        s, c, W2 = torch.sin(th), torch.cos(th), Wh @ Wh
        A, Bc, C = s / th, (1.0 - c) / (th * th), (th - s) / (th * th * th)
        R, V = (I3 + A * Wh) + Bc * W2, (I3 + Bc * Wh) + C * W2
    return R, V @ v


def step(acc, T, dt, dec, damp=DAMP):
    """T (3, 4) -> T' (3, 4): the step, or T itself when it is not applied (a decision)."""
    Hm = torch.zeros((6, 6), dtype=dt)
    iu = torch.triu_indices(6, 6)
    Hm = Hm.index_put((iu[0], iu[1]), acc[:21])
    Hm = Hm + torch.triu(Hm, 1).T
    A = Hm + c32(damp, dt) * torch.eye(6, dtype=dt)
    if float(acc[28].detach()) < 6:
        assert not dec.take(lambda: False)
        return T
    xi = torch.linalg.solve(A.double(), acc[21:27].double()).to(dt)
    R, t = se3_exp(xi, dt)
    Tn = torch.cat([R @ T[:, :3], (R @ T[:, 3] + t)[:, None]], 1)
    applied = dec.take(lambda: bool(torch.isfinite(xi).all() and torch.isfinite(Tn).all()))
    return Tn if applied else T


def odometry(td, tc, sd, sc, K, levels, numiters, dt, init=None, dec=None):
    """One batch element, the whole loop: depth (H,W), rgb (H,W,3) tensors of dtype dt, init (3,4) or None -> T (3,4)."""
    dec = dec or Decisions()
    tp, sp = pyramid(td, tc, levels, dt, dec), pyramid(sd, sc, levels, dt, dec)
    T = torch.eye(4, dtype=dt)[:3] if init is None else init
    for l in range(levels - 1, -1, -1):
        Kl = level_K(K, l, dt)
        for _ in range(numiters[l]):
            rows, _ = linearize(tp[l][0], tp[l][1], sp[l][0], sp[l][1], Kl, T, dt, dec)
            T = step(sums29(rows, dt), T, dt, dec)
    return T


def seam(td, tc, sd, sc, K, T, dt, dec=None):
    """One level-0 linearisation at T (3,4) from the images -> (the 29 sums, the valid pixels and their cells)."""
    dec = dec or Decisions()
    (tI, tD), (sI, sD) = level0(td, tc, dt, dec), level0(sd, sc, dt, dec)
    rows, where = linearize(tI, tD, sI, sD, level_K(K, 0, dt), T, dt, dec)
    return sums29(rows, dt), where


def leaves(arrays, dt):
    """numpy arrays -> leaf tensors of dtype dt that require gradients."""
    return [torch.tensor(np.asarray(a), dtype=dt).requires_grad_(True) for a in arrays]
