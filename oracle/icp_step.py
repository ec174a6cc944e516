"""Float64 restatement of ONE O(1) step of the device (grad)ICP loop, and a float64 loop to differentiate.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

``step(row, T_prev)`` takes what one trace row of the device loop holds (include/gradslam_hip.h:
``H36 | g6 | err | new_err | damp | accept | cnt``, fp32) and the transform before the step, and restates the step:
the damping added in fp32, the 6x6 system solved in float64 and rounded to fp32, the ``se3_exp`` branch picked from an
fp32 ``th`` formed in the kernel's fma order, the LM rule or the gradLM gates, ``T = dT . T`` in float64.  It also
reports which path the kernel's solver takes for this matrix: the no-pivot elimination, or the pivoted fallback when a
pivot is not a positive finite number.  Reference: odometry/icputils.py:310-367 (LM), :479-545 (gradLM),
geometry/se3utils.py:77-115 (se3_exp).

``loop_f64`` is the reference's loop run in float64 with torch autograd, for gradients.  It can drop one adjoint term at a
time (``ablate``), so that a test can show that it would see that term missing.
"""
from fractions import Fraction

import numpy as np
import torch

SMALL_ANGLE = np.float32(1e-6)  # reference geometry/se3utils.py:8, compared in fp32 by the kernel


# ------------------------------------------------------------------ fp32 arithmetic of the kernel
def _round32(q: Fraction) -> np.float32:
    """q rounded once to fp32 (nearest, ties to even)."""
    f = np.float32(float(q))  # float(q) is correctly rounded to fp64; settle a double rounding below
    if Fraction(float(f)) == q:
        return f
    lo, hi = (f, np.nextafter(f, np.float32(np.inf))) if Fraction(float(f)) < q else (np.nextafter(f, np.float32(-np.inf)), f)
    dl, dh = q - Fraction(float(lo)), Fraction(float(hi)) - q
    if dl != dh:
        return lo if dl < dh else hi
    return lo if (lo.view(np.int32) & 1) == 0 else hi


def fma32(a, b, c) -> np.float32:
    """fmaf(a, b, c): the exact a * b + c, rounded once to fp32."""
    return _round32(Fraction(float(np.float32(a))) * Fraction(float(np.float32(b))) + Fraction(float(np.float32(c))))


def theta32(w) -> np.float32:
    """|w| as se3_exp_dev forms it: sqrtf(fmaf(w2, w2, fmaf(w1, w1, w0 * w0)))."""
    w = np.asarray(w, dtype=np.float32)
    p = np.float32(w[0] * w[0])
    p = fma32(w[1], w[1], p)
    p = fma32(w[2], w[2], p)
    return np.sqrt(p)  # IEEE sqrt: correctly rounded, like the device's sqrtf


def damped32(H, damp) -> np.ndarray:
    """H + damp I with the diagonal added in fp32 (reference odometry/icputils.py:86-87)."""
    M = np.array(H, dtype=np.float32).reshape(6, 6).copy()
    for i in range(6):
        M[i, i] = np.float32(M[i, i] + np.float32(damp))
    return M


def nopivot_pivots(M32, g32):
    """Gauss-Jordan without pivoting on [M | g] in fp64 (solve6_wave).  Returns (pivots, x, ok): ok is False when a
    pivot is not a positive finite number, which is when the kernel hands the system to the pivoted elimination."""
    a = np.zeros((6, 7))
    a[:, :6] = np.asarray(M32, dtype=np.float64)
    a[:, 6] = np.asarray(g32, dtype=np.float64)
    piv = []
    with np.errstate(all="ignore"):
        for j in range(6):
            p = a[j, j]
            piv.append(p)
            inv = 1.0 / p
            prow = a[j].copy()
            col = a[:, j].copy()
            a = a - np.outer(col * inv, prow)
            a[j] = prow * inv
    piv = np.array(piv)
    ok = bool(np.all(piv > 0.0) and np.all(piv < 1e300))
    return piv, a[:, 6].copy(), ok


def pivoted_solve(M32, g32) -> np.ndarray:
    """Elimination with partial pivoting in fp64 (solve6_lu)."""
    M = np.zeros((6, 7))
    M[:, :6] = np.asarray(M32, dtype=np.float64)
    M[:, 6] = np.asarray(g32, dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in range(6):
            p = c + int(np.argmax(np.abs(M[c:, c])))
            if np.abs(M[p, c]) > np.abs(M[c, c]):
                M[[c, p]] = M[[p, c]]
            for r in range(c + 1, 6):
                f = M[r, c] / M[c, c]
                M[r, c:] -= f * M[c, c:]
        x = np.zeros(6)
        for r in range(5, -1, -1):
            x[r] = (M[r, 6] - M[r, r + 1:6] @ x[r + 1:]) / M[r, r]
    return x


def se3_exp64(xi, small: bool) -> np.ndarray:
    """se3_exp of the reference in float64 on the given branch (small: V = I + w^, sic)."""
    xi = np.asarray(xi, dtype=np.float64)
    v, w = xi[:3], xi[3:]
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if small:
        R = np.eye(3) + W
        V = R.copy()
    else:
        th = np.sqrt(w @ w)
        s, c = np.sin(th), np.cos(th)
        W2 = W @ W
        R = np.eye(3) + (s / th) * W + ((1 - c) / th ** 2) * W2
        V = np.eye(3) + ((1 - c) / th ** 2) * W + ((th - s) / th ** 3) * W2
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = V @ v
    return T


def grad_gates32(err, new_err, damp, grad_params):
    """The gradLM gates in fp32 as the kernel forms them (GradParams rounded once from fp64 on the host).
    Returns (raw diff, clamped diff, damp_next, sigma)."""
    lmax, B, B2, nu = grad_params
    lmin = np.float32(1.0 / lmax)
    rng = np.float32(lmax - 1.0 / lmax)
    f = np.float32
    raw = f(f(new_err) - f(err))
    diff = f(min(max(raw, f(-70.0)), f(70.0)))
    damp_new = f(lmin + f(rng / f(f(1.0) + np.exp(f(-f(B)) * diff))))
    sig = f(f(1.0) / np.power(f(f(1.0) + np.exp(f(-f(B2)) * diff)), f(1.0 / nu)))
    return raw, diff, f(f(damp) * damp_new), sig


def step(row, T_prev, grad_params=None) -> dict:
    """One step from one trace row (48 fp32) and the transform before it.  grad_params = (lambda_max, B, B2, nu)
    selects the gradLM step, None the LM step."""
    row = np.asarray(row, dtype=np.float32)
    H, g = row[:36], row[36:42]
    err, new_err, damp = row[42], row[43], row[44]
    M = damped32(H, damp)
    piv, x_np, ok = nopivot_pivots(M, g)
    M64 = M.astype(np.float64)
    x64 = np.linalg.solve(M64, g.astype(np.float64))  # the fp64 solution of the fp32 system
    xi = (x_np if ok else pivoted_solve(M, g)).astype(np.float32)
    out = dict(path="nopivot" if ok else "pivoted", pivots=piv, cond=float(np.linalg.cond(M64)), xi=xi, xi64=x64,
               th=theta32(xi[3:]), err=err, new_err=new_err)
    out["small"] = bool(out["th"] < SMALL_ANGLE)
    T_prev = np.asarray(T_prev, dtype=np.float64)
    if grad_params is None:
        out["accept"] = bool(new_err < err)  # strict: a tie rejects
        out["damp"] = np.float32(damp / np.float32(2)) if out["accept"] else np.float32(damp * np.float32(2))
        out["T"] = se3_exp64(xi, out["small"]) @ T_prev if out["accept"] else T_prev.copy()
    else:
        raw, diff, out["damp"], sig = grad_gates32(err, new_err, damp, grad_params)
        sx = (sig * xi).astype(np.float32)
        out.update(accept=True, raw_diff=raw, diff=diff, sigma=sig, sxi=sx, sth=theta32(sx[3:]))
        out["ssmall"] = bool(out["sth"] < SMALL_ANGLE)
        out["T"] = se3_exp64(sx, out["ssmall"]) @ T_prev
    return out


def oracle_row(rec: dict) -> np.ndarray:
    """A trace row (48 fp32) from one record of oracle.icp's trace list."""
    row = np.zeros(48, dtype=np.float32)
    row[:36] = rec["AtA"].reshape(-1).numpy()
    row[36:42] = rec["Atb"].reshape(-1).numpy()
    row[42], row[43], row[44] = float(rec["err"]), float(rec["new_err"]), float(rec["damp"])
    row[45] = 1.0 if rec.get("accept", True) else 0.0
    row[46] = rec["idx"].numel()
    return row


# ------------------------------------------------------------------ float64 loop with autograd
def _hat(w):
    z = w.new_zeros(())
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def se3_exp_t(xi, small: bool, drop_dC: bool = False):
    """geometry/se3utils.py:77-115 in float64 torch; drop_dC removes the adjoint of C through th (gC . dC)."""
    v, w = xi[:3], xi[3:]
    W = _hat(w)
    I = torch.eye(3, dtype=xi.dtype)
    if small:
        R = I + W
        V = I + W
    else:
        th = w.norm()
        s, c = th.sin(), th.cos()
        W2 = W @ W
        thc = th.detach() if drop_dC else th
        C = (thc - thc.sin()) / thc ** 3
        R = I + (s / th) * W + ((1 - c) / th ** 2) * W2
        V = I + ((1 - c) / th ** 2) * W + C * W2
    top = torch.cat([R, (V @ v).view(3, 1)], 1)
    return torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=xi.dtype)], 0)


def _xform(p, T):
    return p @ T[:3, :3].t() + T[:3, 3]


def _linearize(s, tgt, nrm):
    """odometry/icputils.py:196-232 in float64 with an exact nearest neighbour.  Also returns, over the sources, the
    smallest gap between the nearest and the second nearest target distance (how unambiguous the association is)."""
    with torch.no_grad():
        d2 = ((s.detach()[:, None, :] - tgt.detach()[None, :, :]) ** 2).sum(-1)
        two = torch.topk(d2, min(2, d2.shape[1]), dim=1, largest=False)
        idx = two.indices[:, 0]
        gap = float((two.values[:, 1].sqrt() - two.values[:, 0].sqrt()).min()) if d2.shape[1] > 1 else float("inf")
    d, n = tgt[idx], nrm[idx]
    A = torch.cat([n, torch.linalg.cross(s, n)], 1)
    b = (n * (d - s)).sum(1, keepdim=True)
    return A, b, idx, gap


def loop_f64(src, tgt, nrm, T0, numiters, damp, grad_params=None, ablate=()):
    """point_to_plane_ICP (grad_params None) / point_to_plane_gradICP on float64 tensors, no distance threshold.
    The damp starts from the fp32 value the kernel starts from; every se3_exp branch is picked from the fp32 th of the
    fp32-rounded argument, as the kernel picks it.  ablate: a subset of {"dC", "damp", "sigma"}: drop gC . dC in
    se3_exp's adjoint, the adjoint of the solve with respect to damp, or the sigma chain of gradLM.
    Returns (T, log): log holds per iteration the association, its gap, err, new_err, the accept decision and the
    branches taken."""
    th32 = lambda x: theta32(x.detach().numpy()[3:].astype(np.float32))
    s = _xform(src, T0)
    T = T0
    damp = torch.tensor(float(np.float32(damp)), dtype=torch.float64)
    log = []
    for _ in range(numiters):
        A, b, idx, gap = _linearize(s, tgt, nrm)
        dd = damp.detach() if "damp" in ablate else damp
        xi = torch.linalg.solve(A.t() @ A + dd * torch.eye(6, dtype=A.dtype), A.t() @ b)[:, 0]
        err = (b * b).sum()
        small = bool(th32(xi) < SMALL_ANGLE)
        dT = se3_exp_t(xi, small, "dC" in ablate)
        look = _xform(s, dT)
        _, b1, _, gap1 = _linearize(look, tgt, nrm)
        new_err = (b1 * b1).sum()
        rec = dict(idx=idx, gap=min(gap, gap1), err=float(err.detach()), new_err=float(new_err.detach()), small=small,
                   xi=xi.detach().clone())
        if grad_params is None:
            rec["accept"] = bool(new_err < err)
            if rec["accept"]:
                s, damp, T = look, damp / 2, dT @ T
            else:
                damp = damp * 2
        else:
            lmax, Bg, B2, nu = grad_params
            lmin = 1.0 / lmax
            diff = (new_err - err).clamp(-70.0, 70.0)
            damp = damp * (lmin + (lmax - lmin) / (1 + torch.exp(-Bg * diff)))
            sig = 1 / ((1 + torch.exp(-B2 * diff)) ** (1 / nu))
            if "sigma" in ablate:
                sig = sig.detach()
            sx = sig * xi
            rec.update(accept=True, ssmall=bool(th32(sx) < SMALL_ANGLE), raw_diff=float((new_err - err).detach()))
            dT2 = se3_exp_t(sx, rec["ssmall"], "dC" in ablate)
            s, T = _xform(s, dT2), dT2 @ T
        log.append(rec)
    return T, log
