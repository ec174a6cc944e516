"""Trajectory metrics on (B, L, 4, 4) camera poses: plain torch, O(L), differentiable, any device."""
import torch


def _poses(est, gt):
    for name, p in (("est", est), ("gt", gt)):
        if not torch.is_tensor(p):
            raise TypeError("Expected {0} to be of type torch.Tensor. Got {1}.".format(name, type(p)))
        if p.ndim != 4 or p.shape[-2:] != (4, 4):
            raise ValueError("Expected {0} to have shape (B, L, 4, 4). Got {1}.".format(name, tuple(p.shape)))
    if est.shape != gt.shape:
        raise ValueError("Expected est and gt to have the same shape. Got {0} and {1}.".format(tuple(est.shape), tuple(gt.shape)))


def _inv(T):
    """inverse of rigid transforms (..., 4, 4): [R^T, -R^T t]"""
    Rt = T[..., :3, :3].transpose(-1, -2)
    t = -(Rt @ T[..., :3, 3:])
    return torch.cat([torch.cat([Rt, t], dim=-1), T[..., 3:, :]], dim=-2)


def absolute_trajectory_error(est: torch.Tensor, gt: torch.Tensor, align: str = "none") -> torch.Tensor:
    """RMSE of the camera positions of `est` against `gt` -> (B,).  align: "none" (compare as given), "first" (move est by
    the rigid motion that puts its first pose on gt's first pose) or "rigid" (the least-squares rotation + translation of
    est's positions onto gt's, closed form, no scale)."""
    _poses(est, gt)
    if align not in ("none", "first", "rigid"):
        raise ValueError('align must be one of "none", "first", "rigid". Got {0}.'.format(align))
    p, q = est[..., :3, 3], gt[..., :3, 3]  # (B, L, 3)
    if align == "first":
        A = gt[:, :1] @ _inv(est[:, :1])  # (B, 1, 4, 4)
        p = (A[..., :3, :3] @ p.unsqueeze(-1)).squeeze(-1) + A[..., :3, 3]
    elif align == "rigid":
        pm, qm = p.mean(dim=1, keepdim=True), q.mean(dim=1, keepdim=True)
        pc, qc = p - pm, q - qm
        H = pc.transpose(1, 2) @ qc  # (B, 3, 3) = sum_i pc_i qc_i^T
        U, _, Vh = torch.linalg.svd(H)
        V = Vh.transpose(1, 2)
        sign = torch.sign(torch.linalg.det(V @ U.transpose(1, 2))).detach()
        D = torch.diag_embed(torch.stack([torch.ones_like(sign), torch.ones_like(sign), sign], dim=-1))
        R = V @ D @ U.transpose(1, 2)  # argmin_R sum |R pc_i - qc_i|^2 over rotations
        p = (R.unsqueeze(1) @ pc.unsqueeze(-1)).squeeze(-1) + qm
    return ((p - q) ** 2).sum(dim=-1).mean(dim=1).sqrt()


def relative_pose_error(est: torch.Tensor, gt: torch.Tensor, delta: int = 1):
    """RMSE over i of the error of the relative motion i -> i + delta: E_i = (gt_i^-1 gt_{i+delta})^-1 (est_i^-1 est_{i+delta})
    -> (trans_rmse (B,), rot_rmse (B,) in radians).  The rotation error is the angle of E_i's rotation as
    atan2(|axis part of (R - R^T) / 2|, (trace R - 1) / 2): finite, with a finite gradient, at angle 0."""
    _poses(est, gt)
    L = est.shape[1]
    if not isinstance(delta, int) or delta < 1 or delta >= L:
        raise ValueError("delta must be an integer in [1, L - 1] = [1, {0}]. Got {1}.".format(L - 1, delta))
    rel_e = _inv(est[:, :-delta]) @ est[:, delta:]
    rel_g = _inv(gt[:, :-delta]) @ gt[:, delta:]
    E = _inv(rel_g) @ rel_e
    R = E[..., :3, :3]
    trans2 = (E[..., :3, 3] ** 2).sum(dim=-1)
    axis = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], dim=-1)
    sin = torch.linalg.vector_norm(axis, dim=-1)
    cos = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    angle = torch.atan2(sin, cos)
    return trans2.mean(dim=1).sqrt(), (angle ** 2).mean(dim=1).sqrt()
