"""Map metrics on `Pointclouds`: chamfer distance, nearest neighbours, reconstruction figures."""
from typing import Optional

import torch

from .. import ops
from ..structures.pointclouds import Pointclouds

# What `reorder=None` means: scan each target cloud in cell-grid order (True) or as its rows come (False).  The choice is
# the setting whose slower case of {image-ordered, shuffled} clouds is faster ("map metrics").
REORDER_DEFAULT = True


def _pair(x, y, names=("x", "y")):
    for name, pc in zip(names, (x, y)):
        if not isinstance(pc, Pointclouds):
            raise TypeError("Expected {0} to be of type gradslam.Pointclouds. Got {1}.".format(name, type(pc)))
    if len(x) != len(y):
        raise ValueError("Expected {0} and {1} to have the same batch size. Got {2} and {3}.".format(names[0], names[1], len(x), len(y)))
    for name, pc in zip(names, (x, y)):
        if len(pc) == 0 or not pc.has_points or pc.points_padded.shape[1] == 0:
            raise ValueError("Expected {0} to hold at least one point in some cloud of its batch.".format(name))


def _reorder(reorder: Optional[bool]) -> bool:
    return REORDER_DEFAULT if reorder is None else bool(reorder)


def _counts_f(pc: Pointclouds) -> torch.Tensor:
    return pc._counts_i32().clamp(min=1).to(torch.float32)


def chamfer_distance(x: Pointclouds, y: Pointclouds, squared: bool = True, point_reduction: str = "mean",
                     batch_reduction: Optional[str] = "mean", single_directional: bool = False, reorder: Optional[bool] = None):
    """Chamfer distance between two batches of clouds, differentiable w.r.t. both clouds' points.

    Per batch element: reduce_i min_j |x_i - y_j|^2 (+ reduce_j min_i |y_j - x_i|^2 unless `single_directional`), with
    reduce = mean or sum over the cloud's points (`point_reduction`); `squared=False` uses the distances instead of their
    squares.  `batch_reduction`: "mean", "sum", or None for the (B,) values.  An empty cloud's term is 0.  The nearest
    neighbours are exact (the lowest row wins ties) and constants of the graph.  `reorder`: scan the targets in cell-grid
    order (True), as they come (False: good for image-ordered clouds), or the package default (None); same value either way.
    """
    _pair(x, y)
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of "mean", "sum". Got {0}.'.format(point_reduction))
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError('batch_reduction must be one of "mean", "sum", None. Got {0}.'.format(batch_reduction))
    sd2, sd, _, _, _ = ops.chamfer(x.points_padded, y.points_padded, x._counts_i32(), y._counts_i32(), float("inf"), _reorder(reorder))
    s = sd2 if squared else sd  # (B, 2)
    if point_reduction == "mean":
        s = s / torch.stack([_counts_f(x), _counts_f(y)], dim=1)
    out = s[:, 0] if single_directional else s[:, 0] + s[:, 1]
    if batch_reduction == "mean":
        return out.mean()
    if batch_reduction == "sum":
        return out.sum()
    return out


def _unpack(keys: torch.Tensor):
    valid = keys != ops.KEY_NONE
    d2 = torch.where(valid, keys >> 32, torch.zeros_like(keys)).to(torch.int32).view(torch.float32)
    idx = torch.where(valid, keys & 0xFFFFFFFF, torch.full_like(keys, -1))
    return d2, idx


def nearest_neighbor(x: Pointclouds, y: Pointclouds, reorder: Optional[bool] = None):
    """For every point of x its exact nearest point of y: (dist2 (B, Nx_max) fp32, idx (B, Nx_max) int64), padded.  idx is
    the row in y's cloud of the same batch element (the lowest row wins ties), -1 (with dist2 0) beyond x's count and for an
    empty y.  No gradient."""
    _pair(x, y)
    with torch.no_grad():
        _, keys_xy, _ = ops.chamfer_raw(x.points_padded, y.points_padded, x._counts_i32(), y._counts_i32(), float("inf"),
                                        _reorder(reorder))
    return _unpack(keys_xy)


def reconstruction_metrics(pred: Pointclouds, gt: Pointclouds, threshold: float, reorder: Optional[bool] = None) -> dict:
    """Evaluation figures of a reconstruction against ground truth, each a (B,) fp32 tensor, no gradient:
    accuracy (mean distance pred -> gt), completeness (mean distance gt -> pred), precision / recall (fraction of pred / gt
    points closer than `threshold` to the other cloud, strictly), fscore (their harmonic mean, 0 when both are 0), chamfer
    (mean squared distance, both directions added) and hausdorff (the largest distance of either direction)."""
    _pair(pred, gt, names=("pred", "gt"))
    t = torch.tensor(float(threshold), dtype=torch.float32)
    tau2 = float(t * t)  # the fp32 product, rounded once: what the kernel compares the fp32 squared distances with
    with torch.no_grad():
        stats, _, _ = ops.chamfer_raw(pred.points_padded, gt.points_padded, pred._counts_i32(), gt._counts_i32(), tau2,
                                      _reorder(reorder))
        n = torch.stack([pred._counts_i32(), gt._counts_i32()], dim=1).clamp(min=1).to(torch.float64)
        mean_d2, mean_d, frac = stats[..., 0] / n, stats[..., 1] / n, stats[..., 2] / n
        precision, recall = frac[:, 0], frac[:, 1]
        both = precision + recall
        fscore = torch.where(both > 0, 2 * precision * recall / both.clamp(min=1e-300), torch.zeros_like(both))
        out = {"accuracy": mean_d[:, 0], "completeness": mean_d[:, 1], "precision": precision, "recall": recall, "fscore": fscore,
               "chamfer": mean_d2[:, 0] + mean_d2[:, 1], "hausdorff": stats[..., 3].max(dim=1).values.float().sqrt()}
        return {k: v.float() for k, v in out.items()}
