"""GPU tests of the arena-backed sequence drivers (slam/sequence.py): the C calls a sequence makes and the workspaces it takes,
in order, as `ops.call` / `ops.workspace` see them -- the seam every call of the package goes through.  A call that bypassed
`ops`, a third call per frame, another workspace tag (the tag is part of the workspace's address, and the localisation's
captured graph is keyed on that address) or another order shows here.  The expected lists were recorded from the drivers as
they were before the frame loop was stated once (two copies of the loop, the taped calls spelled out inline)."""
import pytest
import torch

from tests.workspace_check import Watch, deterministic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


class Trace(Watch):
    """Watch that also keeps the order: ("call", entry) and ("ws", tag) as they happen."""

    def __init__(self, monkeypatch, gs):
        self.order = []
        super().__init__(monkeypatch, gs)

    def call(self, name, *args):
        self.order.append(("call", name))
        return super().call(name, *args)

    def workspace(self, nbytes, device, tag="default"):
        self.order.append(("ws", tag))
        return super().workspace(nbytes, device, tag)


def sequence(seed):
    """Three frames of 24 x 32: at dsratio 2 the localisation has 192 source points, three tiles, the last one partial."""
    from gradslam_amd.synthetic import make_sequence

    return [x.to(DEV) for x in make_sequence(1, 3, 24, 32, seed=seed)]


def streamed(gs, monkeypatch, cls, odom):
    slam = cls(odom=odom, dsratio=2, numiters=2, device=DEV)
    frames = gs.RGBDImages(*sequence(3))
    t = Trace(monkeypatch, gs)
    with torch.no_grad():
        slam(frames)
    return t.order


def one_node(gs, monkeypatch, det):
    slam = gs.slam.PointFusion(odom="gradicp", dsratio=2, numiters=2, device=DEV)
    leaves = [x.clone().requires_grad_(True) for x in sequence(5)]
    t = Trace(monkeypatch, gs)
    with deterministic(det):
        pcs, poses = slam(gs.RGBDImages(*leaves))
        forward = len(t.order)
        (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.sum()).backward()
    assert all(x.grad is not None and torch.isfinite(x.grad).all() for x in leaves)
    return t.order[:forward], t.order[forward:]


def step(update, ws):
    return [("ws", ws), ("call", update)]


LOCALIZE = [("ws", "localize"), ("call", "gs_slam_localize")]
STREAMED = {
    "pointfusion_icp": step("gs_pointfusion_update", "fusion_step") + 2 * (LOCALIZE + step("gs_pointfusion_update", "fusion_step")),
    "icpslam_gradicp": step("gs_aggregate_update", "aggregate_step") + 2 * (LOCALIZE + step("gs_aggregate_update", "aggregate_step")),
}
TAPED_UPDATE = step("gs_pointfusion_update_taped", "fusion_step")
NODE_FORWARD = TAPED_UPDATE + 2 * ([("call", "gs_vertex_normal_maps"), ("ws", "localize"), ("call", "gs_slam_localize_taped")]
                                   + TAPED_UPDATE)


def node_backward(det):
    maps = step("gs_vertex_normal_maps_backward" + det, "maps_bwd" + det)
    frame = step("gs_pointfusion_update_backward", "fusion_bwd") + maps
    localized = frame + step("gs_slam_localize_backward" + det, "localize_bwd" + det) + maps
    return 2 * localized + frame  # frames 2, 1, 0


@pytest.mark.parametrize("which", sorted(STREAMED))
def test_streamed_call_trace(gs, monkeypatch, which):
    cls = gs.slam.PointFusion if which.startswith("pointfusion") else gs.slam.ICPSLAM
    got = streamed(gs, monkeypatch, cls, which.split("_")[1])
    print(which, got)
    assert got == STREAMED[which]


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
def test_one_node_call_trace(gs, monkeypatch, det):
    forward, backward = one_node(gs, monkeypatch, det)
    print("forward", forward)
    print("backward", backward)
    assert forward == NODE_FORWARD
    assert backward == node_backward("_det" if det else "")
