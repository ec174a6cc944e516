"""GPU tests: the ICP loops and their reverse passes, the projection, the bucketing entries, fusion_unique, the frame intake,
append_rows, the maps' reverse pass and gs_slam_localize stay inside a workspace of EXACTLY the queried size, whatever bytes
it holds, and refuse one byte less.  The other entry points that take (ws, ws_bytes) are tests/test_workspace_exact_families.py's,
which also holds the list of both files' cases to the header; the harness (what a case runs and what is compared) is
tests/workspace_check.py's docstring.

A size that drifts is tests/test_ws_sizes.py's.  The slot order inside a ds-grid pixel is the order its rows arrive in (an
atomic counter), so the scan order of the two bucketing entries is compared by test_icp_target_build.py's set comparison, not
bitwise here.  Not bitwise either (float atomics into the compared outputs): gs_vertex_normal_maps_backward and
gs_icp_point_to_plane_backward; their `_det` twins are."""
import ctypes

import pytest
import torch

from tests import workspace_check
from tests.workspace_check import DEV, check_exact, deterministic, frames, make_clouds, make_table, valid_points

covers = lambda *entries: workspace_check.covers(__name__, *entries)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ------------------------------------------------------------------ ICP loops: 65 source points (two tiles, the second with one
# lane), 130 target points, 2 iterations
@pytest.fixture(scope="module")
def clouds(gs):
    return make_clouds(gs, 65, 130)


def big_clouds(gs, held=[]):
    """The `dirty=` shape of the loops' cases: 131 sources, 261 targets (built once)."""
    if not held:
        held.append(make_clouds(gs, 131, 261))
    return held[0]


GRAD = (None, (2.0, 1.0, 1.0, 200.0))  # grad_lm 0 and 1


@covers("gs_icp_point_to_plane", "gs_icp_point_to_plane_grad")
@pytest.mark.parametrize("grad", GRAD, ids=["lm", "gradlm"])
def test_icp_loop(gs, monkeypatch, clouds, grad):
    src, tgt, nrm, T0 = clouds
    entry, first = ("gs_icp_point_to_plane", 12) if grad is None else ("gs_icp_point_to_plane_grad", 16)
    run = lambda: gs.ops.icp_device_loop(src, tgt, nrm, T0, 2, 1e-8, 0.5, grad, want_trace=True, want_best=True)
    dirty = lambda: gs.ops.icp_device_loop(*big_clouds(gs), 2, 1e-8, 0.5, grad)
    check_exact(gs, monkeypatch, entry, run, outs=[first, first + 1, first + 2], dirty=dirty)


def _icp_autograd(gs, clouds, grad, det):
    src, tgt, nrm, T0 = (x.clone().requires_grad_(True) for x in clouds)
    with deterministic(det):
        T, _ = gs.ops.icp_loop_autograd(src, tgt, nrm, T0, 2, 1e-8, 0.5, grad)
        (T * torch.arange(16.0, device=DEV).view(4, 4)).sum().backward()


@covers("gs_icp_point_to_plane_taped")
@pytest.mark.parametrize("grad", GRAD, ids=["lm", "gradlm"])
def test_icp_loop_taped(gs, monkeypatch, clouds, grad):
    """(the tape, at exactly gs_icp_tape_bytes between guards of its own, is one of the outputs: compared whole)"""
    check_exact(gs, monkeypatch, "gs_icp_point_to_plane_taped", lambda: _icp_autograd(gs, clouds, grad, False), outs=[17, 18], tape=19,
                tape_out=True, dirty=lambda: _icp_autograd(gs, big_clouds(gs), grad, False))


@covers("gs_icp_point_to_plane_backward", "gs_icp_point_to_plane_backward_det")
@pytest.mark.parametrize("grad", GRAD, ids=["lm", "gradlm"])
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
def test_icp_loop_backward(gs, monkeypatch, clouds, grad, det):
    entry = "gs_icp_point_to_plane_backward" + ("_det" if det else "")
    check_exact(gs, monkeypatch, entry, lambda: _icp_autograd(gs, clouds, grad, det), outs=[18, 19, 20, 21], bitwise=det, tape=15,
                dirty=lambda: _icp_autograd(gs, big_clouds(gs), grad, det))


# ------------------------------------------------------------------ table and frame entries: 12 x 16, ds 2, B = 2, Nmax 70
@pytest.fixture(scope="module")
def table(gs):
    return make_table(gs, 12, 16, 70, (70, 50))


@covers("gs_project_active")
@pytest.mark.parametrize("B", [1, 33], ids=["lds_cameras", "camera_launch"])  # kCamB = 32 cameras fit the block's LDS
def test_project_active(gs, monkeypatch, table, B):
    t = table
    pick = torch.arange(B, device=DEV) % t["B"]
    pts, counts = t["mp"][pick].contiguous(), t["counts"][pick].contiguous()
    poses, K = t["P"][pick, 1].contiguous(), t["K"][pick, 0].contiguous()
    run = lambda: gs.ops.project_active_raw(pts, counts, poses, K, t["H"], t["W"], 2)
    check_exact(gs, monkeypatch, "gs_project_active", run, outs=[9, 10])


def _rows(gs, t, ds):
    rows, cnt = gs.ops.project_active_raw(t["mp"], t["counts"], t["P"][:, 1].contiguous(), t["K"][:, 0].contiguous(), t["H"], t["W"], ds)
    assert 0 < int(cnt) <= t["B"] * t["Nmax"]
    return rows, cnt


def _target_outputs(t, cap, npix):
    B = t["B"]
    mk = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    return dict(tgt=mk(B, cap, 3), tnrm=mk(B, cap, 3), counts=mk(B, dtype=torch.int32), scan=mk(B, cap, 3),
                scan_orig=mk(B, cap, dtype=torch.int32), pix_start=mk(B, npix + 1, dtype=torch.int32),
                tgt_index=mk(B, cap, dtype=torch.int32), tgt_pix=mk(B, cap, dtype=torch.int32))


@covers("gs_bucket_by_pixel")
def test_bucket_by_pixel(gs, monkeypatch, table):
    t, ops, ds = table, gs.ops, 2
    B, H, W, Nmax = t["B"], t["H"], t["W"], t["Nmax"]
    rows, cnt = _rows(gs, t, ds)
    o = _target_outputs(t, Nmax, (H // ds) * (W // ds))

    def run():
        ws = ops.workspace(ops.ws_bytes("gs_bucket_by_pixel_ws_bytes", B, H, W, ds), DEV, "bucket")
        ops.call("gs_bucket_by_pixel", ops.ptr(rows), ops.ptr(cnt), B * Nmax, B, H, W, ds, ops.ptr(t["mp"]), Nmax, Nmax, ops.ptr(o["scan"]),
                 ops.ptr(o["scan_orig"]), ops.ptr(o["pix_start"]), ops.ptr(o["tgt_pix"]), ops.ptr(ws), ws.numel(), ops.stream())

    check_exact(gs, monkeypatch, "gs_bucket_by_pixel", run, outs=[10, 11, 12, 13], compare=[12, 13])


@covers("gs_build_icp_target")
def test_build_icp_target(gs, monkeypatch, table):
    t, ops, ds = table, gs.ops, 2
    B, H, W, Nmax = t["B"], t["H"], t["W"], t["Nmax"]
    rows, cnt = _rows(gs, t, ds)
    o = _target_outputs(t, Nmax, (H // ds) * (W // ds))

    def run():
        ws = ops.workspace(ops.ws_bytes("gs_build_icp_target_ws_bytes", B, H, W, ds), DEV, "bucket")
        ops.call("gs_build_icp_target", ops.ptr(rows), ops.ptr(cnt), B * Nmax, B, H, W, ds, ops.ptr(t["mp"]), ops.ptr(t["mn"]), Nmax, Nmax,
                 ops.ptr(o["tgt"]), ops.ptr(o["tnrm"]), ops.ptr(o["counts"]), ops.ptr(o["scan"]), ops.ptr(o["scan_orig"]),
                 ops.ptr(o["pix_start"]), ops.ptr(o["tgt_index"]), ops.ptr(o["tgt_pix"]), ops.ptr(ws), ws.numel(), ops.stream())

    check_exact(gs, monkeypatch, "gs_build_icp_target", run, outs=list(range(11, 19)), compare=[11, 12, 13, 16, 17, 18])


@covers("gs_fusion_unique")
def test_fusion_unique(gs, monkeypatch, table):
    t = table
    rows, cnt = _rows(gs, t, 0)
    gV = t["gV"][:, 1:2].contiguous()
    run = lambda: gs.ops.fusion_unique_raw(rows, None, cnt, t["B"] * t["Nmax"], gV, t["mp"], t["cc"])
    check_exact(gs, monkeypatch, "gs_fusion_unique", run, outs=[11, 12])


@covers("gs_downsample_frame")
def test_downsample_frame(gs, monkeypatch, table):
    t = table
    d, gV, gN, rgb = (t[k][:, 1:2].contiguous() for k in ("depth", "gV", "gN", "rgb"))
    check_exact(gs, monkeypatch, "gs_downsample_frame", lambda: gs.ops.downsample_frame_raw(d, gV, gN, rgb, 2), outs=[9, 10, 11, 13])


@covers("gs_append_rows")
def test_append_rows(gs, monkeypatch, table):
    """One frame's valid pixels (arrays of width 3 and 1) appended to an arena.  The arena, its count and the two counters are
    the outputs: they start from the fill -- an empty arena for the compared runs, where every selected row lands -- and a
    refused call leaves all of them as they were."""
    t, ops = table, gs.ops
    n, cap = t["H"] * t["W"], t["Nmax"] + t["H"] * t["W"]
    a, b = t["gV"][1, 1].reshape(n, 3).contiguous(), t["depth"][1, 1].reshape(n, 1).contiguous()
    mask = (b[:, 0] > 0).to(torch.uint8)
    dst_a, dst_b = torch.zeros(cap, 3, device=DEV), torch.zeros(cap, 1, device=DEV)
    count, appended, overflow = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(3))
    src = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    dst = (ctypes.c_void_p * 2)(dst_a.data_ptr(), dst_b.data_ptr())
    widths = (ctypes.c_int * 2)(3, 1)

    def run():
        ws = ops.workspace(ops.ws_bytes("gs_append_rows_ws_bytes", n), DEV, "append")
        ops.call("gs_append_rows", 2, src, widths, dst, ops.ptr(mask), n, ops.ptr(count), cap, ops.ptr(appended), ops.ptr(overflow),
                 ops.ptr(ws), ws.numel(), ops.stream())

    assert int(mask.sum()) > 0
    check_exact(gs, monkeypatch, "gs_append_rows", run, outs=[dst_a, dst_b, 6, 8, 9], fill=0)


# ------------------------------------------------------------------ the maps' reverse pass: B = 1, L = 2, 9 x 11
@covers("gs_vertex_normal_maps_backward", "gs_vertex_normal_maps_backward_det")
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
def test_vertex_normal_maps_backward(gs, monkeypatch, det):
    f = frames(gs, 1, 2, 9, 11)
    g = [torch.randn(1, 2, 9, 11, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(k)) for k in range(4)]

    def run():
        with deterministic(det):
            gs.ops.vertex_normal_maps_backward_raw(f["depth"], f["K"], f["P"], *g)

    # (the kernels ADD into the three adjoints: they start from zero)
    check_exact(gs, monkeypatch, "gs_vertex_normal_maps_backward" + ("_det" if det else ""), run, outs=[11, 12, 13], bitwise=det, fill=0)


# ------------------------------------------------------------------ gs_slam_localize: 24 x 32, ds 2, 2 iterations
@covers("gs_slam_localize")
@pytest.mark.parametrize("fused", [1, 0], ids=["fused_front", "separate_front"])
def test_slam_localize(gs, monkeypatch, fused):
    """Both carvings of the front end's share of the workspace: project_front1 (fused) and project_target1."""
    f = frames(gs, 1, 2, 24, 32)
    mp, mn = (x.unsqueeze(0).contiguous() for x in valid_points(f, 0, 0))
    counts = torch.tensor([mp.shape[1]], dtype=torch.int32, device=DEV)
    depth, prev = f["depth"][:, 1:2].contiguous(), f["P"][:, :1].contiguous()
    lib = gs._native.lib()
    lib.gs_set_fused_setup(fused)
    try:
        run = lambda: gs.ops.slam_localize_raw(depth, f["K"], prev, mp, mn, counts, 2, 2, 1e-8, 0.1)
        check_exact(gs, monkeypatch, "gs_slam_localize", run, outs=[19, 20, 21, 23])
    finally:
        lib.gs_set_fused_setup(1)
