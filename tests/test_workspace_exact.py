"""GPU tests: every entry point whose workspace layout is one `*_layout` function stays inside a workspace of EXACTLY the
queried size, and refuses one byte less.

Each case makes its call the way the package does -- through `ops`, whose `call` / `ptr` / `workspace` are watched here, or, for
the three entries `ops` has no wrapper for, in `ops`' words -- which gives the reference run: the roomy workspace of the cache,
rounded up to a power of two.  The recorded call is then issued again through `_native.call`, argument for argument, with
  * the cached workspace again, on outputs filled with 0x5A (the reference bits),
  * a workspace of exactly the queried size, 4096 bytes into a buffer of 0xA5 with 4096 more behind it: every guard byte must
    survive and, for entries without float atomics, every output must carry the reference's bits (whole buffers: what a
    kernel leaves unwritten keeps the fill in both runs),
  * one byte less: RuntimeError "workspace too small", code -2, outputs still 0x5A.
An overrun of less than 4 KiB is caught here without leaving the allocation; a size that drifts is tests/test_ws_sizes.py's.
The slot order inside a ds-grid pixel is the order its rows arrive in (an atomic counter), so the scan order of the two
bucketing entries is compared by test_icp_target_build.py's set comparison, not bitwise here."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


class Watch:
    """ops.call / ops.ptr / ops.workspace while a case runs: the calls made, the tensors behind their pointers (kept alive),
    the size each workspace was asked for."""

    def __init__(self, monkeypatch, gs):
        self.nv, self.calls, self.tensors, self.asked = gs._native, [], {}, {}
        monkeypatch.setattr(gs.ops, "call", self.call)
        monkeypatch.setattr(gs.ops, "ptr", self.ptr)
        monkeypatch.setattr(gs.ops, "workspace", self.workspace)

    def call(self, name, *args):
        self.calls.append((name, args))
        return self.nv.call(name, *args)

    def ptr(self, t):
        if t is not None:
            self.tensors[t.data_ptr()] = t
        return self.nv.ptr(t)

    def workspace(self, nbytes, device, tag="default"):
        ws = self.nv.workspace(nbytes, device, tag)
        self.asked[ws.data_ptr()] = int(nbytes)
        return ws


def _bytes(t):
    return t.reshape(-1).view(torch.uint8)


def check_exact(gs, monkeypatch, entry, run, outs, bitwise=True, fill=0x5A, compare=None):
    """`run()` makes one call of `entry` (see the module docstring); `outs` are the positions of its output arguments, or the
    output tensors themselves; `compare` the subset that is compared bitwise (default: all); `fill` what the outputs hold
    before a run (0 for entries that add into them)."""
    nv = gs._native
    w = Watch(monkeypatch, gs)
    run()
    made = [args for name, args in w.calls if name == entry]
    assert len(made) == 1, (entry, [name for name, _ in w.calls])
    args = made[0]
    ws_ptr, ws_have, need = args[-3], args[-2], w.asked[args[-3]]
    assert need <= ws_have
    resolve = lambda which: [w.tensors[args[o]] if isinstance(o, int) else o for o in which if not isinstance(o, int) or args[o] is not None]
    tensors = resolve(outs)
    compared = tensors if compare is None else resolve(compare)
    assert tensors and all(t.is_contiguous() for t in tensors)

    def again(ws, nbytes, value):
        for t in tensors:
            _bytes(t).fill_(value)
        nv.call(entry, *args[:-3], ws, nbytes, args[-1])
        torch.cuda.synchronize()
        return [_bytes(t).clone() for t in compared]

    ref = again(ws_ptr, ws_have, fill)
    buf = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    got = again(buf.data_ptr() + GUARD, need, fill)
    assert bool((buf[:GUARD] == 0xA5).all()), entry + ": wrote in front of its workspace"
    assert bool((buf[GUARD + need:] == 0xA5).all()), entry + ": wrote behind its workspace"
    if bitwise:
        for k, (r, g) in enumerate(zip(ref, got)):
            assert torch.equal(r, g), (entry, "output", k)
            assert fill != 0x5A or not bool((g == 0x5A).all()), (entry, "output", k, "was never written")
        assert any(bool((g != fill).any()) for g in got), (entry, "wrote nothing")
    with pytest.raises(RuntimeError) as e:
        again(buf.data_ptr() + GUARD, need - 1, 0x5A)
    assert "workspace too small" in str(e.value) and "code -2" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert all(bool((_bytes(t) == 0x5A).all()) for t in tensors), entry + ": a refused call wrote to its outputs"


@contextlib.contextmanager
def deterministic(on):
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before)


def frames(gs, B, L, H, W):
    """depth (B,L,H,W,1), rgb (B,L,H,W,3), K (B,1,4,4), poses (B,L,4,4) and the maps of all frames, on the device."""
    from gradslam_amd.synthetic import make_sequence

    c, d, K, P = (x.to(DEV).contiguous() for x in make_sequence(B, L, H, W, seed=0))
    V, N, gV, gN = gs.ops.vertex_normal_maps_raw(d, K, P)
    return dict(rgb=c, depth=d, K=K, P=P, V=V, N=N, gV=gV, gN=gN)


def valid_points(f, b, l):
    """(points, normals) of frame l of sequence b in world coordinates: the pixels with a depth and a normal."""
    ok = (f["depth"][b, l, ..., 0] > 0) & (f["gN"][b, l].abs().sum(-1) > 0)
    return f["gV"][b, l][ok].contiguous(), f["gN"][b, l][ok].contiguous()


# ------------------------------------------------------------------ ICP loops: 65 source points (two tiles, the second with one
# lane), 130 target points, 2 iterations
@pytest.fixture(scope="module")
def clouds(gs):
    f = frames(gs, 1, 2, 24, 32)
    tgt, nrm = valid_points(f, 0, 0)
    src, _ = valid_points(f, 0, 1)
    assert tgt.shape[0] >= 130 and src.shape[0] >= 65
    T0 = torch.eye(4, device=DEV)
    T0[0, 3] = 0.004
    return src[:65].contiguous(), tgt[:130].contiguous(), nrm[:130].contiguous(), T0


GRAD = (None, (2.0, 1.0, 1.0, 200.0))  # grad_lm 0 and 1


@pytest.mark.parametrize("grad", GRAD, ids=["lm", "gradlm"])
def test_icp_loop(gs, monkeypatch, clouds, grad):
    src, tgt, nrm, T0 = clouds
    entry, first = ("gs_icp_point_to_plane", 12) if grad is None else ("gs_icp_point_to_plane_grad", 16)
    run = lambda: gs.ops.icp_device_loop(src, tgt, nrm, T0, 2, 1e-8, 0.5, grad, want_trace=True, want_best=True)
    check_exact(gs, monkeypatch, entry, run, outs=[first, first + 1, first + 2])


def _icp_autograd(gs, clouds, grad, det):
    src, tgt, nrm, T0 = (x.clone().requires_grad_(True) for x in clouds)
    with deterministic(det):
        T, _ = gs.ops.icp_loop_autograd(src, tgt, nrm, T0, 2, 1e-8, 0.5, grad)
        (T * torch.arange(16.0, device=DEV).view(4, 4)).sum().backward()


@pytest.mark.parametrize("grad", GRAD, ids=["lm", "gradlm"])
def test_icp_loop_taped(gs, monkeypatch, clouds, grad):
    """(the tape, allocated at exactly gs_icp_tape_bytes, is one of the outputs: compared whole)"""
    check_exact(gs, monkeypatch, "gs_icp_point_to_plane_taped", lambda: _icp_autograd(gs, clouds, grad, False), outs=[17, 18, 19])


@pytest.mark.parametrize("grad", GRAD, ids=["lm", "gradlm"])
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
def test_icp_loop_backward(gs, monkeypatch, clouds, grad, det):
    entry = "gs_icp_point_to_plane_backward" + ("_det" if det else "")
    check_exact(gs, monkeypatch, entry, lambda: _icp_autograd(gs, clouds, grad, det), outs=[18, 19, 20, 21], bitwise=det)


# ------------------------------------------------------------------ table and frame entries: 12 x 16, ds 2, B = 2, Nmax 70
@pytest.fixture(scope="module")
def table(gs):
    B, H, W, Nmax = 2, 12, 16, 70
    f = frames(gs, B, 2, H, W)
    mp, mn = torch.zeros(B, Nmax, 3, device=DEV), torch.zeros(B, Nmax, 3, device=DEV)
    counts = torch.tensor([70, 50], dtype=torch.int32, device=DEV)
    for b in range(B):
        p, n = valid_points(f, b, 0)
        assert p.shape[0] >= Nmax
        mp[b], mn[b] = p[:Nmax], n[:Nmax]
    f.update(B=B, H=H, W=W, Nmax=Nmax, mp=mp, mn=mn, counts=counts, cc=torch.ones(B, Nmax, 1, device=DEV))
    return f


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


def test_fusion_unique(gs, monkeypatch, table):
    t = table
    rows, cnt = _rows(gs, t, 0)
    gV = t["gV"][:, 1:2].contiguous()
    run = lambda: gs.ops.fusion_unique_raw(rows, None, cnt, t["B"] * t["Nmax"], gV, t["mp"], t["cc"])
    check_exact(gs, monkeypatch, "gs_fusion_unique", run, outs=[11, 12])


def test_downsample_frame(gs, monkeypatch, table):
    t = table
    d, gV, gN, rgb = (t[k][:, 1:2].contiguous() for k in ("depth", "gV", "gN", "rgb"))
    check_exact(gs, monkeypatch, "gs_downsample_frame", lambda: gs.ops.downsample_frame_raw(d, gV, gN, rgb, 2), outs=[9, 10, 11, 13])


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
