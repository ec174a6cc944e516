"""The loops' association kernel with eight waves per block against sixteen (gs_set_loop_waves): everything a loop writes --
pose, trace rows, the last neighbour keys, the partial rows and the state in the workspace, the whole tape (every launch's
cloud and neighbour keys, every step's record) and the taped path's gradients -- must be the same bit for bit.  The neighbour
is a minimum over packed (distance, index) keys whoever finds it, and the 29 sums keep their row groups and their order.

gs_set_loop_waves: 0 = automatic, 8, 16; any other value is IGNORED (the setting stays what it was); the call returns the
setting in force.  Which super-boxes a straggler search lists depends on the order in which the waves improve a bound, so
gs_loop_counts' overflow counter (slot 3) may differ between wave counts and is not compared.

Scenes whose lanes must take the exact search are made so by geometry, not by inspection: a source point half a metre in
front of the wall has no target within the proof's bound (at most 1.5 pixel pitches of ~30 mm at 2 m), so its window best can
never be proven and the lane is in `need`: twenty such lanes per tile force the tile-level box search (more than six), three
per tile the point-serial one (one to six)."""
import ctypes

import pytest
import torch


def _lib():
    from gradslam_amd import _native

    return _native.lib()


def test_set_loop_waves_contract():
    """CPU: 0 / 8 / 16 are taken, anything else is ignored and the setting in force is returned."""
    lib = _lib()
    try:
        assert lib.gs_set_loop_waves(8) == 8
        assert lib.gs_set_loop_waves(16) == 16
        for bad in (4, 12, 32, -1, 7, 1 << 20):
            assert lib.gs_set_loop_waves(bad) == 16, bad
        assert lib.gs_set_loop_waves(8) == 8
        assert lib.gs_set_loop_waves(3) == 8
    finally:
        assert lib.gs_set_loop_waves(0) == 0
    assert lib.gs_set_loop_waves(5) == 0


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import gradslam_amd

    return gradslam_amd


DEV = "cuda:0"


class Hints(ctypes.Structure):
    _fields_ = [("scan_points", ctypes.c_void_p), ("scan_orig", ctypes.c_void_p), ("src_pix", ctypes.c_void_p),
                ("pix_start", ctypes.c_void_p), ("tgt_pix", ctypes.c_void_p), ("grid_w", ctypes.c_int32), ("grid_h", ctypes.c_int32),
                ("cam_pose", ctypes.c_void_p), ("cam_K", ctypes.c_void_p), ("ds", ctypes.c_int32)]


def _counts(lib, reset=False):
    out = (ctypes.c_uint * 4)()
    assert lib.gs_loop_counts(out, 1 if reset else 0) == 0
    return list(out)


def _with_arg16(fn, typ, body):
    old = list(fn.argtypes)
    fn.argtypes = old[:16] + [typ] + old[17:]
    try:
        return body()
    finally:
        fn.argtypes = old


def run_loops(gs, sc, numiters=6, grad_lm=0, hints=True, thresh=-1.0, ns_dev=None, rows_fill=0):
    """One plain and one taped loop through the C ABI on fresh zeroed buffers -> everything they wrote, on the host.
    thresh: the squared-distance threshold (negative: none).  ns_dev: the device count, at most the capacity src.shape[0]
    (None: the capacity).  rows_fill: the byte both partial-row regions of the workspaces hold at the start -- they and
    nothing else (the regions that carry indices must not hold junk)."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    lib = nv.lib()
    src, tgt, nrm = sc["src"], sc["tgt"], sc["nrm"]
    ns, nt = src.shape[0], tgt.shape[0]
    h = None
    if hints:
        h = Hints(sc["scan_points"].data_ptr(), sc["scan_orig"].data_ptr(), sc["src_pix"].data_ptr(), sc["pix_start"].data_ptr(),
                  sc["tgt_pix"].data_ptr() if sc.get("tgt_pix") is not None else None, sc["Wd"], sc["Hd"],
                  sc["cam_pose"].data_ptr(), sc["cam_K"].data_ptr(), sc["ds"])
    hp = ctypes.byref(h) if h is not None else None
    T0 = torch.eye(4, device=DEV)
    assert ns_dev is None or 0 < ns_dev <= ns
    d_ns, d_nt = ops.dev_int(ns if ns_dev is None else ns_dev, DEV), ops.dev_int(nt, DEV)
    b, t, rows = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.gs_icp_launch_geometry(ns, 1, ctypes.byref(b), ctypes.byref(t), ctypes.byref(rows)) == 0
    al = lambda x: (x + 255) // 256 * 256
    # icp.hip icp_ws_layout: state x 2 | clouds x 2 | neighbour keys x 2 | partial rows x 2 | ...
    part0 = 2 * al(348) + 2 * al(ns * 12) + 2 * al(ns * 8)
    ws_head = part0 + 2 * al(rows.value * 29 * 4)
    out = {"blocks": b.value}
    ws_n = nv.ws_bytes("gs_icp_ws_bytes", ns, nt)
    assert ws_head < ws_n
    # plain loop: pose, trace, last keys, workspace head (state, clouds, keys, partial rows)
    ws = torch.zeros(ws_n, dtype=torch.uint8, device=DEV)
    ws[part0:ws_head] = rows_fill
    T = torch.zeros(4, 4, device=DEV)
    best = torch.zeros(ns, dtype=torch.int64, device=DEV)
    trace = torch.zeros(numiters, 48, device=DEV)
    fnp = lib.gs_icp_point_to_plane_grad if grad_lm else lib.gs_icp_point_to_plane
    hint_pos = 15 if grad_lm else 11
    old = list(fnp.argtypes)
    fnp.argtypes = old[:hint_pos] + [ctypes.POINTER(Hints)] + old[hint_pos + 1:]
    try:
        args = [src.data_ptr(), d_ns.data_ptr(), ns, tgt.data_ptr(), nrm.data_ptr(), d_nt.data_ptr(), nt, T0.data_ptr(), numiters, 1e-8, thresh]
        if grad_lm:
            args += [2.0, 1.0, 1.0, 200.0]
        args += [hp, T.data_ptr(), best.data_ptr(), trace.data_ptr(), ws.data_ptr(), ws.numel(), nv.stream()]
        rc = fnp(*args)
    finally:
        fnp.argtypes = old
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    out.update(T=T.cpu(), best_last=best.cpu(), trace=trace.cpu(), ws_head=ws[:ws_head].cpu())
    # taped loop: the tape is the loop's working storage (every launch's cloud and keys, every step's record)
    ws = torch.zeros(ws_n, dtype=torch.uint8, device=DEV)
    ws[part0:ws_head] = rows_fill
    tape = torch.zeros(nv.ws_bytes("gs_icp_tape_bytes", ns, numiters, grad_lm), dtype=torch.uint8, device=DEV)
    T2 = torch.zeros(4, 4, device=DEV)
    best2 = torch.zeros(ns, dtype=torch.int64, device=DEV)
    fn = lib.gs_icp_point_to_plane_taped
    rc = _with_arg16(fn, ctypes.POINTER(Hints), lambda: fn(
        src.data_ptr(), d_ns.data_ptr(), ns, tgt.data_ptr(), nrm.data_ptr(), d_nt.data_ptr(), nt, T0.data_ptr(), numiters, 1e-8, thresh,
        grad_lm, 2.0, 1.0, 1.0, 200.0, hp, T2.data_ptr(), best2.data_ptr(), tape.data_ptr(), tape.numel(), ws.data_ptr(), ws.numel(),
        nv.stream()))
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    out.update(T_taped=T2.cpu(), best_last_taped=best2.cpu(), tape=tape.cpu(), partial_rows_taped=ws[part0:ws_head].cpu(),
               state_taped=ws[:2 * al(348)].cpu())
    return out


def both_waves(gs, fn):
    """fn() under eight and under sixteen waves; the setter is back at its default afterwards."""
    lib = gs._native.lib()
    res = {}
    try:
        for nw in (8, 16):
            assert lib.gs_set_loop_waves(nw) == nw
            res[nw] = fn()
    finally:
        assert lib.gs_set_loop_waves(0) == 0
    return res[8], res[16]


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k
    assert torch.isfinite(a["T"]).all() and not torch.equal(a["T"], torch.eye(4))


def grid_scene(**kw):
    from tests import test_gpu_parity as P  # the synthetic ds-grid scene of the grid-search tests

    return P._grid_scene(**kw)


def off_the_wall(sc, per_tile, tile_points=64):
    """`per_tile` lanes of every tile moved half a metre towards the camera: no target within the proof's bound."""
    src = sc["src"].clone()
    n = src.shape[0]
    for t0 in range(0, n - tile_points + 1, tile_points):
        src[t0 + 5: t0 + 5 + per_tile, 2] -= 0.5
    sc["src"] = src.contiguous()
    return sc


def check_scene(gs, sc, grid=True, hints=True, **kw):
    lib = gs._native.lib()
    _counts(lib, reset=True)
    a, b = both_waves(gs, lambda: run_loops(gs, sc, hints=hints, **kw))
    loops, grid_loops, forced_tiles, _ = _counts(lib)
    assert loops == 4 and grid_loops == (4 if grid else 0), (loops, grid_loops)
    assert_same(a, b)
    return a, forced_tiles


def c2_clouds(gs):
    """The bench's c2 clouds with their hints: the loop inputs gs_slam_localize leaves in its workspace (640 x 480, ds 4)."""
    from tests import test_fused_setup as F

    depth, K, prev, mp, mn, cnt = F.scene(gs, 480, 640)
    v = F.localize(gs, depth, K, prev, mp, mn, cnt, 4, 1, True)[5]
    ns, nt = int(v["ns"][0]), int(v["nt"][0])
    dev = lambda x: x.contiguous().to(DEV)
    return dict(src=dev(v["src"][:3 * ns].view(ns, 3)), src_pix=dev(v["src_pix"][:ns]), tgt=dev(v["tgt"][:3 * nt].view(nt, 3)),
                nrm=dev(v["tnrm"][:3 * nt].view(nt, 3)), scan_points=dev(v["scan"][:3 * nt].view(nt, 3)), scan_orig=dev(v["scan_orig"][:nt]),
                pix_start=dev(v["pix_start"]), tgt_pix=None, Wd=160, Hd=120, cam_pose=prev.reshape(4, 4).contiguous(),
                cam_K=K.reshape(4, 4).contiguous(), ds=4)


@pytest.mark.gpu
def test_loop_waves_c2_clouds(gs):
    sc = c2_clouds(gs)
    assert sc["src"].shape[0] > 15000 and sc["tgt"].shape[0] > 15000
    a, _ = check_scene(gs, sc, numiters=10)
    assert 256 < a["blocks"] <= 320  # more tiles than CUs: the launch the wave count is chosen for


@pytest.mark.gpu
def test_loop_waves_dense_target(gs):
    """~24 targets per pixel: a lane's window row (three pixels) holds more candidates than the block has waves, and three
    bands of 66 pixels overflow the 4096-entry pool (the band left out is read from memory)."""
    sc = grid_scene(seed=11, per_cell=48, Hd=60, Wd=80)
    per_pixel = sc["tgt"].shape[0] / (60 * 80)
    assert 3 * per_pixel > 16 and 3 * 66 * per_pixel > 4096, per_pixel
    check_scene(gs, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("per_tile", [20, 3])
def test_loop_waves_unproven_lanes(gs, per_tile):
    """20 lanes per tile without a proof: the tile-level box search; 3: the point-serial search (module docstring)."""
    check_scene(gs, off_the_wall(grid_scene(seed=12), per_tile))


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [33, 47])
def test_loop_waves_forced_tile_points(gs, tile):
    lib = gs._native.lib()
    lib.gs_set_tile_points(tile)
    try:
        _, forced = check_scene(gs, off_the_wall(grid_scene(seed=13, motion=0.02), 2, tile))
    finally:
        lib.gs_set_tile_points(0)
    assert forced == 4


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["grid_search_off", "no_hints"])
def test_loop_waves_chunk_box_variant(gs, how):
    sc = grid_scene(seed=14, motion=0.02)
    lib = gs._native.lib()
    if how == "grid_search_off":
        lib.gs_set_grid_search(0)
    try:
        check_scene(gs, sc, grid=False, hints=how != "no_hints")
    finally:
        lib.gs_set_grid_search(1)


@pytest.mark.gpu
def test_loop_waves_gradicp(gs):
    check_scene(gs, off_the_wall(grid_scene(seed=15, motion=0.01), 1), grad_lm=1)


@pytest.mark.gpu
def test_loop_waves_more_than_512_blocks(gs):
    """More tiles than the chip holds at once: the steps are launches of their own (not folded into the association)."""
    sc = grid_scene(seed=16, Hd=180, Wd=240, per_cell=2)
    a, _ = check_scene(gs, sc, numiters=4)
    assert a["blocks"] > 512


@pytest.mark.gpu
@pytest.mark.parametrize("odom", ["icp", "gradicp"])
def test_loop_waves_taped_gradients(gs, odom):
    from tests import test_fused_setup as F

    depth, K, prev, mp, mn, cnt = F.scene(gs, 240, 320, seed=5)
    lib = gs._native.lib()

    def run():
        gV = torch.zeros((1, 1, 240, 320, 3), dtype=torch.float32, device=depth.device)
        lib.gs_vertex_normal_maps(depth.data_ptr(), K.data_ptr(), prev.data_ptr(), 1, 1, 240, 320, None, None, gV.data_ptr(), None,
                                  torch.cuda.current_stream().cuda_stream)
        gV.requires_grad_(True)
        mpg, mng, pv = mp.clone().requires_grad_(True), mn.clone().requires_grad_(True), prev.clone().requires_grad_(True)
        out = gs.ops.slam_localize_autograd(gV, depth, K, pv, mpg, mng, cnt, 4, 10, 1e-8, 0.1,
                                            (2.0, 1.0, 1.0, 200.0) if odom == "gradicp" else None)
        (out * torch.arange(16, dtype=torch.float32, device=out.device).view(1, 1, 4, 4)).sum().backward()
        torch.cuda.synchronize()
        return [x.detach().cpu() for x in (out, gV.grad, mpg.grad, mng.grad, pv.grad)]

    # (the default reverse pass scatters with atomics in arrival order: its bits differ from run to run whatever the wave
    # count; under torch's flag the gradients are a pure function of what the forward pass taped)
    _counts(lib, reset=True)
    old = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a, b = both_waves(gs, run)
    finally:
        torch.use_deterministic_algorithms(old)
    assert _counts(lib)[:2] == [2, 2]
    for x, y in zip(a, b):
        assert torch.equal(x, y) and torch.isfinite(x).all()
    assert a[2].abs().sum() > 0
