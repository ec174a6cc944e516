"""gs_slam_localize's fused front end (gs_set_fused_setup, default on) against the separate chain it replaces (off): the loop's
inputs in the workspace, the pose, the maps and the taped path's gradients must be the same bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import gradslam_amd

    return gradslam_amd


def cdiv(a, b):
    return -(-a // b)


def target_cap(nmax):
    c = 1024
    while c < nmax and c < (1 << 30):
        c <<= 1
    return c


def front_views(ws, H, W, ds, Nmax):
    """The loop's inputs in a gs_slam_localize workspace (B = 1; slam.hip loc_layout, in its order)."""
    capS, capT = cdiv(H, ds) * cdiv(W, ds), target_cap(Nmax)
    off, v = 0, {}

    def take(name, nbytes, dtype):
        nonlocal off
        if name:
            v[name] = ws[off:off + nbytes].view(dtype)
        off += cdiv(nbytes, 256) * 256

    take("src", capS * 12, torch.float32); take("ns", 4, torch.int32); take("src_pix", capS * 4, torch.int32)
    take("scan", capT * 12, torch.float32); take("scan_orig", capT * 4, torch.int32)
    take("pix_start", (capS + 1) * 4, torch.int32); take(None, capT * 32, torch.uint8); take(None, 4, torch.uint8)
    take("tgt", capT * 12, torch.float32); take("tnrm", capT * 12, torch.float32); take("nt", 4, torch.int32)
    return {k: t.clone().cpu() for k, t in v.items()}


def scene(gs, H, W, seed=0):
    from gradslam_amd.synthetic import make_sequence

    dev = torch.device("cuda:0")
    c, d, K, P = make_sequence(1, 2, H, W, seed=seed)
    pf = gs.slam.PointFusion(odom="gt", device=dev)
    with torch.no_grad():
        pcs, _ = pf(gs.RGBDImages(c[:, :1].to(dev), d[:, :1].to(dev), K.to(dev), P[:, :1].to(dev)))
    mp = pcs.points_padded.contiguous()
    mn = pcs.normals_padded.contiguous()
    cnt = pcs.num_points_per_pointcloud.to(torch.int32).contiguous()
    return d[:, 1:2].to(dev).contiguous(), K.to(dev).contiguous(), P[:, :1].to(dev).contiguous(), mp, mn, cnt


def localize(gs, depth, K, prev, mp, mn, cnt, ds, numiters, fused, ws=None):
    lib = gs._native.lib()
    lib.gs_set_fused_setup(1 if fused else 0)
    try:
        B, _, H, W = depth.shape[:4]
        Nmax = mp.shape[1]
        dev = depth.device
        if ws is None:
            ws = torch.zeros(lib.gs_slam_localize_ws_bytes(B, H, W, ds, Nmax), dtype=torch.uint8, device=dev)
        mk = lambda: torch.empty((B, 1, H, W, 3), dtype=torch.float32, device=dev)
        V, N, gV, gN = mk(), mk(), mk(), mk()
        out = torch.empty((B, 1, 4, 4), dtype=torch.float32, device=dev)
        p = lambda x: x.data_ptr()
        rc = lib.gs_slam_localize(p(depth), p(K), p(prev), B, H, W, ds, p(mp), p(mn), p(cnt), Nmax, 0, numiters, 1e-8, 0.1,
                                  2.0, 1.0, 1.0, 200.0, p(V), p(N), p(gV), p(gN), p(out), p(ws), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.gs_last_error()
        torch.cuda.synchronize()
        return out.cpu(), V.cpu(), N.cpu(), gV.cpu(), gN.cpu(), front_views(ws, H, W, ds, Nmax)
    finally:
        lib.gs_set_fused_setup(1)


def assert_fronts_equal(a, b):
    ns, nt = int(a["ns"][0]), int(a["nt"][0])
    assert int(b["ns"][0]) == ns and int(b["nt"][0]) == nt
    assert torch.equal(a["src"][:3 * ns], b["src"][:3 * ns]) and torch.equal(a["src_pix"][:ns], b["src_pix"][:ns])
    assert torch.equal(a["tgt"][:3 * nt], b["tgt"][:3 * nt]) and torch.equal(a["tnrm"][:3 * nt], b["tnrm"][:3 * nt])
    assert torch.equal(a["pix_start"], b["pix_start"])
    start = a["pix_start"].numpy()
    tgt = a["tgt"][:3 * nt].view(-1, 3)
    for v in (a, b):  # every slot holds the target row it names; per bucket the same rows (arrival order inside one)
        orig = v["scan_orig"][:nt].long()
        assert torch.equal(v["scan"][:3 * nt].view(-1, 3), tgt[orig])
    oa, ob = a["scan_orig"][:nt].numpy(), b["scan_orig"][:nt].numpy()
    for q in np.nonzero(start[1:] - start[:-1])[0]:
        s0, s1 = start[q], start[q + 1]
        assert np.array_equal(np.sort(oa[s0:s1]), np.sort(ob[s0:s1])), q
    return ns, nt


def check_both(gs, depth, K, prev, mp, mn, cnt, ds, numiters=10):
    on = localize(gs, depth, K, prev, mp, mn, cnt, ds, numiters, True)
    off = localize(gs, depth, K, prev, mp, mn, cnt, ds, numiters, False)
    for x, y in zip(on[:5], off[:5]):
        assert torch.equal(x, y)
    return assert_fronts_equal(on[5], off[5])


def test_fused_setup_bench_like_scene(gs):
    ns, nt = check_both(gs, *scene(gs, 240, 320), 4)
    assert ns > 1000 and nt > 1000


def test_fused_setup_grid_not_divisible(gs):
    ns, nt = check_both(gs, *scene(gs, 122, 158, seed=3), 4)
    assert ns > 0 and nt > 0


def test_fused_setup_empty_map(gs):
    depth, K, prev, mp, mn, cnt = scene(gs, 120, 160, seed=1)
    ns, nt = check_both(gs, depth, K, prev, mp, mn, torch.zeros_like(cnt), 4)
    assert nt == 0


def test_fused_setup_nothing_in_view(gs):
    depth, K, prev, mp, mn, cnt = scene(gs, 120, 160, seed=2)
    behind = mp.clone()
    behind[..., 2] = -behind[..., 2] - 5.0  # every map point behind the camera
    ns, nt = check_both(gs, depth, K, prev, behind, mn, cnt, 4)
    assert nt == 0 and ns > 0


def test_fused_setup_growing_map_through_graphs(gs):
    """A map growing inside one capacity bucket, replayed from captured graphs: every call equal under both settings."""
    depth, K, prev, mp, mn, cnt = scene(gs, 120, 160, seed=4)
    lib = gs._native.lib()
    n = int(cnt[0])
    lib.gs_set_graph_mode(1)
    try:
        B, _, H, W = depth.shape[:4]
        ws = {f: torch.zeros(lib.gs_slam_localize_ws_bytes(B, H, W, 4, mp.shape[1]), dtype=torch.uint8, device=depth.device)
              for f in (True, False)}
        for k in range(4):
            c = torch.tensor([n * (k + 5) // 8], dtype=torch.int32, device=depth.device)
            on = localize(gs, depth, K, prev, mp, mn, c, 4, 10, True, ws[True])
            off = localize(gs, depth, K, prev, mp, mn, c, 4, 10, False, ws[False])
            for x, y in zip(on[:5], off[:5]):
                assert torch.equal(x, y), k
            assert_fronts_equal(on[5], off[5])
    finally:
        lib.gs_set_graph_mode(-1)


def test_fused_setup_taped_gradients(gs):
    depth, K, prev, mp, mn, cnt = scene(gs, 120, 160, seed=5)
    lib = gs._native.lib()
    res = {}
    for fused in (True, False):
        lib.gs_set_fused_setup(1 if fused else 0)
        try:
            gV = torch.zeros((1, 1, 120, 160, 3), dtype=torch.float32, device=depth.device)
            lib.gs_vertex_normal_maps(depth.data_ptr(), K.data_ptr(), prev.data_ptr(), 1, 1, 120, 160, None, None, gV.data_ptr(), None,
                                      torch.cuda.current_stream().cuda_stream)
            gV.requires_grad_(True)
            mpg, mng, pv = mp.clone().requires_grad_(True), mn.clone().requires_grad_(True), prev.clone().requires_grad_(True)
            out = gs.ops.slam_localize_autograd(gV, depth, K, pv, mpg, mng, cnt, 4, 10, 1e-8, 0.1, (2.0, 1.0, 1.0, 200.0))
            (out * torch.arange(16, dtype=torch.float32, device=out.device).view(1, 1, 4, 4)).sum().backward()
            torch.cuda.synchronize()
            res[fused] = [x.detach().cpu() for x in (out, gV.grad, mpg.grad, mng.grad, pv.grad)]
        finally:
            lib.gs_set_fused_setup(1)
    for x, y in zip(res[True], res[False]):
        assert torch.equal(x, y)


def _taped_vs_untaped(gs, depth, K, prev, mp, mn, cnt, numiters, grad_params):
    B, _, H, W = depth.shape[:4]
    gV = torch.zeros((B, 1, H, W, 3), dtype=torch.float32, device=depth.device)
    gs._native.lib().gs_vertex_normal_maps(depth.data_ptr(), K.data_ptr(), prev.data_ptr(), B, 1, H, W, None, None, gV.data_ptr(), None,
                                           torch.cuda.current_stream().cuda_stream)
    with torch.no_grad():
        raw, _, _ = gs.ops.slam_localize_raw(depth, K, prev, mp, mn, cnt, 4, numiters, 1e-8, 0.1, grad_params)
        taped = gs.ops.slam_localize_autograd(gV, depth, K, prev, mp, mn, cnt, 4, numiters, 1e-8, 0.1, grad_params)
    torch.cuda.synchronize()
    assert torch.isfinite(raw).all()
    assert torch.equal(raw.cpu(), taped.cpu())


@pytest.fixture(scope="module")
def scene6(gs):
    return scene(gs, 120, 160, seed=6)


@pytest.mark.parametrize("grad_params", [None, (2.0, 1.0, 1.0, 200.0)], ids=["lm", "gradlm"])
@pytest.mark.parametrize("front", ["fused", "separate", "batch2"])
def test_taped_and_untaped_localize_return_the_same_pose(gs, scene6, front, grad_params):
    """gs_slam_localize and gs_slam_localize_taped share one front end and one loop: the same pose, bit for bit, through the fused
    front end, the 4-launch one (fused setup off) and the batched chain (B = 2: the same scene twice)."""
    args = [x.repeat(2, *([1] * (x.dim() - 1))).contiguous() for x in scene6] if front == "batch2" else list(scene6)
    lib = gs._native.lib()
    lib.gs_set_fused_setup(0 if front == "separate" else 1)
    try:
        _taped_vs_untaped(gs, *args, 10, grad_params)
    finally:
        lib.gs_set_fused_setup(1)


def test_taped_and_untaped_localize_return_the_same_pose_without_iterations(gs, scene6):
    _taped_vs_untaped(gs, *scene6, 0, None)
