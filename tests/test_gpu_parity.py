"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs, against the committed golden vectors, and through size-independent properties at
BASELINE sizes.  Tolerances: integer / index outputs bit-exact (a counted handful of fp32
decision-boundary flips is allowed where the inputs themselves differ by rounding); floating point
within 1e-4 relative (BASELINE.json north_star) unless a test says why not."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import cloud_from_golden, rel_err, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


def d(x):
    return t(x).to(DEV) if isinstance(x, np.ndarray) else x.to(DEV)


def frames_from(g, gsmod, s=None):
    rgb, depth, K, poses = d(g["colors"]), d(g["depths"]), d(g["intrinsics"]), d(g["poses"])
    r = gsmod.RGBDImages(rgb, depth, K, poses)
    return r if s is None else r[:, s]


def to_pc(gsmod, cloud):
    mv = lambda xs: None if xs is None else [x.to(DEV) for x in xs]
    return gsmod.Pointclouds(mv(cloud.points), mv(cloud.normals), mv(cloud.colors), mv(cloud.feats))


# ------------------------------------------------------------------ V
def test_maps_vs_oracle_and_fixture(gs, golden):
    from oracle import maps

    g = golden("msrd_b2s3")
    r = frames_from(g, gs)
    V, N, gV, gN = r.vertex_map.cpu(), r.normal_map.cpu(), r.global_vertex_map.cpu(), r.global_normal_map.cpu()
    # the reference's own fixture bounds (tests/structures/test_rgbdimages.py:56-165)
    assert ((V - t(g["vertex_map"])) ** 2).sum() < 1e-2
    assert ((gV - t(g["global_vertex_map"])) ** 2).sum() < 1e-2
    for mine, ref in ((N, g["normal_map"]), (gN, g["global_normal_map"])):
        assert (((mine - t(ref)) ** 2) < 1e-5).float().mean() > 0.99
    oV, oN, ogV, ogN = maps.all_maps(t(g["depths"]), t(g["intrinsics"]), t(g["poses"]))
    for name, a, b in (("V", V, oV), ("N", N, oN), ("gV", gV, ogV), ("gN", gN, ogN)):
        exact = (a == b).float().mean().item()
        print(name, "bit-exact fraction", exact, "rel err", rel_err(a, b))
        assert rel_err(a, b) < 1e-6
        # V and N follow the measured rounding of the CPU kernels bit for bit; the global maps go through
        # the host BLAS on the oracle side, whose FMA order depends on the CPU model -> tolerance only
        if name in ("V", "N"):
            assert exact > 0.97, name


def test_maps_no_poses_and_channels_first(gs, golden):
    g = golden("msrd_b2s3")
    rgb, depth, K = d(g["colors"]), d(g["depths"]), d(g["intrinsics"])
    r = gs.RGBDImages(rgb, depth, K)
    assert torch.equal(r.global_vertex_map, r.vertex_map) and torch.equal(r.global_normal_map, r.normal_map)
    rcf = gs.RGBDImages(rgb.permute(0, 1, 4, 2, 3).contiguous(), depth.permute(0, 1, 4, 2, 3).contiguous(), K,
                        d(g["poses"]), channels_first=True)
    rcl = frames_from(g, gs)
    assert torch.equal(rcf.global_vertex_map.permute(0, 1, 3, 4, 2), rcl.global_vertex_map)
    assert torch.equal(rcf.normal_map.permute(0, 1, 3, 4, 2), rcl.normal_map)


def _maps_grads(gs, depth0, K0, P0, w):
    from oracle import maps

    grads = []
    for dev in ("cpu", DEV):
        depth, K, P = (x.to(dev).clone().requires_grad_(True) for x in (depth0, K0, P0))
        outs = maps.all_maps(depth, K, P) if dev == "cpu" else gs.ops.vertex_normal_maps(depth, K, P)
        sum((o * wi.to(dev)).sum() for o, wi in zip(outs, w)).backward()
        grads.append([x.grad.cpu() for x in (depth, K, P)])
    return grads


def test_maps_backward_vs_oracle(gs, golden):
    from gradslam_amd.synthetic import make_sequence
    from oracle import maps

    torch.manual_seed(1)
    w = [torch.randn(1, 2, 64, 64, 3) for _ in range(4)]
    # (a) hole-free depth: every gradient (depth, intrinsics, poses) tight
    _, dclean, K, P = make_sequence(1, 2, 64, 64, seed=0, dropout=0.0, band=0)
    got, ref = _maps_grads(gs, dclean, K, P, w)[::-1]
    for name, a, b in zip(("depth", "K", "poses"), got, ref):
        print("clean", name, rel_err(a, b))
        assert rel_err(a, b) < 2e-4, name
    # (b) depth with holes.  Pixels whose two forward neighbours are invalid get dh == dv: the cross
    # product is a rounding residue, the "normal" is garbage and its gradient is O(1/residue) noise in the
    # reference too.  Exclude those stencils (dilated by one pixel), compare everything else tightly.
    g = golden("ref_slam_c1")
    depth = t(g["depths"])
    got, ref = _maps_grads(gs, depth, t(g["intrinsics"]), t(g["poses"]), w)[::-1]
    V = maps.vertex_map(depth, t(g["intrinsics"]))
    dh, dv = torch.zeros_like(V), torch.zeros_like(V)
    dh[..., :-1, :] = V[..., 1:, :] - V[..., :-1, :]
    dv[..., :-1, :, :] = V[..., 1:, :, :] - V[..., :-1, :, :]
    dh[..., -1, :], dv[..., -1, :, :] = dh[..., -2, :], dv[..., -2, :, :]
    cr = torch.cross(dh, dv, dim=-1).norm(dim=-1)
    degenerate = (cr < 1e-3 * dh.norm(dim=-1) * dv.norm(dim=-1)).float()
    bad = torch.nn.functional.max_pool2d(degenerate.view(-1, 1, 64, 64), 3, 1, 1).view(1, 2, 64, 64, 1) > 0
    err_d = ((got[0] - ref[0])[~bad].abs().max() / ref[0][~bad].abs().max()).item()
    print("holes: degenerate-stencil pixels excluded", bad.float().mean().item(), "depth grad rel err elsewhere", err_d)
    assert err_d < 2e-4 and bad.float().mean() < 0.25
    assert rel_err(got[2], ref[2]) < 1e-2  # pose gradient: sums the garbage pixels too


# ------------------------------------------------------------------ K
@pytest.mark.parametrize("ns,nt", [(1, 1), (63, 65), (1000, 777), (5000, 19000), (19000, 5001)])
def test_knn_bit_exact_random(gs, ns, nt):
    from oracle.knn import knn1, knn1_f64

    torch.manual_seed(ns * 7 + nt)
    src, tgt = torch.randn(ns, 3), torch.randn(nt, 3)
    tgt[nt // 2:] = tgt[: nt - nt // 2].clone()  # exact duplicates -> ties: the lowest index must win
    d2, idx = gs.ops.knn1_unpack(gs.ops.knn1_raw(src.to(DEV), tgt.to(DEV)))
    od2, oidx = knn1(src, tgt)
    assert torch.equal(idx.cpu(), oidx) and torch.equal(d2.cpu(), od2)
    # independent fp64 bound on the distances (the oracle's own contract is parity-unpinned)
    assert torch.allclose(d2.cpu().double(), knn1_f64(src, tgt), rtol=1e-5, atol=1e-10)


@pytest.mark.parametrize("kind", ["random", "sorted", "duplicates", "far"])
def test_knn_pruned_equals_bruteforce(gs, kind):
    """The AABB-pruned search must return the brute-force scan's bits on any input, including ones where
    pruning cannot help (unordered clouds) and ones full of ties."""
    torch.manual_seed(11)
    ns, nt = 7000, 9000
    src, tgt = torch.randn(ns, 3, device=DEV), torch.randn(nt, 3, device=DEV)
    if kind == "sorted":
        tgt = tgt[tgt[:, 0].argsort()].contiguous()
        src = src[src[:, 0].argsort()].contiguous()
    elif kind == "duplicates":
        tgt = (tgt * 4).round() / 4      # lattice: many exact ties
        src = (src * 4).round() / 4
    elif kind == "far":
        src = src + 50.0
    a = gs.ops.knn1_raw(src, tgt)
    b = gs.ops.knn1_raw(src, tgt, brute_force=True)
    assert torch.equal(a, b)


def test_knn_image_order_clouds(gs, golden):
    from oracle.knn import knn1

    g = golden("ref_icp_trace")
    src, tgt = t(g["fix_src"]), t(g["fix_tgt"])
    d2, idx = gs.ops.knn1_unpack(gs.ops.knn1_raw(src.to(DEV), tgt.to(DEV)))
    od2, oidx = knn1(src, tgt)
    assert torch.equal(idx.cpu(), oidx) and torch.equal(d2.cpu(), od2)


# ------------------------------------------------------------------ J
@pytest.mark.parametrize("thresh", [None, 0.01])
def test_linearize_vs_oracle(gs, golden, thresh):
    from oracle import icp

    g = golden("ref_icp_trace")
    src, tgt, nrm = t(g["syn_src"]), t(g["syn_tgt"]), t(g["syn_tgt_n"])
    A, b, idx = icp.gauss_newton_solve(src[None], tgt[None], nrm[None], thresh)
    A64, b64 = A.double(), b.double()
    best = gs.ops.knn1_raw(src.to(DEV), tgt.to(DEV))
    out = gs.ops.icp_linearize_raw(src.to(DEV), tgt.to(DEV), nrm.to(DEV), best, thresh).cpu().double()
    assert int(out[43]) == A.shape[0]
    np.testing.assert_allclose(out[:36].view(6, 6), A64.t() @ A64, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(out[36:42], (A64.t() @ b64)[:, 0], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(out[42], (b64 * b64).sum(), rtol=2e-5)
    # rows API (gauss_newton_solve) bit-exact vs the oracle's elementwise algebra
    gA, gb, gidx = gs.odometry.icputils.gauss_newton_solve(src[None].to(DEV), tgt[None].to(DEV), nrm[None].to(DEV), thresh)
    assert torch.equal(gidx.cpu(), idx) and torch.equal(gA.cpu(), A) and torch.equal(gb.cpu(), b)


def test_linearize_backward_vs_oracle(gs, golden):
    from oracle import icp

    g = golden("ref_icp_trace")
    torch.manual_seed(3)
    wH, wg = torch.randn(6, 6), torch.randn(6, 1)
    res = []
    for dev in ("cpu", DEV):
        src, tgt, nrm = (t(g[k]).to(dev).clone().requires_grad_(True) for k in ("syn_src", "syn_tgt", "syn_tgt_n"))
        if dev == "cpu":
            A, b, _ = icp.gauss_newton_solve(src[None], tgt[None], nrm[None], None)
            H, gg, e = A.t() @ A, A.t() @ b, (b * b).sum()
        else:
            best = gs.ops.knn1_raw(src.detach(), tgt.detach())
            H, gg, e = gs.ops.icp_linearize(src, tgt, nrm, best, None)
        ((H * wH.to(dev)).sum() + (gg * wg.to(dev)).sum() + 0.7 * e).backward()
        res.append([x.grad.cpu() for x in (src, tgt, nrm)])
    for name, a, b in zip(("src", "tgt", "nrm"), res[1], res[0]):
        assert rel_err(a, b) < 1e-4, (name, rel_err(a, b))


# ------------------------------------------------------------------ X: whole loops on the device
def _trace_case(golden, case):
    g = golden("ref_icp_trace")
    p = case.split("_")[0]
    return g, t(g[p + "_src"]), t(g[p + "_tgt"]), t(g[p + "_tgt_n"])


@pytest.mark.parametrize("case,kw", [("syn_icp", dict(numiters=10, dist_thresh=None)),
                                     ("syn_icp_th", dict(numiters=10, dist_thresh=0.01)),
                                     ("fix_icp", dict(numiters=30, dist_thresh=0.2))])
def test_icp_device_loop_vs_reference_trace(gs, golden, case, kw):
    g, src, tgt, nrm = _trace_case(golden, case)
    T, best, trace = gs.ops.icp_device_loop(src.to(DEV), tgt.to(DEV), nrm.to(DEV), torch.eye(4, device=DEV), kw["numiters"],
                                            1e-8, kw["dist_thresh"], want_trace=True, want_best=True)
    trace = trace.cpu().double().numpy()
    n = kw["numiters"]
    # per-iteration LM state against the reference's own trace
    # errors are compared down to 1e-8 of the first one: a converged residual (~1e-10) is rounding noise.
    # With a distance threshold that points actually cross (fix_icp: 0.2), the residual sum moves in steps under ANY
    # 1e-7-level change: tools/trace_attribution.py replays the CPU oracle on this case with the 6x6 system solved in
    # fp64, with A^T A summed in fp64, and with the source nudged by 1e-7 -- err / new_err of the late iterations move
    # by 5e-3 / 7e-3 / 3.5e-1 respectively while the final transform stays within 2.4e-7.  So:
    # first iterations tight, the rest to 1e-2 there; without crossings the sums agree to 1e-4 throughout (the same
    # three variants move them by <= 1.5e-6).  The final transform is always held to 1e-4.
    atol = 1e-8 * float(g[case + "_err"][0])
    rtol = 1e-4 if kw["dist_thresh"] is None else 1e-2
    np.testing.assert_allclose(trace[:3, 42], g[case + "_err"][:3], rtol=1e-4, atol=atol)
    np.testing.assert_allclose(trace[:n, 42], g[case + "_err"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(trace[:n, 43], g[case + "_new_err"], rtol=rtol, atol=atol)
    # the accept/reject sequence (hence damp) must match while the residual is above rounding noise; once
    # converged, new_err == err to the last bits and the decision is a coin toss in the reference too
    live = g[case + "_err"] > 1e-6 * g[case + "_err"][0]
    np.testing.assert_allclose(trace[:n, 44][live], g[case + "_damp"][live], rtol=1e-6)
    assert live.sum() >= 5
    np.testing.assert_allclose(trace[:n, 46], g[case + "_n"])
    np.testing.assert_allclose(trace[0, :36].reshape(6, 6), g[case + "_AtA"][0], rtol=1e-4, atol=1e-5)
    assert rel_err(T.cpu(), g[case + "_T"]) < 1e-4
    idx_last = gs.odometry.icputils._unpack_last(best, kw["dist_thresh"]).cpu()
    assert torch.equal(idx_last, t(g[case + "_idx_last"]))


@pytest.mark.parametrize("case,kw", [("syn_gradicp", dict(numiters=10, dist_thresh=None)),
                                     ("fix_gradicp", dict(numiters=30, dist_thresh=0.2))])
def test_gradicp_device_loop_vs_reference_trace(gs, golden, case, kw):
    g, src, tgt, nrm = _trace_case(golden, case)
    T, _, trace = gs.ops.icp_device_loop(src.to(DEV), tgt.to(DEV), nrm.to(DEV), torch.eye(4, device=DEV), kw["numiters"],
                                         1e-8, kw["dist_thresh"], grad_params=(2.0, 1.0, 1.0, 200.0), want_trace=True)
    trace = trace.cpu().double().numpy()
    n = kw["numiters"]
    assert rel_err(T.cpu(), g[case + "_T"]) < 1e-4
    # the first iterations must agree tightly; later ones only to 5e-3: with a distance threshold, points
    # cross it under 1e-7 pose differences and the residual sum moves in steps (no accept/reject here,
    # every step is applied, so the differences are carried along)
    atol = 1e-8 * float(g[case + "_err"][0])
    np.testing.assert_allclose(trace[:3, 42], g[case + "_err"][:3], rtol=1e-4, atol=atol)
    np.testing.assert_allclose(trace[:n, 42], g[case + "_err"], rtol=5e-3, atol=atol)
    np.testing.assert_allclose(trace[:n, 43], g[case + "_new_err"], rtol=5e-3, atol=atol)
    np.testing.assert_allclose(trace[:n, 44], g[case + "_damp"], rtol=5e-3)


def test_provider_recovers_known_transform(gs, golden):
    """The reference's own pin (tests/odometry/test_icp.py:14-53, test_gradicp.py:14-60)."""
    g = golden("msrd_b2s3")
    r = gs.RGBDImages(d(g["colors"][:1]), d(g["depths"][:1]), d(g["intrinsics"][:1]), d(g["poses"][:1]))
    src = gs.structures.pointclouds_from_rgbdimages(r[:, 0])
    rad = 0.1
    T = torch.tensor([[np.cos(rad), -np.sin(rad), 0.0, 0.05], [np.sin(rad), np.cos(rad), 0.0, 0.03],
                      [0.0, 0.0, 1.0, 0.01], [0.0, 0.0, 0.0, 1.0]], device=DEV, dtype=torch.float32)
    tgt = src.transform(T)
    for prov in (gs.odometry.ICPOdometryProvider(numiters=30, damp=1e-8, dist_thresh=0.2),
                 gs.odometry.GradICPOdometryProvider(numiters=30, damp=1e-8, dist_thresh=0.2)):
        out = prov.provide(tgt, src).squeeze(1).squeeze(0)
        assert out.shape == T.shape
        torch.testing.assert_close(out, T, rtol=1e-4, atol=1e-5)


def test_icp_grad_path_matches_device_loop(gs, golden):
    g, src, tgt, nrm = _trace_case(golden, "syn_icp")
    ut = gs.odometry.icputils
    s = src.to(DEV)[None]
    T0, i0 = ut.point_to_plane_ICP(s, tgt.to(DEV)[None], nrm.to(DEV)[None], torch.eye(4, device=DEV), numiters=10)
    s2 = s.clone().requires_grad_(True)
    T1, i1 = ut.point_to_plane_ICP(s2, tgt.to(DEV)[None], nrm.to(DEV)[None], torch.eye(4, device=DEV), numiters=10)
    assert rel_err(T1.detach().cpu(), T0.cpu()) < 1e-5 and torch.equal(i0, i1)
    T1.sum().backward()
    assert torch.isfinite(s2.grad).all() and s2.grad.abs().sum() > 0


ICP_GRAD_CASES = [("icp_n1", False, dict(numiters=1, damp=1e-8, dist_thresh=None)),
                  ("icp_n4", False, dict(numiters=4, damp=1e-8, dist_thresh=None)),
                  ("icp_n4_th", False, dict(numiters=4, damp=1e-8, dist_thresh=2e-4)),
                  ("icp_n3_damp", False, dict(numiters=3, damp=1e-2, dist_thresh=None)),
                  ("gradicp_n1", True, dict(numiters=1, damp=1e-8, dist_thresh=None)),
                  ("gradicp_n3", True, dict(numiters=3, damp=1e-8, dist_thresh=None)),
                  ("gradicp_n3_th", True, dict(numiters=3, damp=1e-8, dist_thresh=2e-4)),
                  ("gradicp_n3_damp", True, dict(numiters=3, damp=1e-2, dist_thresh=None, lambda_max=3.0, B=0.7, B2=1.3, nu=50.0))]


def _icp_grads(gs, g, grad_lm, kw, fused):
    ut = gs.odometry.icputils
    s, tg, n, T0 = (d(g[k]).clone().requires_grad_(True) for k in ("src", "tgt", "tgt_n", "T0"))
    old, ut.FUSED_AUTOGRAD = ut.FUSED_AUTOGRAD, fused
    try:
        fn = ut.point_to_plane_gradICP if grad_lm else ut.point_to_plane_ICP
        T, _ = fn(s[None], tg[None], n[None], T0, **kw)
        (T * d(g["W"])).sum().backward()
    finally:
        ut.FUSED_AUTOGRAD = old
    return T.detach().cpu(), [x.grad.cpu() for x in (s, tg, n, T0)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused_reverse_pass", "unrolled_autograd"])
def test_icp_input_gradients_vs_reference(gs, golden, fused):
    """Input gradients of point_to_plane_ICP / gradICP against the reference's own autograd
    (tests/golden/ref_icp_grads.npz, tools/gen_golden_icp_grads.py).  Tolerance: 1e-4 of the largest
    reference entry per tensor (north_star's bound; measured worst case 2.2e-5)."""
    g = golden("ref_icp_grads")
    worst = 0.0
    for name, grad_lm, kw in ICP_GRAD_CASES:
        T, grads = _icp_grads(gs, g, grad_lm, kw, fused)
        assert rel_err(T, t(g[name + "_T"])) < 1e-4, name
        for key, mine in zip(("g_src", "g_tgt", "g_nrm", "g_T0"), grads):
            ref = t(g[name + "_" + key])
            e = rel_err(mine, ref)
            worst = max(worst, e)
            print(name, key, "rel err %.2e" % e)
            assert torch.isfinite(mine).all() and e < 1e-4, (name, key, e)
    print("worst", worst)


def test_fused_reverse_pass_matches_unrolled_autograd_at_size(gs):
    """19 200-point clouds (160x120 ds=1), 10 iterations, both variants: the one-node reverse pass against
    the per-op autograd graph over the same kernels (same associations, same accept decisions)."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(1, 2, 120, 160, seed=3)
    r = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P[:, :1].repeat(1, 2, 1, 1).to(DEV))
    tgt_pc = gs.structures.utils.pointclouds_from_rgbdimages(r[:, 0])
    src_pc = gs.structures.utils.pointclouds_from_rgbdimages(r[:, 1])
    torch.manual_seed(0)
    g = dict(src=src_pc.points_list[0], tgt=tgt_pc.points_list[0], tgt_n=tgt_pc.normals_list[0], T0=torch.eye(4),
             W=torch.randn(4, 4))
    for grad_lm, kw in ((False, dict(numiters=10, damp=1e-8, dist_thresh=None)), (True, dict(numiters=10, damp=1e-8, dist_thresh=None)),
                        (False, dict(numiters=6, damp=1e-8, dist_thresh=1e-3)), (True, dict(numiters=6, damp=1e-8, dist_thresh=1e-3))):
        Ta, ga = _icp_grads(gs, g, grad_lm, kw, True)
        Tb, gb = _icp_grads(gs, g, grad_lm, kw, False)
        assert rel_err(Ta, Tb) < 1e-5
        for key, a, b in zip(("g_src", "g_tgt", "g_nrm", "g_T0"), ga, gb):
            print("gradLM" if grad_lm else "LM", kw["numiters"], key, "rel err %.2e" % rel_err(a, b), "|ref| %.3e" % float(b.abs().max()))
            assert rel_err(a, b) < 3e-4, (grad_lm, key)  # measured 6e-5


@pytest.mark.parametrize("odom", ["icp", "gradicp"])
def test_fused_differentiable_localisation_matches_staged(gs, odom):
    """PointFusion over 3 frames at 160x120 with gradients: the one-node localisation (taped device loop,
    search hints, device-side reverse pass) against the staged per-op autograd graph."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(1, 3, 120, 160, seed=5)
    res = []
    for fused in (True, False):
        cc, d2, kk, pp = (x.to(DEV).clone().requires_grad_(True) for x in (c, dd, K, P))
        slam = gs.slam.PointFusion(odom=odom, dsratio=2, numiters=6, device=DEV)
        slam.fused_autograd = fused
        old, gs.odometry.icputils.FUSED_AUTOGRAD = gs.odometry.icputils.FUSED_AUTOGRAD, fused
        try:
            pcs, poses = slam(gs.RGBDImages(cc, d2, kk, pp))
            (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
        finally:
            gs.odometry.icputils.FUSED_AUTOGRAD = old
        res.append((poses.detach().cpu(), pcs.points_padded.detach().cpu(), [x.grad.cpu() for x in (cc, d2, kk, pp)]))
    (pa, ma, ga), (pb, mb, gb) = res
    assert rel_err(pa, pb) < 1e-5 and ma.shape == mb.shape and rel_err(ma, mb) < 1e-5
    for name, a, b in zip(("colors", "depths", "intrinsics", "poses"), ga, gb):
        print(odom, name, "rel err %.2e" % rel_err(a, b))
        assert rel_err(a, b) < 1e-3, name


# ------------------------------------------------------------------ P / S / D
def test_active_points_and_downsample_vs_oracle(gs, golden):
    from oracle import fusion, icp

    g, gu = golden("msrd_b2s3"), golden("ref_units")
    m0 = cloud_from_golden(gu, "map0", 2)
    pc = to_pc(gs, m0)
    f1 = frames_from(g, gs, 1)
    tab = gs.slam.fusionutils.find_active_map_points(pc, f1).cpu()
    ref = t(gu["active_f1"])
    assert tab.dtype == torch.int64
    if not torch.equal(tab, ref):  # count decision-boundary flips instead of hiding them
        assert abs(tab.shape[0] - ref.shape[0]) <= 2
        common = min(tab.shape[0], ref.shape[0])
        assert (tab[:common] != ref[:common]).any(1).float().mean() < 1e-4
    # downsampling of frame and map
    fr = gs.odometry.icputils.downsample_rgbdimages(f1, 4)
    ofr = cloud_from_golden(gu, "frame_ds4", 2, feats=False)
    f0 = frames_from(g, gs, 0)
    mp = gs.odometry.icputils.downsample_pointclouds(pc, gs.slam.fusionutils.find_active_map_points(pc, f0), 4)
    omp = cloud_from_golden(gu, "mapds4", 2, feats=False)
    for b in range(2):
        assert fr.points_list[b].shape == ofr.points[b].shape
        assert rel_err(fr.points_list[b].cpu(), ofr.points[b]) < 1e-6 and rel_err(fr.normals_list[b].cpu(), ofr.normals[b]) < 1e-5
        assert torch.equal(fr.colors_list[b].cpu(), ofr.colors[b])
        assert torch.equal(mp.points_list[b].cpu(), omp.points[b]) and torch.equal(mp.normals_list[b].cpu(), omp.normals[b])


# ------------------------------------------------------------------ C / U / F / A
def test_fusion_stages_vs_reference(gs, golden):
    g, gu = golden("msrd_b2s3"), golden("ref_units")
    fu = gs.slam.fusionutils
    pc = to_pc(gs, cloud_from_golden(gu, "map0", 2))
    f1 = frames_from(g, gs, 1)
    dot_th = math.cos(math.radians(20))
    act = d(gu["active_f1"])
    sim, mask = fu.find_similar_map_points(pc, f1, act, 0.05, dot_th)
    ref_mask = t(gu["similar_mask_f1"])
    flips = (mask.cpu() != ref_mask).float().mean().item()
    print("similar-mask flips", flips)
    assert flips < 1e-4
    uni = fu.find_best_unique_correspondences(pc, f1, d(gu["similar_f1"])).cpu()
    assert torch.equal(uni, t(gu["unique_f1"]))
    # fused chain == staged chain
    chain = fu.find_correspondences(pc, f1, 0.05, dot_th).cpu()
    staged = fu.find_best_unique_correspondences(pc, f1, sim).cpu()
    assert torch.equal(chain, staged)
    alpha = fu.get_alpha(f1.vertex_map, dim=4, keepdim=True, sigma=0.6).cpu()
    assert rel_err(alpha, gu["alpha_f1"]) < 1e-6
    # merge + append with the reference's table
    out = fu.fuse_with_map(pc, f1, d(gu["unique_f1"]), 0.6)
    ref = cloud_from_golden(gu, "map1", 2)
    for b in range(2):
        assert out.points_list[b].shape == ref.points[b].shape
        for mine, theirs in ((out.points_list, ref.points), (out.normals_list, ref.normals), (out.colors_list, ref.colors),
                             (out.features_list, ref.feats)):
            assert rel_err(mine[b].cpu(), theirs[b]) < 1e-5
    # third frame through the fused update: counts and checksums
    out2 = fu.update_map_fusion(out, frames_from(g, gs, 2), 0.05, dot_th, 0.6)
    counts = out2.num_points_per_pointcloud.tolist()
    assert all(abs(c - rc) <= 3 for c, rc in zip(counts, gu["map2_counts"].tolist())), (counts, gu["map2_counts"])


def test_unique_tiebreak_handmade(gs):
    H = W = 4
    gV = torch.zeros(1, 1, H, W, 3)
    gV[0, 0, 1, 2] = torch.tensor([0.0, 0.0, 1.0])
    pts = torch.tensor([[0.0, 0.0, 1.3], [0.0, 0.0, 1.1], [0.0, 0.0, 0.9], [0.0, 0.0, 1.05], [5.0, 5.0, 5.0]])
    cc = torch.tensor([[1.0], [2.0], [2.0], [0.5], [9.0]])
    pc = gs.Pointclouds([pts.to(DEV)], [pts.to(DEV)], [pts.to(DEV)], [cc.to(DEV)])
    r = gs.RGBDImages(torch.zeros(1, 1, H, W, 3, device=DEV), torch.ones(1, 1, H, W, 1, device=DEV),
                      torch.eye(4, device=DEV).view(1, 1, 4, 4), torch.eye(4, device=DEV).view(1, 1, 4, 4))
    r._global_vertex_map = gV.to(DEV)
    r._global_normal_map = torch.zeros_like(r._global_vertex_map)
    tab = torch.tensor([[0, 0, 1, 2], [0, 1, 1, 2], [0, 2, 1, 2], [0, 3, 1, 2], [0, 4, 3, 3]], device=DEV)
    out = gs.slam.fusionutils.find_best_unique_correspondences(pc, r, tab).cpu()
    r1 = float((torch.tensor(1.1) - 1.0) ** 2)
    r2 = float((torch.tensor(0.9) - 1.0) ** 2)
    want_n = 1 if (r1, 1) < (r2, 2) else 2
    assert out.tolist() == [[0, want_n, 1, 2], [0, 4, 3, 3]]


# ------------------------------------------------------------------ config 1 end to end (+ gradients)
# Tolerances = what tools/parity_probe.py measures on an MI355X plus a margin (profiles/r02_parity_probe.txt):
#   poses 0 (gt) / 2e-8 (icp) / 1.2e-6 (gradicp) relative; map sizes exact; attributes <= 7e-7;
#   gradients of colours and poses <= 4e-7; depth gradients equal to 1e-4 of their maximum except on <= 5 pixels
#   (the dh == dv stencils of DESIGN.md "sensitivity", where the reference's normal is a rounding residue);
#   intrinsics gradients -- sums over ALL pixels, those few included -- 1.2e-2 at 64x64, 6e-4 at 160x120.
# For scale: the reference's OWN outputs move by 6.6e-5 (poses), 1e-3 (intrinsics gradient) and 5-20 % (depth
# gradient, maximum norm) when its depth input is perturbed by 1e-7 relative (tools/gen_golden_c1b.py --sensitivity).
C1_CASES = [("pf_gt", "PointFusion", "gt"), ("pf_icp", "PointFusion", "icp"), ("pf_gradicp", "PointFusion", "gradicp"),
            ("is_gradicp", "ICPSLAM", "gradicp")]


def _c1_inputs(g):
    if "colors" in g:
        c = t(g["colors"])
    else:  # ref_slam_c1b: the colours are regenerated (uniform noise does not compress) and pinned by a checksum
        from gradslam_amd.synthetic import make_sequence

        L, H, W, seed = (int(x) for x in g["shape"])
        c = make_sequence(1, L, H, W, seed=seed)[0]
        assert float(c.double().sum()) == float(g["colors_sum"][0])
    return c, t(g["depths"]), t(g["intrinsics"]), t(g["poses"])


def _check_map(pcs, g, name, tol):
    st = int(g[name + "_map_stride"][0]) if name + "_map_stride" in g else 1
    n_ref = int(g[name + "_map_count"][0]) if name + "_map_count" in g else g[name + "_map_points_0"].shape[0]
    assert pcs.points_list[0].shape[0] == n_ref, (name, pcs.points_list[0].shape[0], n_ref)
    for attr, key in (("points_list", "points"), ("normals_list", "normals"), ("colors_list", "colors")):
        e = rel_err(getattr(pcs, attr)[0].detach().cpu()[::st], g[f"{name}_map_{key}_0"])
        assert e < tol, (name, key, e)
    if name + "_map_feats_0" in g:
        e = rel_err(pcs.features_list[0].detach().cpu(), g[name + "_map_feats_0"])
        assert e < tol, (name, "feats", e)


@pytest.mark.parametrize("gname", ["ref_slam_c1", "ref_slam_c1b"])
@pytest.mark.parametrize("name,cls,odom", C1_CASES)
def test_config1_forward_vs_reference(gs, golden, gname, name, cls, odom):
    """BASELINE config 1 (2-frame 64x64) and its 3-frame 160x120 sibling against the REFERENCE's outputs: poses to 1e-5
    (north_star asks 1e-4; measured <= 1.2e-6), the map size exactly, every fused attribute to 1e-5 (measured <= 7e-7)."""
    g = golden(gname)
    if name + "_poses" not in g:
        pytest.skip("case not in this golden")
    c, dd, K, P = _c1_inputs(g)
    slam = getattr(gs.slam, cls)(odom=odom, dsratio=4, numiters=10, device=DEV)
    with torch.no_grad():
        pcs, poses = slam(gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV)))
    err = rel_err(poses.cpu(), g[name + "_poses"])
    print(gname, name, "pose rel err", err)
    assert err < 1e-5, (name, err)
    _check_map(pcs, g, name, 1e-5)


@pytest.mark.parametrize("gname", ["ref_slam_c1", "ref_slam_c1b"])
@pytest.mark.parametrize("name,cls,odom", C1_CASES)
def test_config1_gradients_vs_reference(gs, golden, gname, name, cls, odom):
    """All four input gradients of  poses.sum() + points.sum() + colors.mean()  against the reference's own autograd,
    with and without ICP in the graph (tolerances: see the comment above C1_CASES)."""
    g = golden(gname)
    if name + "_poses" not in g:
        pytest.skip("case not in this golden")
    c, dd, K, P = (x.to(DEV).clone().requires_grad_(True) for x in _c1_inputs(g))
    slam = getattr(gs.slam, cls)(odom=odom, dsratio=4, numiters=10, device=DEV)
    pcs, poses = slam(gs.RGBDImages(c, dd, K, P))
    (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
    assert rel_err(poses.detach().cpu(), g[name + "_poses"]) < 1e-5
    _check_map(pcs, g, name, 1e-5)  # the differentiable (staged mapping) path builds the same map
    grads = {k: (x.grad.cpu() if x.grad is not None else torch.zeros(x.shape)) for k, x in
             (("colors", c), ("depths", dd), ("intrinsics", K), ("poses", P))}
    for k in ("colors", "poses"):
        e = rel_err(grads[k], g[f"{name}_grad_{k}"])
        assert e < 1e-5, (name, k, e)
    ref = t(g[f"{name}_grad_depths"]).double()
    off = ((grads["depths"].double() - ref).abs() > 1e-4 * ref.abs().max()).sum().item()
    e_d = rel_err(grads["depths"], ref)
    print(gname, name, "depth gradient: elements off by > 1e-4 of the maximum:", off, "max rel err", e_d)
    assert off <= (0 if odom == "gt" else 12), (name, "depths", off)          # measured: 0 / <= 5
    assert e_d < (1e-5 if odom == "gt" else 0.1), (name, "depths", e_d)         # measured: 4e-6 / <= 2.7e-2 (those pixels)
    e_k = rel_err(grads["intrinsics"], g[f"{name}_grad_intrinsics"])
    tol_k = 1e-5 if odom == "gt" else (5e-2 if gname == "ref_slam_c1" else 5e-3)  # measured: 1e-7 / 1.2e-2 / 6e-4
    assert e_k < tol_k, (name, "intrinsics", e_k, "the reference's own value moves by ~1e-3 under a 1e-7 depth perturbation")


# ------------------------------------------------------------------ BASELINE size vs the oracle
def test_full_size_localize_vs_oracle(gs):
    """c2 at full size: one 640x480 / ds4 / 10-iteration localisation step, HIP vs CPU oracle."""
    from gradslam_amd.synthetic import make_sequence
    from oracle import fusion as ofu
    from oracle import slam as oslam
    from oracle.cloud import Cloud

    c, dd, K, P = make_sequence(1, 2, 480, 640, seed=0)
    dot_th = math.cos(math.radians(20))
    f0 = ofu.make_frame(c[:, :1], dd[:, :1], K, P[:, :1])
    cloud = ofu.update_map_fusion(Cloud(), f0, 0.05, dot_th, 0.6)
    live = ofu.make_frame(c[:, 1:2], dd[:, 1:2], K, f0["pose"])
    ref = oslam.localize(cloud, live, f0, "icp", 4, numiters=10, damp=1e-8, dist_thresh=None)
    slam = gs.slam.PointFusion(odom="icp", dsratio=4, numiters=10, device=DEV)
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    with torch.no_grad():
        pcs, _ = slam.step(gs.Pointclouds(device=DEV), frames[:, 0], None)
        got = slam._localize(pcs, gs.RGBDImages(c[:, 1:2].to(DEV), dd[:, 1:2].to(DEV), K.to(DEV)), frames[:, 0])
    e = rel_err(got.cpu(), ref)
    print("full-size localisation pose rel err vs oracle", e)
    assert e < 1e-4
    # and the fused map after frame 0 is the oracle's
    assert pcs.num_points_per_pointcloud.item() == cloud.counts[0]
    assert rel_err(pcs.points_list[0].cpu(), cloud.points[0]) < 1e-6


@pytest.mark.parametrize("odom", ["gt", "icp"])
def test_full_size_pointfusion_vs_oracle(gs, odom):
    """BASELINE configs[2] shape at reduced length: 3-frame 640x480 PointFusion, HIP vs the CPU oracle --
    recovered poses, map size and every fused attribute."""
    from gradslam_amd.synthetic import make_sequence
    from oracle import slam as oslam

    c, dd, K, P = make_sequence(1, 3, 480, 640, seed=3)
    ocloud, oposes = oslam.run(c, dd, K, P, mode="pointfusion", odom=odom, dsratio=4, numiters=10)
    slam = gs.slam.PointFusion(odom=odom, dsratio=4, numiters=10, device=DEV)
    with torch.no_grad():
        pcs, poses = slam(gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV)))
    perr = rel_err(poses.cpu(), oposes)
    n, on = int(pcs.num_points_per_pointcloud.item()), ocloud.counts[0]
    print(odom, "pose rel err", perr, "map points", n, "oracle", on)
    assert perr < 1e-4
    if odom == "gt":
        assert n == on
        # The global maps differ from the oracle's by an ulp where the host BLAS fuses differently, so a
        # projection can round to the neighbouring pixel about once per 1e6 points: count the points that
        # took a different decision instead of hiding them, and hold all the others to 1e-5.
        for name, mine, theirs in (("points", pcs.points_list, ocloud.points), ("normals", pcs.normals_list, ocloud.normals),
                                   ("colors", pcs.colors_list, ocloud.colors), ("ccounts", pcs.features_list, ocloud.feats)):
            a, b = mine[0].cpu().double(), theirs[0].double()
            bad = ((a - b).abs().amax(1) > 1e-5 * b.abs().max()).float().mean().item()
            print("   ", name, "fraction of points off by > 1e-5:", bad)
            assert bad < 1e-4, name
    else:
        # poses agree to ~1e-7, so a handful of pixels may fall on the other side of the 5 cm / 20 degree
        # fusion thresholds: the map sizes may differ by a few points out of ~3e5
        assert abs(n - on) <= max(20, on // 5000)


def test_fused_localize_equals_staged(gs, golden):
    """gs_slam_localize (one sync-free C call) must reproduce the staged Python path bit for bit, for
    icp and gradicp, on a ragged batch of 2."""
    g = golden("msrd_b2s3")
    frames = frames_from(g, gs)
    for odom in ("icp", "gradicp"):
        slam = gs.slam.PointFusion(odom=odom, dsratio=4, numiters=6, device=DEV)
        with torch.no_grad():
            pcs, _ = slam.step(gs.Pointclouds(device=DEV), frames[:, 0], None)
            mk = lambda: gs.RGBDImages(d(g["colors"][:, 1:2]), d(g["depths"][:, 1:2]), d(g["intrinsics"]))
            fused = slam._localize(pcs, mk(), frames[:, 0])
            slam._localize_fused = lambda *a: None  # force the staged path
            staged = slam._localize(pcs, mk(), frames[:, 0])
        assert torch.equal(fused, staged), odom


def test_graph_replay_equals_eager_on_a_growing_map(gs):
    """The cached hipGraph of the ICP loops bakes workspace pointers in: a sequence whose map grows every
    frame (same capacity bucket, different sizes) must give the eager result bit for bit."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(1, 8, 120, 160, seed=5)
    out = []
    for mode in (0, 1):
        gs._native.lib().gs_set_graph_mode(mode)
        slam = gs.slam.PointFusion(odom="icp", dsratio=2, numiters=5, device=DEV)
        with torch.no_grad():
            pcs, poses = slam(gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV)))
        out.append((poses.clone(), pcs.points_list[0].clone()))
    gs._native.lib().gs_set_graph_mode(-1)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert rel_err(out[1][0].cpu(), P) < 5e-2  # and it is a sane trajectory


def test_sequence_is_reproducible_and_graph_equals_eager_640x480(gs):
    """60 frames of 640x480 PointFusion, four runs in one process (eager, graph replay, graph replay, eager): poses and
    map bit for bit.  On the way the ICP target crosses the density at which the association kernel switches to smaller
    tiles (a different summation order): that switch must follow the DATA -- decided on the device from the target's
    count -- and not the host's upper bound of the map size, which depends on when asynchronous read-backs land
    (profiles/r02c_graph_vs_eager_determinism.txt: what a host-side decision did)."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(1, 60, 480, 640, seed=100)
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    out = []
    try:
        for mode in (0, 1, 1, 0):
            gs._native.lib().gs_set_graph_mode(mode)
            slam = gs.slam.PointFusion(odom="icp", dsratio=4, numiters=10, device=DEV)
            with torch.no_grad():
                pcs, poses = slam(frames)
            out.append((poses.clone(), pcs.points_list[0].clone()))
    finally:
        gs._native.lib().gs_set_graph_mode(-1)
    assert out[0][1].shape[0] > 1300000  # dense by the end: > 4 targets per ds-grid pixel in the ICP target
    for k in (1, 2, 3):
        assert torch.equal(out[0][0], out[k][0]) and torch.equal(out[0][1], out[k][1]), k


# ------------------------------------------------------------------ BASELINE sizes: properties
def test_full_size_properties(gs):
    """640x480: size-independent properties (the oracle would take minutes here)."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(1, 3, 480, 640, seed=0)
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    slam = gs.slam.PointFusion(odom="icp", dsratio=4, numiters=10, device=DEV)
    with torch.no_grad():
        pcs, poses = slam(frames)
    # (1) ICP follows the true camera motion of the synthetic scene (10 point-to-plane iterations on a
    # nearly fronto-parallel wall slide a little along it; exact parity at this size is checked against the
    # oracle in test_full_size_localize_vs_oracle)
    assert rel_err(poses.cpu(), P) < 2e-2
    # (2) map never shrinks, all confidence counts positive, normals ~unit
    n = pcs.num_points_per_pointcloud.item()
    assert n >= int((dd[0, 0] > 0).sum())
    assert (pcs.features_list[0] > 0).all()
    nn = pcs.normals_list[0].norm(dim=-1)
    assert ((nn - 1).abs() < 5e-2).float().mean() > 0.99
    # (3) unique correspondences: every (h,w) and every n at most once, sorted by (b,h,w)
    tab = gs.slam.fusionutils.find_correspondences(pcs, frames[:, 2], 0.05, math.cos(math.radians(20)))
    key = tab[:, 2] * 640 + tab[:, 3]
    assert (key[1:] > key[:-1]).all() and tab[:, 1].unique().numel() == tab.shape[0]
    # (4) nearest neighbour: idempotence (NN of the target in itself is itself, distance 0)
    pts = pcs.points_list[0][:20000].contiguous()
    d2, idx = gs.ops.knn1_unpack(gs.ops.knn1_raw(pts, pts))
    dup_ok = (pts[idx] == pts).all(1)
    assert (d2 == 0).all() and dup_ok.all() and (idx <= torch.arange(20000, device=DEV)).all()


def test_config5_shape_batch_independence_and_pose_gradients(gs):
    """BASELINE configs[4] shape: ICPSLAM (gradicp) on 1296x968 depth, batch 4, L=3.  Properties that need no
    oracle at this size: (1) sequences are independent -- the batched run equals four single-sequence runs bit
    for bit (poses, map sizes, map points); (2) poses follow the synthetic trajectory; (3) gradients through
    the recovered poses reach depth / intrinsics / first pose of EVERY sequence, are finite, and the batched
    gradients equal the single-sequence ones."""
    from gradslam_amd.synthetic import make_sequence

    B, L, H, W = 4, 3, 968, 1296
    c, dd, K, P = make_sequence(B, L, H, W, seed=11)
    run = lambda sl: gs.slam.ICPSLAM(odom="gradicp", dsratio=4, numiters=6, device=DEV)(
        gs.RGBDImages(*(x[sl].to(DEV) for x in (c, dd, K, P))))
    with torch.no_grad():
        pcs, poses = run(slice(0, B))
        singles = [run(slice(b, b + 1)) for b in range(B)]
    assert rel_err(poses.cpu(), P) < 3e-2
    for b in range(B):
        assert torch.equal(poses[b], singles[b][1][0])
        assert pcs.points_list[b].shape == singles[b][0].points_list[0].shape
        assert torch.equal(pcs.points_list[b], singles[b][0].points_list[0])
    # gradient through the poses
    def grads(sl):
        leaves = [x[sl].to(DEV).clone().requires_grad_(True) for x in (dd, K, P)]
        slam = gs.slam.ICPSLAM(odom="gradicp", dsratio=4, numiters=6, device=DEV)
        _, rp = slam(gs.RGBDImages(c[sl].to(DEV), *leaves))
        rp[:, -1, :3, 3].sum().backward()  # the last recovered camera position of every sequence
        return [x.grad.cpu() for x in leaves]
    gb = grads(slice(0, B))
    assert all(torch.isfinite(g).all() for g in gb)
    for b in range(B):
        assert gb[0][b].abs().sum() > 0 and gb[2][b, 0].abs().sum() > 0
    g1 = grads(slice(1, 2))
    for name, a, s in zip(("depth", "intrinsics", "poses"), gb, g1):
        print("c5 grads", name, "batched vs single rel err %.2e" % rel_err(a[1:2], s))
        assert rel_err(a[1:2], s) < 1e-5, name


@pytest.mark.parametrize("cls", ["PointFusion", "ICPSLAM"])
@pytest.mark.parametrize("odom,B", [("icp", 1), ("gradicp", 2), ("gt", 2)])
def test_streamed_arena_forward_equals_stepwise(gs, odom, B, cls):
    """PointFusion.forward on the arena-backed driver (two C calls per frame, device-resident counts, one host
    sync per sequence) returns bit for bit what the step-by-step path returns, including when the arena has to
    grow (8 frames at 160x120 start from a 2*H*W-row arena)."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(B, 8, 120, 160, seed=21)
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    out = {}
    # streamed sequence driver / step() with the one-call mapping step / step() with the staged mapping step
    for mode, (streamed, fused_map) in {"arena": (True, True), "step": (False, True), "staged": (False, False)}.items():
        slam = getattr(gs.slam, cls)(odom=odom, dsratio=2, numiters=6, device=DEV)
        slam.streamed, slam.fused_map = streamed, fused_map
        with torch.no_grad():
            out[mode] = slam(frames)
    pb, qb = out["staged"]
    for mode in ("arena", "step"):
        pa, qa = out[mode]
        assert torch.equal(qa, qb), mode
        assert pa.num_points_per_pointcloud.tolist() == pb.num_points_per_pointcloud.tolist(), mode
        assert pa.has_features == pb.has_features == (cls == "PointFusion")
        for attr in ("points_list", "normals_list", "colors_list") + (("features_list",) if cls == "PointFusion" else ()):
            for b in range(B):
                assert torch.equal(getattr(pa, attr)[b], getattr(pb, attr)[b]), (mode, attr, b)
        # padded views keep the zero-padding contract
        assert torch.equal(pa.points_padded, pb.points_padded), mode


@pytest.mark.parametrize("cls", ["PointFusion", "ICPSLAM"])
def test_step_out_of_place_leaves_a_separate_map(gs, cls):
    """step(..., inplace=False) on the one-call mapping step: the returned map is the staged path's, the map that
    was passed in keeps its own storage and length (and, like the reference's, now holds the merged rows)."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(1, 3, 120, 160, seed=4)
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    res = {}
    for fused_map in (True, False):
        slam = getattr(gs.slam, cls)(odom="gt", device=DEV)
        slam.fused_map = fused_map
        with torch.no_grad():
            m0, _ = slam.step(gs.Pointclouds(device=DEV), frames[:, 0], None)
            n0 = m0.num_points_per_pointcloud.tolist()
            m1, _ = slam.step(m0, frames[:, 1], None, inplace=False)
        assert m0.num_points_per_pointcloud.tolist() == n0 and m1 is not m0
        assert m1.points_padded.data_ptr() != m0.points_padded.data_ptr()
        assert int(m1.num_points_per_pointcloud[0]) > n0[0]
        res[fused_map] = (m0, m1)
    for a, b in zip(res[True], res[False]):
        for attr in ("points_list", "normals_list", "colors_list") + (("features_list",) if cls == "PointFusion" else ()):
            assert torch.equal(getattr(a, attr)[0], getattr(b, attr)[0]), attr


@pytest.mark.parametrize("grad_lm", [False, True], ids=["LM", "gradLM"])
def test_short_loops_match_the_per_op_formulation(gs, golden, grad_lm):
    """numiters = 0, 1, 2, 3: the edge cases of the folded-step launch sequence (first association without a step,
    the loop's last step as a launch of its own) against the per-op formulation of the same kernels."""
    g = golden("ref_icp_grads")
    ut = gs.odometry.icputils
    fn = ut.point_to_plane_gradICP if grad_lm else ut.point_to_plane_ICP
    s, tg, n, T0 = (d(g[k]) for k in ("src", "tgt", "tgt_n", "T0"))
    for numiters in (0, 1, 2, 3):
        Ta, ia = fn(s[None], tg[None], n[None], T0, numiters=numiters)           # device loop
        s2 = s.clone().requires_grad_(True)
        old, ut.FUSED_AUTOGRAD = ut.FUSED_AUTOGRAD, False
        try:
            Tb, ib = fn(s2[None], tg[None], n[None], T0, numiters=numiters)      # unrolled, one node per op
        finally:
            ut.FUSED_AUTOGRAD = old
        s3 = s.clone().requires_grad_(True)
        Tc, ic = fn(s3[None], tg[None], n[None], T0, numiters=numiters)          # taped loop
        assert rel_err(Ta.cpu(), Tb.detach().cpu()) < 1e-5 and torch.equal(Ta, Tc.detach()), numiters
        if numiters == 0:
            assert ia is None and ib is None and torch.equal(Ta, T0)
        else:
            assert torch.equal(ia, ib) and torch.equal(ia, ic), numiters


@pytest.mark.parametrize("kind,ns,nt", [("sorted", 6000, 200037), ("random", 6000, 200037), ("clustered", 6000, 200037),
                                        ("sorted", 1500, 1300011), ("clustered", 1500, 1300011)])
def test_knn_large_target_equals_bruteforce(gs, kind, ns, nt):
    """200 k targets (two-level boxes, several survivor rounds per tile) and 1.3 M targets (more super-boxes than one
    first-level round holds): the pruned search must stay the brute-force scan's, bit for bit, whether the boxes
    prune a lot (sorted / clustered clouds) or nothing (random)."""
    torch.manual_seed(5)
    src, tgt = torch.randn(ns, 3, device=DEV), torch.randn(nt, 3, device=DEV)
    if kind == "sorted":
        tgt = tgt[tgt[:, 0].argsort()].contiguous()
    elif kind == "clustered":
        centres = torch.randn(nt // 250 + 1, 3, device=DEV) * 3
        tgt = (centres.repeat_interleave(250, 0)[:nt] + 0.01 * torch.randn(nt, 3, device=DEV)).contiguous()
        src = (centres[torch.randint(0, centres.shape[0], (ns,), device=DEV)] + 0.02 * torch.randn(ns, 3, device=DEV)).contiguous()
        tgt[1000:1010] = tgt[2000:2010].clone()   # exact duplicates far apart in index: lowest index must win
    a = gs.ops.knn1_raw(src, tgt)
    b = gs.ops.knn1_raw(src, tgt, brute_force=True)
    assert torch.equal(a, b)


def test_degenerate_frames_streamed_and_stepwise(gs):
    """Ragged / empty inputs: one sequence of a batch of two loses a whole frame (all-zero depth), the other a
    block of rows.  Nothing may crash or go non-finite; the empty frame leaves the pose where it was and appends
    nothing; the streamed driver still equals the step-by-step path bit for bit."""
    import warnings

    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(2, 5, 120, 160, seed=31)
    dd = dd.clone()
    dd[0, 2] = 0.0            # sequence 0: frame 2 has no valid pixel at all
    dd[1, 3, :60] = 0.0       # sequence 1: frame 3 lost its upper half
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    out = {}
    for streamed in (True, False):
        slam = gs.slam.PointFusion(odom="icp", dsratio=2, numiters=5, device=DEV)
        slam.streamed = streamed
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[streamed] = slam(frames)
    (pa, qa), (pb, qb) = out[True], out[False]
    assert torch.isfinite(qa).all() and torch.equal(qa, qb)
    assert torch.equal(qa[0, 2], qa[0, 1])                     # nothing to align: the pose stays
    assert pa.num_points_per_pointcloud.tolist() == pb.num_points_per_pointcloud.tolist()
    for b in range(2):
        assert torch.equal(pa.points_list[b], pb.points_list[b]) and torch.isfinite(pa.points_list[b]).all()


def test_arena_entry_points_against_torch(gs):
    """The two arena primitives of the C ABI called directly: gs_append_rows (device-side append offset, capacity
    clamp, overflow flag) and gs_fusion_merge_inplace (== gs_fusion_merge on the rows that exist, no-op without
    correspondences)."""
    import ctypes

    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    torch.manual_seed(3)
    n, cap = 5000, 6000
    a, b = torch.randn(n, 3, device=DEV), torch.randn(n, 1, device=DEV)
    mask = (torch.rand(n, device=DEV) < 0.3).to(torch.uint8)
    dst_a, dst_b = torch.zeros(cap, 3, device=DEV), torch.zeros(cap, 1, device=DEV)
    dst_a[:4000], dst_b[:4000] = 7.0, 7.0
    count = torch.tensor([4000], dtype=torch.int32, device=DEV)
    appended, overflow = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = nv.workspace(nv.ws_bytes("gs_append_rows_ws_bytes", n), a.device, "append_test")
    src = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    dst = (ctypes.c_void_p * 2)(dst_a.data_ptr(), dst_b.data_ptr())
    widths = (ctypes.c_int * 2)(3, 1)
    nv.call("gs_append_rows", 2, src, widths, dst, nv.ptr(mask), n, nv.ptr(count), cap, nv.ptr(appended), nv.ptr(overflow),
            nv.ptr(ws), ws.numel(), nv.stream())
    sel = a[mask.bool()]
    k = sel.shape[0]
    assert int(count) == 4000 + k and int(appended) == k and int(overflow) == 0
    assert torch.equal(dst_a[4000:4000 + k], sel) and torch.equal(dst_b[4000:4000 + k], b[mask.bool()])
    assert (dst_a[:4000] == 7.0).all() and (dst_a[4000 + k:] == 0).all()
    # capacity clamp
    count.fill_(cap - 10)
    nv.call("gs_append_rows", 2, src, widths, dst, nv.ptr(mask), n, nv.ptr(count), cap, nv.ptr(appended), nv.ptr(overflow),
            nv.ptr(ws), ws.numel(), nv.stream())
    assert int(count) == cap and int(appended) == 10 and int(overflow) == 1 and torch.equal(dst_a[cap - 10:], sel[:10])

    # in-place merge against the out-of-place one
    B, H, W, N = 1, 24, 32, 900
    gV, gN, rgb = (torch.randn(B, 1, H, W, 3, device=DEV) for _ in range(3))
    alpha = torch.rand(B, 1, H, W, 1, device=DEV)
    mp, mn, mc = (torch.randn(B, N, 3, device=DEV) for _ in range(3))
    cc = torch.rand(B, N, 1, device=DEV) + 0.5
    live = 700                                    # rows beyond the count are padding
    for t in (mp, mn, mc, cc):
        t[:, live:] = 0
    counts = torch.tensor([live], dtype=torch.int32, device=DEV)
    pix = torch.randperm(H * W, device=DEV)[:300]
    rows = torch.stack([torch.zeros(300, dtype=torch.int64, device=DEV), torch.randperm(live, device=DEV)[:300], pix // W, pix % W], 1).contiguous()
    for n_rows in (300, 0):
        d_n = ops.dev_int(n_rows, DEV)
        ref = ops.fusion_merge_raw(rows, d_n, 300, gV, gN, rgb, alpha, counts, mp, mn, mc, cc)
        got = [t.clone() for t in (mp, mn, mc, cc)]
        ws = nv.workspace(nv.ws_bytes("gs_fusion_merge_inplace_ws_bytes", B, N), mp.device, "merge_test")
        nv.call("gs_fusion_merge_inplace", nv.ptr(rows), nv.ptr(d_n), 300, nv.ptr(gV), nv.ptr(gN), nv.ptr(rgb), nv.ptr(alpha), B, H, W,
                N, nv.ptr(counts), nv.ptr(got[0]), nv.ptr(got[1]), nv.ptr(got[2]), nv.ptr(got[3]), nv.ptr(ws), ws.numel(), nv.stream())
        if n_rows:
            for x, y in zip(got, ref):
                assert torch.equal(x, y)
        else:  # no correspondence: untouched (fuse_with_map skips the merge), whereas the formula would re-round every point
            for x, y in zip(got, (mp, mn, mc, cc)):
                assert torch.equal(x, y)


# rel_err of gs_fusion_merge_backward's eight outputs against float64 autograd in test_merge_row_edges.  Measured worst on an
# MI355X: 1.09e-7 (g_alpha); g_ccounts 9.1e-8, the three map adjoints 4.9e-8 .. 7.5e-8, the frame's vertex / normal / colour
# adjoints 1.2e-8 .. 3.8e-8.  The bound is under 3x the worst.
MERGE_BWD_TOL = 3e-7


def test_merge_row_edges(gs):
    """The merge of one map row (slam/fusionutils.py:678-699) and its adjoint at the rows where the formula branches,
    through the C ABI: ordinary matched rows, matched rows with c == 0 and a == 0 (c2 == 0: the where() picks the
    constant 1, so inv == 1 and d inv / d c2 == 0), matched rows with c == 0 and a > 0, unmatched live rows (one of
    them with c == 0) and zero padding.  Forward: out-of-place == in-place == the float32 restatement, bit for bit.
    Backward: float64 autograd through the same restatement; the c2 == 0 rows hold multiples of 1/8, so every sum
    there is exact in float32 and their adjoints are asserted exactly."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    B, H, W, N = 2, 4, 6, 40
    cnts = (33, 7)
    gen = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=gen)
    eighths = lambda *s: torch.round(rn(*s) * 8) / 8
    gV, gN, rgb = rn(B, 1, H, W, 3), rn(B, 1, H, W, 3), rn(B, 1, H, W, 3)
    alpha = torch.rand(B, 1, H, W, 1, generator=gen) + 0.1
    mp, mn, mc = rn(B, N, 3), rn(B, N, 3), rn(B, N, 3)
    cc = torch.rand(B, N, 1, generator=gen) + 0.5
    g_out = [rn(B, N, 3), rn(B, N, 3), rn(B, N, 3), rn(B, N, 1)]
    # (b, n, h, w) of every kind of matched row; one map point per pixel and one pixel per map point
    ordinary = [(0, 0, 0, 0), (0, 1, 3, 5), (0, 2, 1, 2), (0, 5, 2, 4), (0, 13, 0, 3), (0, 32, 3, 0), (1, 0, 1, 1), (1, 6, 3, 5)]
    zero_zero = [(0, 3, 2, 2), (1, 1, 0, 0)]  # c == 0 and a == 0
    zero_c = [(0, 4, 1, 5), (1, 3, 2, 3)]     # c == 0, a > 0
    zero_unmatched = [(0, 6)]                 # unmatched live row with c == 0: c2 == 0 without a pixel
    for b, n, h, w in zero_zero + zero_c:
        cc[b, n] = 0
    for b, n, h, w in zero_zero:
        alpha[b, 0, h, w] = 0
        for t_ in (gV, gN, rgb):
            t_[b, 0, h, w] = eighths(3)
    for b, n in [r[:2] for r in zero_zero] + zero_unmatched:
        cc[b, n] = 0
        for t_ in (mp, mn, mc) + tuple(g_out[:3]):
            t_[b, n] = eighths(3)
        g_out[3][b, n] = eighths(1)
    for b in range(B):
        for t_ in (mp, mn, mc, cc):
            t_[b, cnts[b]:] = 0
    gV, gN, rgb, alpha, mp, mn, mc, cc = (x.to(DEV) for x in (gV, gN, rgb, alpha, mp, mn, mc, cc))
    g_out = [x.to(DEV) for x in g_out]
    rows = torch.tensor(sorted(ordinary + zero_zero + zero_c), dtype=torch.int64, device=DEV)
    n_rows = rows.shape[0]
    rb, rpt, rh, rw = rows.unbind(1)
    counts = torch.tensor(cnts, dtype=torch.int32, device=DEV)
    live = (torch.arange(N, device=DEV)[None] < counts[:, None])  # (B, N)
    d_n = ops.dev_int(n_rows, DEV)
    ws = nv.workspace(nv.ws_bytes("gs_fusion_merge_ws_bytes", B, N), mp.device, "merge_test")
    frame = (nv.ptr(rows), nv.ptr(d_n), n_rows, nv.ptr(gV), nv.ptr(gN), nv.ptr(rgb), nv.ptr(alpha), B, H, W, N, nv.ptr(counts))

    def restate(gV, gN, rgb, alpha, mp, mn, mc, cc):  # fusionutils.py:660-699, op by op
        fp, fn, fc, fa = (torch.zeros_like(x) for x in (mp, mn, mc, cc))
        fp[rb, rpt], fn[rb, rpt], fc[rb, rpt], fa[rb, rpt] = gV[rb, 0, rh, rw], gN[rb, 0, rh, rw], rgb[rb, 0, rh, rw], alpha[rb, 0, rh, rw]
        c2 = cc + fa
        inv = 1 / torch.where(c2 == 0, torch.ones_like(c2), c2)
        return ((cc * mp) + (fa * fp)) * inv, ((cc * mn) + (fa * fn)) * inv, ((cc * mc) + (fa * fc)) * inv, c2

    # ---- forward
    out = [torch.full_like(x, float("nan")) for x in (mp, mn, mc, cc)]
    nv.call("gs_fusion_merge", *frame, nv.ptr(mp), nv.ptr(mn), nv.ptr(mc), nv.ptr(cc), *(nv.ptr(x) for x in out), nv.ptr(ws), ws.numel(),
            nv.stream())
    inpl = [x.clone() for x in (mp, mn, mc, cc)]
    for x in inpl:
        x[~live] = 7.0
    nv.call("gs_fusion_merge_inplace", *frame, *(nv.ptr(x) for x in inpl), nv.ptr(ws), ws.numel(), nv.stream())
    want = restate(gV, gN, rgb, alpha, mp, mn, mc, cc)
    for name, o, i, r in zip(("points", "normals", "colors", "ccounts"), out, inpl, want):
        print("merge_row_edges forward", name, "max |out - restatement|", float((o - r).abs().max()))
        assert torch.equal(o[live], i[live]), name
        assert (o[~live] == 0).all() and (i[~live] == 7.0).all(), name
        assert torch.equal(o, r), name
    for b, n in [r[:2] for r in zero_zero] + zero_unmatched:  # (0 x + 0 f) * 1
        assert all((o[b, n] == 0).all() for o in out)

    # ---- backward
    g_in = [torch.full_like(x, float("nan")) for x in (mp, mn, mc, cc)]
    g_fr = [torch.zeros_like(x) for x in (gV, gN, rgb, alpha)]
    nv.call("gs_fusion_merge_backward", *frame, nv.ptr(mp), nv.ptr(mn), nv.ptr(mc), nv.ptr(cc), *(nv.ptr(x) for x in g_out),
            *(nv.ptr(x) for x in g_in), *(nv.ptr(x) for x in g_fr), nv.ptr(ws), ws.numel(), nv.stream())
    leaves = [x.double().requires_grad_(True) for x in (gV, gN, rgb, alpha, mp, mn, mc, cc)]
    ref = torch.autograd.grad(restate(*leaves), leaves, [x.double() for x in g_out])
    ref_fr, ref_in = ref[:4], ref[4:]
    matched = torch.zeros(B, 1, H, W, dtype=torch.bool, device=DEV)
    matched[rb, 0, rh, rw] = True
    worst = 0.0
    for name, got, r in zip(("g_points", "g_normals", "g_colors", "g_ccounts"), g_in, ref_in):
        assert (got[~live] == 0).all(), name  # the kernel's padding carries no adjoint
        e = rel_err(got[live], r[live])
        print("merge_row_edges backward", name, "rel_err", e)
        worst = max(worst, e)
    for name, got, r in zip(("g_gvertex", "g_gnormal", "g_rgb", "g_alpha"), g_fr, ref_fr):
        assert (got[~matched] == 0).all(), name  # unmatched pixels keep the caller's zeros
        e = rel_err(got[matched], r[matched])
        print("merge_row_edges backward", name, "rel_err", e)
        worst = max(worst, e)
    print("merge_row_edges backward worst rel_err", worst)
    # c2 == 0: inv == 1 and dinv == 0, so x_bar = c g = 0, c_bar = c2_bar + sum x.g, and at a matched pixel
    # f_bar = a g = 0, a_bar = c2_bar + sum f.g -- exact in float32 on multiples of 1/8
    for b, n in [r[:2] for r in zero_zero] + zero_unmatched:
        for got, r in zip(g_in, ref_in):
            assert torch.equal(got[b, n].double(), r[b, n])
        assert all((got[b, n] == 0).all() for got in g_in[:3])
        s_in = sum((x[b, n] * g[b, n]).sum() for x, g in zip((mp, mn, mc), g_out))
        assert float(g_in[3][b, n]) == float(g_out[3][b, n, 0] + s_in)
    for b, n, h, w in zero_zero:
        for got, r in zip(g_fr, ref_fr):
            assert torch.equal(got[b, 0, h, w].double(), r[b, 0, h, w])
        assert all((got[b, 0, h, w] == 0).all() for got in g_fr[:3])
        s_f = sum((f[b, 0, h, w] * g[b, n]).sum() for f, g in zip((gV, gN, rgb), g_out))
        assert float(g_fr[3][b, 0, h, w]) == float(g_out[3][b, n, 0] + s_f)
    assert worst <= MERGE_BWD_TOL


@pytest.mark.parametrize("H,W,ds,B", [(50, 70, 3, 1), (33, 65, 2, 2), (17, 19, 1, 1), (121, 67, 5, 2)])
def test_odd_image_shapes_vs_oracle(gs, H, W, ds, B):
    """Image sizes that are no multiple of any tile (64x4 map tiles, 64-point ICP tiles, 256-row compaction blocks)
    and ds ratios that do not divide them: the ground-truth-odometry map must be the oracle's (same counts, same
    attributes), ICP localisation must agree with it to the path's tolerance, on all three drivers."""
    from gradslam_amd.synthetic import make_sequence
    from oracle import slam as oslam

    c, dd, K, P = make_sequence(B, 3, H, W, seed=H + W, band=2)
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    ocloud, oposes = oslam.run(c, dd, K, P, mode="pointfusion", odom="gt", dsratio=ds, numiters=5)
    for streamed, fused_map in ((True, True), (False, True), (False, False)):
        slam = gs.slam.PointFusion(odom="gt", dsratio=ds, numiters=5, device=DEV)
        slam.streamed, slam.fused_map = streamed, fused_map
        with torch.no_grad():
            pcs, poses = slam(frames)
        assert pcs.num_points_per_pointcloud.tolist() == list(ocloud.counts)
        for mine, theirs in ((pcs.points_list, ocloud.points), (pcs.normals_list, ocloud.normals),
                             (pcs.colors_list, ocloud.colors), (pcs.features_list, ocloud.feats)):
            for b in range(B):
                a, r = mine[b].cpu().double(), theirs[b].double()
                assert ((a - r).abs().amax(1) > 1e-5 * r.abs().max()).float().mean().item() < 2e-3
    # ICP on the same odd grids: a few hundred source points, fewer than one 64-point tile per wave in places
    _, oposes = oslam.run(c, dd, K, P, mode="pointfusion", odom="icp", dsratio=ds, numiters=5)
    slam = gs.slam.PointFusion(odom="icp", dsratio=ds, numiters=5, device=DEV)
    with torch.no_grad():
        pcs, poses = slam(frames)
    assert torch.isfinite(poses).all()
    assert rel_err(poses.cpu(), oposes) < 5e-3  # small clouds: the LM loop amplifies rounding


# ------------------------------------------------------------------ grid search with distance certificates
def _grid_scene(seed, Hd=60, Wd=80, ds=4, per_cell=6, motion=0.004, shuffle_hints=False, duplicates=False, with_tgt_pix=True,
                posed=False, flip_fy=False):
    """A synthetic ds-grid scene: up to `per_cell` targets per ds-grid pixel on a wavy wall (reference order
    shuffled, like a map), one source point per pixel with drop-outs, displaced by a small rigid motion.  Returns
    (src, src_pix, tgt, nrm, hints tensors) on the device."""
    g = torch.Generator().manual_seed(seed)
    fx = 525.0 * (Wd * ds) / 640.0
    fy = -fx if flip_fy else fx  # (the reference's own fixture has fy < 0)
    cx, cy = (Wd * ds - 1) / 2.0, (Hd * ds - 1) / 2.0
    wall = lambda x, y: 2.0 + 0.3 * torch.sin(2.0 * x) * torch.cos(2.0 * y)

    def backproject(u, v, jitter):
        x, y = (u - cx) / fx * 2.0, (v - cy) / fy * 2.0
        z = wall(x, y) + jitter
        return torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)

    rr, cc = torch.meshgrid(torch.arange(Hd), torch.arange(Wd), indexing="ij")
    cell = (rr * Wd + cc).reshape(-1)
    n_per = torch.randint(0, per_cell + 1, (Hd * Wd,), generator=g)
    tcell = cell.repeat_interleave(n_per)
    nt = tcell.shape[0]
    u = (tcell % Wd).float() * ds + (torch.rand(nt, generator=g) - 0.5)
    v = (tcell // Wd).float() * ds + (torch.rand(nt, generator=g) - 0.5)
    tgt = backproject(u, v, 0.002 * torch.randn(nt, generator=g))
    if duplicates:  # exact duplicates far apart in reference index and in scan order: the lowest index must win
        tgt[-50:] = tgt[:50]
        tcell[-50:] = tcell[:50]
    perm = torch.randperm(nt, generator=g)          # reference order is not image coherent
    tgt, tcell = tgt[perm].contiguous(), tcell[perm]
    nrm = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.1 * torch.randn(nt, 3, generator=g), dim=-1)
    order = torch.argsort(tcell, stable=True)
    pix_start = torch.zeros(Hd * Wd + 1, dtype=torch.int64)
    pix_start[1:] = torch.cumsum(torch.bincount(tcell, minlength=Hd * Wd), 0)
    keep = torch.rand(Hd * Wd, generator=g) > 0.08
    sc = cell[keep]
    src = backproject((sc % Wd).float() * ds, (sc // Wd).float() * ds, 0.001 * torch.randn(sc.shape[0], generator=g))
    a = 0.5 * motion
    R = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float32)
    src = (src @ R.t() + torch.tensor([motion, -0.5 * motion, 0.3 * motion])).contiguous()
    if shuffle_hints:  # inconsistent per-point hints must cost speed only
        sc = sc[torch.randperm(sc.shape[0], generator=g)]
    # the camera the targets were bucketed with (ABI 3: part of the hints; the buckets above ARE its ds-grid pixels)
    K = torch.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    pose = torch.eye(4)
    if posed:  # everything moved rigidly into a world frame: camera -> world = pose
        a, b2 = 0.4, -0.25
        Ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float32)
        Rx = torch.tensor([[1, 0, 0], [0, math.cos(b2), -math.sin(b2)], [0, math.sin(b2), math.cos(b2)]], dtype=torch.float32)
        pose[:3, :3] = Ry @ Rx
        pose[:3, 3] = torch.tensor([0.7, -0.3, 1.1])
        move = lambda x: (x @ pose[:3, :3].t() + pose[:3, 3]).contiguous()
        src, tgt, nrm = move(src), move(tgt), (nrm @ pose[:3, :3].t()).contiguous()
    dev = lambda x, dt=None: (x if dt is None else x.to(dt)).contiguous().to(DEV)
    return dict(src=dev(src), src_pix=dev(sc, torch.int32), tgt=dev(tgt), nrm=dev(nrm.contiguous()), scan_points=dev(tgt[order]),
                scan_orig=dev(order, torch.int32), pix_start=dev(pix_start, torch.int32),
                tgt_pix=dev(tcell, torch.int32) if with_tgt_pix else None, Wd=Wd, Hd=Hd, cam_pose=dev(pose), cam_K=dev(K), ds=ds)


def _taped_loop_with_hints(gs, sc, numiters, grad_lm, init_T=None):
    """gs_icp_point_to_plane_taped through the C ABI with search hints; returns (T, [(cloud, keys) per association])."""
    import ctypes

    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    class Hints(ctypes.Structure):
        _fields_ = [("scan_points", ctypes.c_void_p), ("scan_orig", ctypes.c_void_p), ("src_pix", ctypes.c_void_p),
                    ("pix_start", ctypes.c_void_p), ("tgt_pix", ctypes.c_void_p), ("grid_w", ctypes.c_int32), ("grid_h", ctypes.c_int32),
                    ("cam_pose", ctypes.c_void_p), ("cam_K", ctypes.c_void_p), ("ds", ctypes.c_int32)]

    h = Hints(sc["scan_points"].data_ptr(), sc["scan_orig"].data_ptr(), sc["src_pix"].data_ptr(), sc["pix_start"].data_ptr(),
              sc["tgt_pix"].data_ptr() if sc.get("tgt_pix") is not None else None, sc["Wd"], sc["Hd"],
              sc["cam_pose"].data_ptr(), sc["cam_K"].data_ptr(), sc["ds"])
    src, tgt, nrm = sc["src"], sc["tgt"], sc["nrm"]
    ns, nt = src.shape[0], tgt.shape[0]
    T0 = (torch.eye(4) if init_T is None else init_T).to(DEV).contiguous()
    T = torch.empty(4, 4, device=DEV)
    best = torch.empty(ns, dtype=torch.int64, device=DEV)
    # (filled with junk: the loop must not depend on what a tape or workspace held before)
    tape = torch.full((nv.ws_bytes("gs_icp_tape_bytes", ns, numiters, grad_lm),), 0xAB, dtype=torch.uint8, device=DEV)
    ws = nv.workspace(nv.ws_bytes("gs_icp_ws_bytes", ns, nt), src.device, "icp")
    lib = nv.lib()
    fn = lib.gs_icp_point_to_plane_taped
    old = list(fn.argtypes)
    fn.argtypes = old[:16] + [ctypes.POINTER(Hints)] + old[17:]
    d_ns, d_nt = ops.dev_int(ns, DEV), ops.dev_int(nt, DEV)  # held: a temporary's block would be reused by the next one
    try:
        rc = fn(src.data_ptr(), d_ns.data_ptr(), ns, tgt.data_ptr(), nrm.data_ptr(), d_nt.data_ptr(), nt,
                T0.data_ptr(), numiters, 1e-8, -1.0, grad_lm, 2.0, 1.0, 1.0, 200.0, ctypes.byref(h), T.data_ptr(), best.data_ptr(),
                tape.data_ptr(), tape.numel(), ws.data_ptr(), ws.numel(), nv.stream())
    finally:
        fn.argtypes = old
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    # tape layout (icp.hip tape_layout): records | cloud slots | neighbour slots, everything 256-byte aligned
    al = lambda x: (x + 255) // 256 * 256
    n = 2 * numiters if grad_lm else numiters + 1
    rec_b, pts_b, best_b = al((n + 1) * 160 * 4), al(ns * 12), al(ns * 8)
    out = []
    for a in range(n):
        cloud = tape[rec_b + a * pts_b: rec_b + a * pts_b + ns * 12].view(torch.float32).view(ns, 3)
        keys = tape[rec_b + n * pts_b + a * best_b: rec_b + n * pts_b + a * best_b + ns * 8].view(torch.int64)
        out.append((cloud, keys))
    return T, out


@pytest.mark.parametrize("case", ["plain", "dense", "big_motion", "big_motion_dense", "big_motion_no_tgt_pix", "shuffled_hints",
                                  "duplicates", "gradlm", "sparse", "two_rows_per_tile", "posed_camera", "negative_fy", "posed_dense_big_motion"])
def test_grid_search_every_association_is_the_bruteforce_scan(gs, case):
    """The grid search with distance certificates (knn1_loop_k<true>) must return, for EVERY association launch of a
    loop, exactly what the brute-force scan returns on that launch's cloud: same packed (distance, index) keys.  Cases:
    converging loop (certificates hold), dense pixels (>16 targets per pixel: several chunks per pixel), a 6 cm initial
    offset (certificates fail, lanes leave their window), hints that do not match the geometry, exact duplicate targets
    (lowest reference index wins), the gradLM sequence, a sparse target with empty pixels, and a grid narrower than a
    tile (every tile spans three pixel rows)."""
    kw = dict(plain={}, dense=dict(per_cell=40, Hd=30, Wd=40), big_motion=dict(motion=0.06),
              big_motion_dense=dict(motion=0.05, per_cell=24, Hd=40, Wd=60), big_motion_no_tgt_pix=dict(motion=0.06, with_tgt_pix=False),
              shuffled_hints=dict(shuffle_hints=True), duplicates=dict(duplicates=True), gradlm={}, sparse=dict(per_cell=1),
              two_rows_per_tile=dict(Hd=90, Wd=24, motion=0.03), posed_camera=dict(posed=True), negative_fy=dict(flip_fy=True, motion=0.01),
              posed_dense_big_motion=dict(posed=True, flip_fy=True, motion=0.04, per_cell=16, Hd=40, Wd=60))[case]
    sc = _grid_scene(seed=len(case), **kw)
    grad_lm = 1 if case == "gradlm" else 0
    for mode in (2, 0):  # with certificates (whatever the density) / chunk boxes only: both exact, and equal to each other
        gs._native.lib().gs_set_grid_search(mode)
        try:
            T, assoc = _taped_loop_with_hints(gs, sc, 6, grad_lm)
        finally:
            gs._native.lib().gs_set_grid_search(1)
        for a, (cloud, keys) in enumerate(assoc):
            want = gs.ops.knn1_raw(cloud.contiguous(), sc["tgt"], brute_force=True)
            bad = (keys != want).sum().item()
            assert bad == 0, (case, mode, a, bad)
        if mode == 2:
            T_grid = T.clone()
    assert torch.equal(T, T_grid)


@pytest.mark.parametrize("case,tile", [("plain", 33), ("big_motion_dense", 38), ("two_rows_per_tile", 48), ("duplicates", 47), ("gradlm", 40)])
def test_tile_points_every_association_is_the_bruteforce_scan(gs, case, tile):
    """Tiles of fewer than 64 source points per block (gs_set_tile_points; chosen automatically where every CU can host
    two of them): every association of the loop is still the brute-force scan's, with either search, and the pose
    agrees with the 64-point tiling to rounding (the tile size fixes the summation order of the 6x6 system)."""
    kw = dict(plain={}, big_motion_dense=dict(motion=0.05, per_cell=24, Hd=40, Wd=60), duplicates=dict(duplicates=True), gradlm={},
              two_rows_per_tile=dict(Hd=90, Wd=24, motion=0.03))[case]
    sc = _grid_scene(seed=len(case), **kw)
    grad_lm = 1 if case == "gradlm" else 0
    lib = gs._native.lib()
    res = {}
    for tp in (tile, 64):
        for mode in (2, 0):
            lib.gs_set_grid_search(mode)
            lib.gs_set_tile_points(tp)
            try:
                T, assoc = _taped_loop_with_hints(gs, sc, 6, grad_lm)
            finally:
                lib.gs_set_grid_search(1)
                lib.gs_set_tile_points(0)
            for a, (cloud, keys) in enumerate(assoc):
                want = gs.ops.knn1_raw(cloud.contiguous(), sc["tgt"], brute_force=True)
                bad = (keys != want).sum().item()
                assert bad == 0, (case, tp, mode, a, bad)
            res[(tp, mode)] = T.clone()
        assert torch.equal(res[(tp, 2)], res[(tp, 0)])  # same tiling: same sums, whatever the search
    assert (res[(tile, 2)] - res[(64, 2)]).abs().max().item() < 2e-5, (res[(tile, 2)] - res[(64, 2)]).abs().max().item()


def test_grid_search_sequence_equals_chunk_search(gs):
    """A 25-frame PointFusion run (map and ICP target growing, several targets per pixel) with the grid search on and
    off: poses and map bit for bit."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(1, 25, 240, 320, seed=17)
    frames = gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV))
    out = []
    for mode in (2, 0):
        gs._native.lib().gs_set_grid_search(mode)
        try:
            for odom in ("icp", "gradicp"):
                slam = gs.slam.PointFusion(odom=odom, dsratio=4, numiters=10, device=DEV)
                with torch.no_grad():
                    pcs, poses = slam(frames)
                out.append((poses.clone(), pcs.points_list[0].clone()))
        finally:
            gs._native.lib().gs_set_grid_search(1)
    for a, b in ((0, 2), (1, 3)):
        assert torch.equal(out[a][0], out[b][0]) and torch.equal(out[a][1], out[b][1])


# ------------------------------------------------------------------ BASELINE configs 3 and 4 at full image size
def test_config3_forward_backward_vs_oracle_640x480(gs):
    """BASELINE configs[2] ("c3": PointFusion, 640x480, forward + backward) at reduced length (L = 3, the CPU oracle's
    autograd takes seconds per frame): recovered poses, map size, and ALL FOUR input gradients of
    poses.sum() + points.sum() + colors.mean() against the oracle's torch-CPU autograd (the oracle itself is pinned to
    the reference's gradients at 64x64 and 160x120 by tests/test_oracle_golden.py).  reference: slam/pointfusion.py:107-112,
    slam/fusionutils.py:654-720, odometry/icputils.py:479-545 under torch autograd."""
    from gradslam_amd.synthetic import make_sequence
    from oracle import slam as oslam

    c0, d0, K0, P0 = make_sequence(1, 3, 480, 640, seed=3)
    oc, od, oK, oP = (x.clone().requires_grad_(True) for x in (c0, d0, K0, P0))
    ocloud, oposes = oslam.run(oc, od, oK, oP, mode="pointfusion", odom="gradicp", dsratio=4, numiters=10)
    (oposes.sum() + ocloud.padded("points").sum() + ocloud.padded("colors").mean()).backward()
    c, dd, K, P = (x.to(DEV).clone().requires_grad_(True) for x in (c0, d0, K0, P0))
    slam = gs.slam.PointFusion(odom="gradicp", dsratio=4, numiters=10, device=DEV)
    pcs, poses = slam(gs.RGBDImages(c, dd, K, P))
    (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
    perr = rel_err(poses.detach().cpu(), oposes.detach())
    n, on = int(pcs.num_points_per_pointcloud.item()), ocloud.counts[0]
    print("c3 fwd+bwd: pose rel err", perr, "map", n, "oracle", on)
    assert perr < 1e-4
    assert abs(n - on) <= max(20, on // 5000)   # a few pixels fall on the other side of the 5 cm / 20 degree thresholds
    same_map = n == on
    for k, x, ox in (("colors", c, oc), ("depths", dd, od), ("intrinsics", K, oK), ("poses", P, oP)):
        got, ref = x.grad.cpu().double(), ox.grad.double()
        assert torch.isfinite(got).all(), k
        off = ((got - ref).abs() > 1e-3 * ref.abs().max()).double().mean().item()
        print("   grad", k, "max rel err %.2e" % rel_err(got, ref), "fraction of elements off by > 1e-3 of the maximum: %.1e" % off)
        if k in ("colors", "depths"):
            # per-pixel gradients: equal but for the pixels whose fusion decision differs (the map sizes above) and the
            # degenerate normal stencils (DESIGN.md "sensitivity")
            assert off < (1e-4 if same_map else 1e-3), (k, off)
        else:
            assert rel_err(got, ref) < 5e-3, (k, rel_err(got, ref))


def test_config4_batch_of_eight_equals_eight_single_runs(gs):
    """BASELINE configs[3] ("c4") shape: PointFusion on B = 8 independent 640x480 sequences.  Sequences never interact
    (one per GPU in deployment): the batched run must equal eight single-sequence runs bit for bit -- poses, map sizes
    and every map attribute -- on the streamed driver and through step()."""
    from gradslam_amd.synthetic import make_sequence

    B, L = 8, 3
    c, dd, K, P = make_sequence(B, L, 480, 640, seed=40)
    run = lambda sl, streamed: _run_pf(gs, c[sl], dd[sl], K[sl], P[sl], streamed)
    for streamed in (True, False):
        pcs, poses = run(slice(0, B), streamed)
        assert rel_err(poses.cpu(), P) < 2e-2
        for b in range(B):
            spcs, sposes = run(slice(b, b + 1), streamed)
            assert torch.equal(poses[b], sposes[0]), (streamed, b)
            for attr in ("points_list", "normals_list", "colors_list", "features_list"):
                assert torch.equal(getattr(pcs, attr)[b], getattr(spcs, attr)[0]), (streamed, b, attr)


def _run_pf(gs, c, dd, K, P, streamed):
    slam = gs.slam.PointFusion(odom="icp", dsratio=4, numiters=10, device=DEV)
    slam.streamed = streamed
    with torch.no_grad():
        return slam(gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV)))


def _sharded_worker(rank, world, port, out_dir):
    """One rank of the world-size-2 rehearsal: real PointFusion on this rank's shard through run_sharded (gloo; both
    ranks share the one card of the test box)."""
    import os

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import gradslam_amd as gsm
    from gradslam_amd import parallel
    from gradslam_amd.synthetic import make_sequence

    parallel.init_from_env(backend="gloo")
    dev = torch.device("cuda", torch.cuda.current_device())
    c, dd, K, P = (x.to(dev) for x in make_sequence(3, 3, 120, 160, seed=50))

    def slam_fn(cs, ds, ks, ps):
        slam = gsm.slam.PointFusion(odom="icp", dsratio=2, numiters=5, device=dev)
        with torch.no_grad():
            return slam(gsm.RGBDImages(cs, ds, ks, ps))

    _, poses, maps = parallel.run_sharded(slam_fn, c, dd, K, P, gather_maps=True)
    torch.save({"poses": poses.cpu(), "maps": {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in maps.items()}},
               os.path.join(out_dir, "r{}.pt".format(rank)))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_run_sharded_real_slam_two_ranks(gs, tmp_path):
    """Multi-rank path with the REAL kernels: B = 3 sequences sharded 2 + 1 over two ranks, PointFusion per rank, final
    gather of poses and of the full maps (all four attributes) -- equal on every rank to the unsharded batch, in the
    reference's padded layout (structures/pointclouds.py:960-995)."""
    import socket

    import torch.multiprocessing as mp
    from gradslam_amd.synthetic import make_sequence

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_sharded_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    c, dd, K, P = make_sequence(3, 3, 120, 160, seed=50)
    slam = gs.slam.PointFusion(odom="icp", dsratio=2, numiters=5, device=DEV)
    with torch.no_grad():
        pcs, poses = slam(gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV)))
    for r in range(2):
        o = torch.load(str(tmp_path / "r{}.pt".format(r)))
        assert torch.equal(o["poses"], poses.cpu())
        assert o["maps"]["counts"] == pcs.num_points_per_pointcloud.tolist()
        for key, want in (("points", pcs.points_padded), ("normals", pcs.normals_padded), ("colors", pcs.colors_padded),
                          ("features", pcs.features_padded)):
            assert torch.equal(o["maps"][key], want.cpu()), key


def test_downsample_pointclouds_accepts_an_unsorted_table(gs, golden):
    """The reference filters rows with `pc2im_bnhw[..., 0] == b` (odometry/icputils.py:600-619): any row order is
    accepted and kept within each batch element.  A table shuffled across batch elements must give the sorted one's rows."""
    g = golden("msrd_b2s3")
    frames = frames_from(g, gs)
    fu = gs.slam.fusionutils
    pc = fu.update_map_fusion(gs.Pointclouds(device=DEV), frames[:, 0], 0.05, math.cos(math.radians(20)), 0.6)
    tab = fu.find_active_map_points(pc, frames[:, 0])
    ref = gs.odometry.icputils.downsample_pointclouds(pc, tab, 4)
    perm = torch.randperm(tab.shape[0], generator=torch.Generator().manual_seed(0)).to(DEV)
    shuffled = tab[perm]
    got = gs.odometry.icputils.downsample_pointclouds(pc, shuffled, 4)
    for b in range(2):
        # same rows per batch element, in the shuffled table's own order
        keep = shuffled[(shuffled[:, 0] == b) & (shuffled[:, 2] % 4 == 0) & (shuffled[:, 3] % 4 == 0)][:, 1]
        assert torch.equal(got.points_list[b], pc.points_list[b][keep])
        assert got.points_list[b].shape == ref.points_list[b].shape


@pytest.mark.parametrize("odom", ["gt", "icp", "gradicp"])
def test_sequence_node_gradients_equal_per_op_nodes(gs, odom):
    """PointFusion.forward with gradients as ONE autograd node per sequence (taped arena update + reverse pass over the
    frames, slam.sequence._PointFusionSeqFn) against the per-frame formulation (one node per localisation, staged differentiable
    mapping step): same poses and map bit for bit (same kernels), input gradients to 1e-5 of their maximum (the
    unmatched map points' adjoints pass through exactly here, through (c x) (1 / c) there)."""
    from gradslam_amd.synthetic import make_sequence

    c0, d0, K0, P0 = make_sequence(1, 5, 120, 160, seed=61)
    res = {}
    for fused in (True, False):
        leaves = [x.to(DEV).clone().requires_grad_(True) for x in (c0, d0, K0, P0)]
        slam = gs.slam.PointFusion(odom=odom, dsratio=2, numiters=6, device=DEV)
        slam.fused_sequence_autograd = fused
        pcs, poses = slam(gs.RGBDImages(*leaves))
        loss = (poses * torch.linspace(0.5, 1.5, poses.numel(), device=DEV).view_as(poses)).sum() + pcs.points_padded.sum() + \
            (pcs.normals_padded * 0.3).sum() + pcs.colors_padded.mean() + (pcs.features_padded ** 2).sum() * 1e-3
        loss.backward()
        res[fused] = (poses.detach().clone(), pcs.points_list[0].detach().clone(), pcs.features_list[0].detach().clone(),
                      [x.grad.clone() if x.grad is not None else torch.zeros_like(x) for x in leaves])
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
    for name, a, b in zip(("colors", "depths", "intrinsics", "poses"), res[True][3], res[False][3]):
        e = rel_err(a.cpu(), b.cpu())
        off = int(((a - b).abs() > 1e-4 * b.abs().max()).sum())
        print(odom, "sequence node vs per-op nodes, grad", name, "rel err %.2e" % e, "max |g| %.3e" % float(b.abs().max()),
              "elements off by > 1e-4 of the maximum:", off, "of", a.numel())
        assert torch.isfinite(a).all()
        if odom == "gt":
            assert e < 1e-5, (odom, name, e)
        elif name == "depths":
            # with ICP in the graph the handful of degenerate-stencil pixels (DESIGN.md "sensitivity") amplify the
            # 1-ulp differences between the two formulations (here: unmatched map points keep their adjoint exactly,
            # there it goes through (c x)(1 / c), and their coordinates have been re-rounded by later frames)
            assert off <= 12 and e < 5e-2, (odom, name, off, e)
        else:
            assert e < (1e-5 if name == "colors" else 1e-4), (odom, name, e)   # measured: 3e-7 / 2.4e-6 (intrinsics) / 1.8e-7 (poses)


def test_sequence_node_edge_cases(gs):
    """The sequence-level autograd node on the inputs the reference's forward() also accepts: no poses at all (identity
    start, slam/icpslam.py:128-134), a one-frame sequence, and zero ICP iterations -- same map, poses and gradients as the
    per-frame formulation."""
    from gradslam_amd.synthetic import make_sequence

    c0, d0, K0, P0 = make_sequence(1, 3, 60, 80, seed=71)
    for tag, (L, with_poses, numiters) in {"no_poses": (3, False, 4), "one_frame": (1, True, 4), "zero_iters": (3, True, 0)}.items():
        res = {}
        for fused in (True, False):
            c, dd, K = (x[:, :L].to(DEV).clone().requires_grad_(True) if x.dim() > 4 else x.to(DEV).clone().requires_grad_(True)
                        for x in (c0, d0, K0))
            P = P0[:, :L].to(DEV).clone().requires_grad_(True) if with_poses else None
            slam = gs.slam.PointFusion(odom="gradicp", dsratio=2, numiters=numiters, device=DEV)
            slam.fused_sequence_autograd = fused
            pcs, poses = slam(gs.RGBDImages(c, dd, K, P))
            (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
            res[fused] = (poses.detach().clone(), pcs.points_list[0].detach().clone(), dd.grad.clone(), K.grad.clone(),
                          None if P is None else P.grad.clone())
        a, b = res[True], res[False]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), tag
        off = int(((a[2] - b[2]).abs() > 1e-4 * b[2].abs().max()).sum())
        assert off <= 12, (tag, off)
        assert rel_err(a[3].cpu(), b[3].cpu()) < 1e-3, (tag, rel_err(a[3].cpu(), b[3].cpu()))
        if with_poses:
            assert rel_err(a[4].cpu(), b[4].cpu()) < 1e-4, tag


@pytest.mark.parametrize("seed", list(range(8)))
def test_grid_search_fuzz_against_bruteforce(gs, seed):
    """Randomised scenes for the grid search with distance certificates: grid shape, density, motion, loop length and
    LM / gradLM drawn per seed; every association of every loop must be the brute-force scan's, and the loop's result
    the chunk-box search's."""
    import random

    rnd = random.Random(1000 + seed)
    Hd, Wd = rnd.choice([(20, 30), (45, 64), (60, 80), (33, 129), (96, 17)])
    kw = dict(Hd=Hd, Wd=Wd, per_cell=rnd.choice([2, 5, 9, 20, 33]), motion=rnd.choice([0.001, 0.004, 0.012, 0.03, 0.08]),
              shuffle_hints=rnd.random() < 0.15, duplicates=rnd.random() < 0.3, with_tgt_pix=rnd.random() < 0.8)
    sc = _grid_scene(seed=50 + seed, **kw)
    grad_lm, iters = int(rnd.random() < 0.5), rnd.choice([1, 2, 5, 9])
    T0 = torch.eye(4)
    T0[:3, 3] = torch.tensor([rnd.uniform(-0.02, 0.02) for _ in range(3)])
    res = {}
    for mode in (2, 0):
        gs._native.lib().gs_set_grid_search(mode)
        try:
            T, assoc = _taped_loop_with_hints(gs, sc, iters, grad_lm, init_T=T0)
        finally:
            gs._native.lib().gs_set_grid_search(1)
        for a, (cloud, keys) in enumerate(assoc):
            want = gs.ops.knn1_raw(cloud.contiguous(), sc["tgt"], brute_force=True)
            assert int((keys != want).sum()) == 0, (seed, kw, mode, a)
        res[mode] = T.clone()
    assert torch.equal(res[2], res[0]), (seed, kw)


# ------------------------------------------------------------------ round 3: the REFERENCE at the sizes the dense-target kernels run at
def _loop_counts(gs, reset=False):
    import ctypes

    out = (ctypes.c_uint * 4)()
    assert gs._native.lib().gs_loop_counts(out, 1 if reset else 0) == 0
    return list(out)


_C3_CACHE = {}


def _c3_sequence(g):
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence

    L, H, W, seed = (int(x) for x in g["shape"])
    if "seq" not in _C3_CACHE:  # the ray-cast generator takes ~20 s for 64 frames: once per session
        c, dd, K, P = make_sequence(1, L, H, W, seed=seed)
        assert float(dd.double().sum()) == float(g["depths_sum"][0]) and float(c.double().sum()) == float(g["colors_sum"][0])
        assert torch.equal(K, t(g["intrinsics"])) and torch.equal(P, t(g["poses_gt"]))
        _C3_CACHE["seq"] = (c, dd, K, P)
    return _C3_CACHE["seq"]


@pytest.mark.parametrize("odom", ["icp", "gradicp"])
def test_c3_64_frames_vs_reference(gs, golden, odom):
    """BASELINE configs[2]'s shape against the REFERENCE itself (tests/golden/ref_slam_c3.npz, tools/gen_golden_c3.py:
    the unmodified reference's PointFusion on 64 synthetic 640x480 frames, dsratio 4, 10 iterations), under the default
    switches.  What can be asserted over 64 frames is bounded by the reference's OWN sensitivity, which the golden file
    carries: under a 1e-7 relative perturbation of the depth its poses move by 2e-5 at frame 1, 1e-2 from frame 17 on
    (icp; 4e-3 for gradicp) and its map size by up to 20 321 / 4 260 points -- ten LM iterations from the identity on a
    weakly constrained surface amplify a last-bit difference frame after frame.  So: every frame's pose within 10x the
    reference's own deviation so far (ONE realisation of a last-bit change: an order of magnitude, not a bound; floor:
    north_star's 1e-4), every frame's map size within 10x its own (floor 8; measured on an MI355X: poses 2.3e-2 / 4.8e-3
    against the reference's own 2.6e-2 / 3.9e-3, map sizes 21 506 / 3 722 against 20 321 / 4 274);
    the tight per-step comparison in the dense regime is test_dense_regime_step_vs_oracle.
    reference: slam/icpslam.py:99-138, slam/pointfusion.py:107-112."""
    import numpy as np

    g = golden("ref_slam_c3")
    c, dd, K, P = _c3_sequence(g)
    L = c.shape[1]
    _loop_counts(gs, reset=True)
    slam = gs.slam.PointFusion(odom=odom, dsratio=4, numiters=10, device=DEV)
    with torch.no_grad():
        pcs, poses = slam(gs.RGBDImages(c.to(DEV), dd.to(DEV), K.to(DEV), P.to(DEV)))
    loops, grid_loops, small_tile_loops, _ = _loop_counts(gs)
    name = "pf_" + odom
    ref_poses = t(g[name + "_poses"])
    per_frame = ((poses.cpu() - ref_poses).abs().amax((0, 2, 3)) / ref_poses.abs().amax((0, 2, 3))).numpy()
    counts = torch.tensor(slam.last_appended).sum(1).cumsum(0).numpy()
    dcount = np.abs(counts - g[name + "_counts"])
    pose_bound = np.maximum(1e-4, 10.0 * np.maximum.accumulate(g[name + "_sens_pose"]))
    count_bound = np.maximum(8, 10 * np.maximum.accumulate(g[name + "_sens_counts"]))
    print(name, "pose rel err per frame:", " ".join("%.1e" % x for x in per_frame[:12]), "... max %.1e at frame %d" % (per_frame.max(), per_frame.argmax()),
          "| reference's own: max %.1e" % g[name + "_sens_pose"].max())
    print("    map size differs by", dcount[:12].tolist(), "... max", int(dcount.max()), "of", int(counts[-1]), "| reference's own: max",
          int(g[name + "_sens_counts"].max()), "| loops", loops, "grid", grid_loops, "small tiles", small_tile_loops)
    assert loops == L - 1 and grid_loops == L - 1  # the grid search with its geometric proof carried every loop
    assert (per_frame <= pose_bound).all(), (name, np.nonzero(per_frame > pose_bound)[0][:5], per_frame.max())
    assert (dcount <= count_bound).all(), (name, np.nonzero(dcount > count_bound)[0][:5], dcount.max())
    # the first frames, before the amplification sets in: tight
    assert per_frame[:4].max() < 1e-4 and dcount[:3].max() <= 8, (per_frame[:4], dcount[:3])


FIXTURE_CASES = [("pf_icp", "PointFusion", "icp"), ("pf_gradicp", "PointFusion", "gradicp"),
                 ("is_icp", "ICPSLAM", "icp"), ("is_gradicp", "ICPSLAM", "gradicp")]


@pytest.mark.parametrize("name,cls,odom", FIXTURE_CASES)
def test_fixture_full_slam_vs_reference(gs, golden, name, cls, odom):
    """Full SLAM on the reference's own REAL-SENSOR fixture (tests/data/msrd_b2s3: B = 2, L = 3, 160x120, 11.8 % holes,
    fy < 0) against the reference's outputs (tests/golden/ref_slam_fixture.npz, tools/gen_golden_fixture.py): poses,
    per-sequence map sizes, map attributes (strided sample + checksums) from the no-grad path, then the four input
    gradients of  poses.sum() + points.sum() + colors.mean()  against the reference's autograd.
    reference: slam/icpslam.py:99-138, slam/pointfusion.py:107-112."""
    fx, g = golden("msrd_b2s3"), golden("ref_slam_fixture")
    inputs = [t(fx[k]) for k in ("colors", "depths", "intrinsics", "poses")]
    slam = getattr(gs.slam, cls)(odom=odom, dsratio=4, numiters=10, device=DEV)
    with torch.no_grad():
        pcs, poses = slam(gs.RGBDImages(*[x.to(DEV) for x in inputs]))
    err = rel_err(poses.cpu(), g[name + "_poses"])
    print(name, "pose rel err", err, "maps", pcs.num_points_per_pointcloud.tolist(), "reference", g[name + "_counts"].tolist())
    assert err < 1e-4, (name, err)
    st = int(g[name + "_map_stride"][0])

    def check_map(pcs):
        # a pixel is appended iff no map point passes the distance / angle thresholds for it: one of the ~19 000 decisions
        # per frame may sit on a threshold and flip with the last bit of a global vertex (the host BLAS the goldens were
        # made with contracts differently) -- measured: one extra point in one of the eight maps
        n_ref = g[name + "_counts"].tolist()
        n = pcs.num_points_per_pointcloud.tolist()
        assert all(abs(a - r) <= 2 for a, r in zip(n, n_ref)), (n, n_ref)
        attrs = [("points_list", "points"), ("normals_list", "normals"), ("colors_list", "colors")]
        if cls == "PointFusion":
            attrs.append(("features_list", "feats"))
        for b in range(2):
            for attr, key in attrs:
                a = getattr(pcs, attr)[b].detach().cpu()
                s_ref = g[f"{name}_map_{key}_{b}_sum"]
                s_err = abs(float(a.double().abs().sum()) - s_ref[1]) / s_ref[1]
                if n[b] == n_ref[b]:
                    e = rel_err(a[::st], g[f"{name}_map_{key}_{b}"])
                    assert e < 1e-4 and s_err < 1e-5, (name, b, key, e, s_err)
                else:  # rows behind the flipped pixel are shifted by one: the whole-array checksum still pins the content
                    assert s_err < 2e-3, (name, b, key, s_err)

    check_map(pcs)
    c, dd, K, P = (x.to(DEV).clone().requires_grad_(True) for x in inputs)
    pcs, poses = slam(gs.RGBDImages(c, dd, K, P))
    (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
    assert rel_err(poses.detach().cpu(), g[name + "_poses"]) < 1e-4
    check_map(pcs)
    cs = int(g["color_grad_stride"][0])
    e_c = rel_err(c.grad.cpu().reshape(-1, 3)[::cs], g[name + "_grad_colors"])
    e_p = rel_err(P.grad.cpu(), g[name + "_grad_poses"])
    ref = t(g[name + "_grad_depths"]).double()
    off = ((dd.grad.cpu().double() - ref).abs() > 1e-3 * ref.abs().max()).sum().item()
    e_k = rel_err(K.grad.cpu(), g[name + "_grad_intrinsics"])
    print(name, "gradients: colours", e_c, "poses", e_p, "intrinsics", e_k, "depth pixels off by > 1e-3 of the maximum:", off)
    assert e_c < 1e-4 and e_p < 1e-3 and e_k < 5e-3 and off <= 16, (name, e_c, e_p, e_k, off)


def test_straggler_search_overflow_falls_back_to_the_tile_search(gs):
    """the point-serial search for up to six uncertified lanes of a tile shares ONE 4096-entry list
    of (point, super-box) pairs.  One far-away lane makes the common look-ahead radius huge, every super-box then passes
    for every straggler, and on a target of more than ~700 k points six stragglers overflow the list -- the pairs that
    were dropped used to depend on the atomics' arrival order.  Now the attempt is discarded and the tile-level search
    runs.  768 k targets, six far outliers in each of 40 tiles: every association must still be the brute-force scan's,
    and the device-side counter must show that the fallback ran."""
    sc = _grid_scene(seed=5, Hd=240, Wd=320, per_cell=20, motion=0.0005)
    src = sc["src"].clone()
    for tile in range(20, 1000, 25):
        src[64 * tile + 10: 64 * tile + 16, 2] += 4.0
    sc["src"] = src.contiguous()
    lib = gs._native.lib()
    _loop_counts(gs, reset=True)
    lib.gs_set_grid_search(2)
    try:
        T, assoc = _taped_loop_with_hints(gs, sc, 4, 0)
    finally:
        lib.gs_set_grid_search(1)
    overflows = _loop_counts(gs)[3]
    print("targets", sc["tgt"].shape[0], "sources", sc["src"].shape[0], "overflowing tile searches", overflows)
    for a, (cloud, keys) in enumerate(assoc):
        want = gs.ops.knn1_raw(cloud.contiguous(), sc["tgt"], brute_force=True)
        assert (keys != want).sum().item() == 0, a
    assert sc["tgt"].shape[0] > 700000 and overflows > 0


@pytest.mark.parametrize("odom,k", [("icp", 110), ("gradicp", 140)])
def test_dense_regime_step_vs_oracle(gs, odom, k):
    """The kernels that carry a LONG sequence, pinned against the oracle at the state they run in: k frames of 640x480
    PointFusion on the HIP path (map of ~2 M points, ICP target at 6-8 points per ds-grid pixel: grid search with its
    geometric proof -- asserted from the device-side counters), then frame k+1 once on the HIP path and once
    by the CPU oracle FROM THE SAME STATE (the HIP map and pose of frame k).  Whole-sequence comparisons cannot do this:
    the reference's own poses move by 1e-2 over 64 frames under a 1e-7 depth perturbation (tests/golden/ref_slam_c3.npz,
    `*_sens_pose`), a single step does not.  Pose to north_star's 1e-4, map size to a handful of threshold flips, every
    attribute of the fused map.  reference: slam/icpslam.py:238-247, slam/fusionutils.py:761-789."""
    from gradslam_amd.synthetic import make_sequence_cached as make_sequence
    from oracle import fusion as ofu
    from oracle import knn as oknn
    from oracle import slam as oslam
    from oracle.cloud import Cloud

    c, dd, K, P = make_sequence(1, 200, 480, 640, seed=100)
    c, dd, P = c[:, :k + 1], dd[:, :k + 1], P[:, :k + 1]
    slam = gs.slam.PointFusion(odom=odom, dsratio=4, numiters=10, device=DEV)
    dev = lambda x: x.to(DEV).contiguous()
    with torch.no_grad():
        pcs, poses = slam(gs.RGBDImages(dev(c[:, :k]), dev(dd[:, :k]), dev(K), dev(P[:, :k])))
        prev = gs.RGBDImages(dev(c[:, k - 1:k]), dev(dd[:, k - 1:k]), dev(K), poses[:, k - 1:k].contiguous())
        live = gs.RGBDImages(dev(c[:, k:k + 1]), dev(dd[:, k:k + 1]), dev(K))
        state = [x[0].cpu().clone() for x in (pcs.points_list, pcs.normals_list, pcs.colors_list, pcs.features_list)]
        _loop_counts(gs, reset=True)
        pcs2, pose2 = slam.step(pcs, live, prev, inplace=False)
    loops, grid_loops, small_tile_loops, _ = _loop_counts(gs)
    n_before, n_after = state[0].shape[0], int(pcs2.num_points_per_pointcloud.item())
    # the oracle from the same state
    dot_th = math.cos(math.radians(20))
    cloud = Cloud([state[0]], [state[1]], [state[2]], [state[3]])
    pose_prev = poses[:, k - 1:k].cpu()
    f_prev = ofu.make_frame(c[:, k - 1:k], dd[:, k - 1:k], K, pose_prev)
    f_live = ofu.make_frame(c[:, k:k + 1], dd[:, k:k + 1], K, pose_prev)
    oknn.WIDE = True
    try:
        o_pose = oslam.localize(cloud, f_live, f_prev, odom, 4, numiters=10, damp=1e-8, dist_thresh=None, lambda_max=2.0, B=1.0, B2=1.0, nu=200.0)
    finally:
        oknn.WIDE = False
    o_cloud = ofu.update_map_fusion(cloud, ofu.make_frame(c[:, k:k + 1], dd[:, k:k + 1], K, o_pose), 0.05, dot_th, 0.6)
    e = rel_err(pose2.cpu(), o_pose)
    print(odom, "frame", k, "map", n_before, "->", n_after, "oracle", o_cloud.counts[0], "| pose rel err vs oracle", e,
          "| loops", loops, "grid", grid_loops, "small tiles", small_tile_loops)
    assert (loops, grid_loops, small_tile_loops) == (1, 1, 0)
    assert e < 1e-4, e
    assert abs(n_after - o_cloud.counts[0]) <= 8, (n_after, o_cloud.counts[0])
    # merged rows (the first n_before): compare all; a pose that differs in the last digits flips a few correspondences
    for mine, theirs, nm in ((pcs2.points_list, o_cloud.points, "points"), (pcs2.normals_list, o_cloud.normals, "normals"),
                             (pcs2.colors_list, o_cloud.colors, "colors"), (pcs2.features_list, o_cloud.feats, "feats")):
        a, r = mine[0][:n_before].cpu().double(), theirs[0][:n_before].double()
        bad = ((a - r).abs().amax(1) > 1e-4 * r.abs().max()).float().mean().item()
        print("   ", nm, "merged rows off by > 1e-4 of the maximum:", bad)
        assert bad < 1e-3, (nm, bad)


@pytest.mark.parametrize("odom", ["gt", "gradicp"])
def test_sequence_node_batch_equals_single_runs(gs, monkeypatch, odom):
    """The sequence-level autograd node on a BATCH: three sequences of different lengths of map in one
    call against three single-sequence calls -- poses and maps bit for bit (sequences never interact), all four input
    gradients to 1e-5 of their maximum (the scattered target adjoints are float atomics: ~1e-7)."""
    from gradslam_amd.synthetic import make_sequence

    B, L = 3, 4
    c0, d0, K0, P0 = make_sequence(B, L, 96, 128, seed=81)
    d0[1, :, :, 40:70] = 0.0  # a different hole pattern per sequence: ragged maps
    d0[2, :, 30:50] = 0.0

    def run(sl):
        leaves = [x[sl].to(DEV).clone().requires_grad_(True) for x in (c0, d0, K0, P0)]
        slam = gs.slam.PointFusion(odom=odom, dsratio=2, numiters=5, device=DEV)
        pcs, poses = slam(gs.RGBDImages(*leaves))
        loss = (poses * torch.linspace(0.5, 1.5, poses[0].numel(), device=DEV).view_as(poses[0])).sum() + pcs.points_padded.sum() + \
            (pcs.normals_padded * 0.3).sum() + pcs.colors_padded.mean() * pcs.colors_padded.numel() * 1e-6 + (pcs.features_padded ** 2).sum() * 1e-3
        loss.backward()
        return pcs, poses.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in leaves]

    singles = [run(slice(b, b + 1)) for b in range(B)]
    from gradslam_amd.slam import sequence as _sequence

    reserve, bounds = _sequence._MapArena.reserve_frame, []

    def watched_reserve(arena):
        bounds.append(reserve(arena))
        return bounds[-1]

    monkeypatch.setattr(_sequence._MapArena, "reserve_frame", watched_reserve)
    for grow in (False, True):
        # grow: the host never learns the map counts, so its bound -- and with it the batch's row stride -- outgrows the
        # first capacity in the middle of the sequence: the tapes of the early frames carry the old stride, and the
        # reverse pass has to repack its working arrays when it walks back past the growth step
        monkeypatch.setattr(_sequence, "_NO_READBACK", grow)
        del bounds[:]
        pcs, poses, grads = run(slice(0, B))
        if grow:  # (not a race against the read-backs: without them the bounds are 32768, 32768, 65536, 65536)
            assert len(bounds) == L and len(set(bounds)) == 2, bounds
        assert len(set(pcs.num_points_per_pointcloud.tolist())) == B  # really ragged
        for b in range(B):
            spcs, sposes, sgrads = singles[b]
            assert torch.equal(poses[b], sposes[0]), (grow, b)
            for attr in ("points_list", "normals_list", "colors_list", "features_list"):
                assert torch.equal(getattr(pcs, attr)[b].detach(), getattr(spcs, attr)[0].detach()), (grow, b, attr)
            for name, g, sg in zip(("colors", "depths", "intrinsics", "poses"), grads, sgrads):
                e = rel_err(g[b].cpu(), sg[0].cpu())
                assert e < 1e-5, (odom, grow, b, name, e)

@pytest.mark.gpu
def test_localize_with_a_ds_grid_of_more_than_a_million_pixels(gs):
    """gs_slam_localize stages the frame's ds-grid source cloud on the launches of the map's projection (two compactions per
    launch); a ds-grid that needs more than 1024 compaction blocks (> 2^20 pixels: its write pass needs the scan launch)
    must take the separate form instead of failing.  numiters = 0: the target is built, the pose is the previous one."""
    dev = torch.device("cuda:0")
    H, W = 1056, 1024  # 1 081 344 pixels at ds = 1 -> 1056 compaction blocks
    g = torch.Generator().manual_seed(7)
    depth = (1.0 + torch.rand((1, 1, H, W, 1), generator=g)).to(dev)
    depth[0, 0, ::7, ::5] = 0.0  # holes
    K = torch.eye(4).reshape(1, 1, 4, 4).clone()
    K[0, 0, 0, 0] = K[0, 0, 1, 1] = 500.0; K[0, 0, 0, 2] = W / 2; K[0, 0, 1, 2] = H / 2
    prev = torch.eye(4).reshape(1, 1, 4, 4).clone()
    prev[0, 0, 0, 3] = 0.1
    mp = torch.rand((1, 4096, 3), generator=g).to(dev) + torch.tensor([0.0, 0.0, 1.0], device=dev)
    mn = torch.nn.functional.normalize(torch.rand((1, 4096, 3), generator=g), dim=-1).to(dev)
    cnt = torch.tensor([4096], dtype=torch.int32, device=dev)
    poses, _, _ = gs.ops.slam_localize_raw(depth, K.to(dev), prev.to(dev), mp, mn, cnt, 1, 0, 1e-8, None, want_maps=False)
    torch.cuda.synchronize()
    assert torch.equal(poses.cpu(), prev)
