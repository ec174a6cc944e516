"""Bit-reproducible gradients under torch.use_deterministic_algorithms(True).

With torch's flag on, every backward that scatters into shared rows calls the `_det` entry of its kernel: the ICP reverse
passes (bare loop, per-frame localisation, the sequence node), the linearisation's adjoint and the maps' intrinsics adjoint.
Their gradients are then a pure function of the inputs: the same bits from run to run and under any scheduling.  With the
flag off nothing changes.  The tests run with torch's fill of uninitialised memory on (its default under the flag), so a
kernel that read memory it never wrote would show up here.  Tolerances are stated per test."""
import numpy as np
import pytest
import torch

from tests.helpers import rel_err, t

DEV = "cuda:0"

DET_SYMBOLS = ["gs_icp_backward_det_ws_bytes", "gs_icp_point_to_plane_backward_det",
               "gs_slam_localize_backward_det_ws_bytes", "gs_slam_localize_backward_det",
               "gs_icp_linearize_backward_det_ws_bytes", "gs_icp_linearize_backward_det",
               "gs_vertex_normal_maps_backward_det_ws_bytes", "gs_vertex_normal_maps_backward_det"]


# ------------------------------------------------------------------ CPU: the ABI
def test_det_entry_points_are_exported_and_bound():
    from gradslam_amd import _native

    lib = _native.lib()  # loads without a GPU; only size queries are called
    for n in DET_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _native.SIGNATURES, n
    assert lib.gs_abi_version() == 3
    sz = lambda name, *a: int(getattr(lib, name)(*a))
    assert sz("gs_icp_backward_ws_bytes", 1) <= sz("gs_icp_backward_det_ws_bytes", 1, 1, 1, 0)
    for ns, nt in ((4800, 1024), (19200, 76800)):
        base = sz("gs_icp_backward_ws_bytes", ns)
        for g in (0, 1):
            w = [sz("gs_icp_backward_det_ws_bytes", ns, nt, it, g) for it in (1, 2, 10)]
            assert base <= w[0] < w[1] < w[2], (ns, nt, g, w)
        assert sz("gs_icp_backward_det_ws_bytes", ns, nt, 10, 1) > sz("gs_icp_backward_det_ws_bytes", ns, nt, 10, 0)
        assert sz("gs_icp_linearize_backward_det_ws_bytes", ns, nt) > 0
    base = sz("gs_slam_localize_backward_ws_bytes", 2, 480, 640, 4, 100000)
    w = [sz("gs_slam_localize_backward_det_ws_bytes", 2, 480, 640, 4, 100000, it, g) for it, g in ((1, 0), (10, 0), (10, 1))]
    assert base <= w[0] < w[1] < w[2], (base, w)
    assert sz("gs_vertex_normal_maps_backward_det_ws_bytes", 2, 8, 48, 64) > sz("gs_vertex_normal_maps_backward_ws_bytes", 2, 8, 48, 64)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


class _Flag:
    """torch.use_deterministic_algorithms for a block; the state found on entry is restored on exit."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.old)


@pytest.fixture
def det_flag():
    """Restores torch's flag whatever the test did with it."""
    old = torch.are_deterministic_algorithms_enabled()
    try:
        yield _Flag
    finally:
        torch.use_deterministic_algorithms(old)


def _surface(n_side_x, n_side_y, seed):
    """Points and unit normals of the smooth random surface z = f(x, y) over [0, 1]^2 on a grid."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(4, generator=g, dtype=torch.float64) * 0.05
    x, y = torch.meshgrid(torch.linspace(0, 1, n_side_x, dtype=torch.float64), torch.linspace(0, 1, n_side_y, dtype=torch.float64),
                          indexing="ij")
    z = a[0] * torch.sin(3 * x) + a[1] * torch.cos(4 * y) + a[2] * torch.sin(2 * x + 5 * y) + a[3] * x * y
    zx = 3 * a[0] * torch.cos(3 * x) + 2 * a[2] * torch.cos(2 * x + 5 * y) + a[3] * y
    zy = -4 * a[1] * torch.sin(4 * y) + 5 * a[2] * torch.cos(2 * x + 5 * y) + a[3] * x
    p = torch.stack([x, y, z], -1).reshape(-1, 3)
    n = torch.stack([-zx, -zy, torch.ones_like(z)], -1).reshape(-1, 3)
    return p.float(), (n / n.norm(dim=-1, keepdim=True)).float()


def _contention_scene():
    """131 072 sources on the surface, 1 024 targets (a 32 x 32 grid of it): ~128 adders per target and launch."""
    src, _ = _surface(256, 512, 0)
    tgt, nrm = _surface(32, 32, 0)
    ang = 0.01
    T0 = torch.eye(4)
    T0[:3, :3] = torch.tensor([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    T0[:3, 3] = torch.tensor([0.003, -0.002, 0.004])
    W = torch.randn(4, 4, generator=torch.Generator().manual_seed(7))
    return src, tgt, nrm, T0, W


def _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm, numiters=10, damp=1e-8, grad_T=None):
    ut = gs.odometry.icputils
    s, tg, n, T = (x.to(DEV).clone().requires_grad_(True) for x in (src, tgt, nrm, T0))
    fn = ut.point_to_plane_gradICP if grad_lm else ut.point_to_plane_ICP
    out, _ = fn(s[None], tg[None], n[None], T, numiters=numiters, damp=damp, dist_thresh=None)
    if grad_T is None:
        (out * W.to(DEV)).sum().backward()
    else:
        out.backward(grad_T.to(DEV))
    torch.cuda.synchronize()
    return [x.grad.detach().clone() for x in (s, tg, n, T)]


def _assert_equal(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, k, float((x - y).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("grad_lm", [False, True], ids=["icp", "gradicp"])
def test_contention_scene_is_bitwise_reproducible(gs, det_flag, grad_lm):
    """Flag on: three independent forward + backward runs give the same bits for all four gradients.  Flag on vs off:
    rel_err <= 1e-5 per tensor (the default path adds the same contributions with float atomics)."""
    src, tgt, nrm, T0, W = _contention_scene()
    with det_flag(True):
        runs = [_icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm) for _ in range(3)]
    with det_flag(False):
        ref = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm)
    for r in runs[1:]:
        _assert_equal(runs[0], r, "det runs")
    for key, a, b in zip(("g_src", "g_tgt", "g_nrm", "g_T0"), runs[0], ref):
        e = rel_err(a.cpu(), b.cpu())
        print("gradLM" if grad_lm else "LM", key, "det vs default rel err %.2e" % e, "|g| %.3e" % float(b.abs().max()))
        assert torch.isfinite(a).all() and float(b.abs().max()) > 0 and e <= 1e-5, (key, e)


ICP_GRAD_CASES = [("icp_n1", False, dict(numiters=1, damp=1e-8, dist_thresh=None)),
                  ("icp_n4", False, dict(numiters=4, damp=1e-8, dist_thresh=None)),
                  ("icp_n4_th", False, dict(numiters=4, damp=1e-8, dist_thresh=2e-4)),
                  ("icp_n3_damp", False, dict(numiters=3, damp=1e-2, dist_thresh=None)),
                  ("gradicp_n1", True, dict(numiters=1, damp=1e-8, dist_thresh=None)),
                  ("gradicp_n3", True, dict(numiters=3, damp=1e-8, dist_thresh=None)),
                  ("gradicp_n3_th", True, dict(numiters=3, damp=1e-8, dist_thresh=2e-4)),
                  ("gradicp_n3_damp", True, dict(numiters=3, damp=1e-2, dist_thresh=None, lambda_max=3.0, B=0.7, B2=1.3, nu=50.0))]


@pytest.mark.gpu
def test_reference_goldens_under_the_flag(gs, golden, det_flag):
    """The eight reference gradient cases of tests/golden/ref_icp_grads.npz through the deterministic reverse pass:
    1e-4 of the largest reference entry per tensor (the bound of the default path's own test)."""
    g = golden("ref_icp_grads")
    ut = gs.odometry.icputils
    with det_flag(True):
        for name, grad_lm, kw in ICP_GRAD_CASES:
            s, tg, n, T0 = (t(g[k]).to(DEV).clone().requires_grad_(True) for k in ("src", "tgt", "tgt_n", "T0"))
            fn = ut.point_to_plane_gradICP if grad_lm else ut.point_to_plane_ICP
            T, _ = fn(s[None], tg[None], n[None], T0, **kw)
            (T * t(g["W"]).to(DEV)).sum().backward()
            assert rel_err(T.detach().cpu(), t(g[name + "_T"])) < 1e-4, name
            for key, x in zip(("g_src", "g_tgt", "g_nrm", "g_T0"), (s, tg, n, T0)):
                e = rel_err(x.grad.cpu(), t(g[name + "_" + key]))
                print(name, key, "rel err %.2e" % e)
                assert torch.isfinite(x.grad).all() and e < 1e-4, (name, key, e)


@pytest.mark.gpu
@pytest.mark.parametrize("grad_lm", [False, True], ids=["icp", "gradicp"])
def test_one_target_scene(gs, det_flag, grad_lm):
    """Every source's contribution lands on ONE target (one segment of Q x 131 072 entries): finite and bitwise reproducible;
    against the flag-off run see the bounds below; grad_T = 0 gives exact zeros, a NaN in grad_T gives NaN."""
    src, _ = _surface(256, 512, 1)
    src = src - torch.tensor([0.5, 0.5, 0.0])
    tgt = torch.tensor([[0.0, 0.0, 0.05]])
    nrm = torch.tensor([[0.0, 0.6, 0.8]])
    T0, W = torch.eye(4), torch.randn(4, 4, generator=torch.Generator().manual_seed(3))
    kw = dict(numiters=10, damp=1e-2)
    with det_flag(True):
        a = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm, **kw)
        b = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm, **kw)
        zero = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm, grad_T=torch.zeros(4, 4), **kw)
        gT = torch.zeros(4, 4)
        gT[0, 3] = float("nan")
        nan = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm, grad_T=gT, **kw)
    with det_flag(False):
        ref = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, grad_lm, **kw)
    _assert_equal(a, b, "det runs")
    errs = {}
    for key, x, y in zip(("g_src", "g_tgt", "g_nrm", "g_T0"), a, ref):
        errs[key] = rel_err(x.cpu(), y.cpu())
        print("gradLM" if grad_lm else "LM", key, "det vs default rel err %.2e" % errs[key], "|g| %.3e" % float(y.abs().max()))
        assert torch.isfinite(x).all(), key
    # The source and transform adjoints do not go through the scatter: 1e-5 (measured: identical).  The target's two rows
    # are sums of Q x 131 072 contributions that largely cancel; the flag-off run adds them into ONE fp32 address with
    # atomics, a running sum whose rounding error is ~sqrt(N) 2^-24 of the running magnitude, not of the result (measured
    # 4e-4 for g_tgt, 3e-2 for g_nrm against the fold, which is exact up to its one rounding): 5e-2, the flag-off run's
    # own error being the bound here.
    assert errs["g_src"] <= 1e-5 and errs["g_T0"] <= 1e-5, errs
    assert errs["g_tgt"] <= 5e-2 and errs["g_nrm"] <= 5e-2, errs
    for key, x in zip(("g_src", "g_tgt", "g_nrm", "g_T0"), zero):
        assert torch.equal(x, torch.zeros_like(x)), key
    for key, x in zip(("g_src", "g_tgt", "g_nrm", "g_T0"), nan):
        assert torch.isnan(x).any(), key
    assert torch.isnan(nan[1]).all() and torch.isnan(nan[2]).all()


def _slam_grads(gs, cls, odom, c, dd, K, P, **kw):
    cc, d2, kk, pp = (x.to(DEV).clone().requires_grad_(True) for x in (c, dd, K, P))
    slam = getattr(gs.slam, cls)(odom=odom, device=DEV, **kw)
    pcs, poses = slam(gs.RGBDImages(cc, d2, kk, pp))
    (poses.sum() + pcs.points_padded.sum() + pcs.colors_padded.mean()).backward()
    torch.cuda.synchronize()
    return [x.grad.detach().clone() if x.grad is not None else torch.zeros_like(x) for x in (cc, d2, kk, pp)]


@pytest.mark.gpu
@pytest.mark.parametrize("cls,B,L,H,W", [("PointFusion", 1, 3, 480, 640), ("ICPSLAM", 2, 3, 120, 160)], ids=["pointfusion_seq", "icpslam_b2"])
def test_slam_nodes_are_bitwise_reproducible(gs, det_flag, cls, B, L, H, W):
    """gradICP SLAM through the nodes users reach (PointFusion: the sequence node; ICPSLAM B = 2: the per-frame
    localisation nodes and the maps' adjoint): two runs under the flag give the same bits for the gradients of rgb, depth,
    K and poses, and stay within 1e-3 of the flag-off run (the bound of the fused-vs-staged localisation test)."""
    from gradslam_amd.synthetic import make_sequence

    c, dd, K, P = make_sequence(B, L, H, W, seed=5)
    kw = dict(dsratio=4, numiters=10)
    with det_flag(True):
        a = _slam_grads(gs, cls, "gradicp", c, dd, K, P, **kw)
        b = _slam_grads(gs, cls, "gradicp", c, dd, K, P, **kw)
    with det_flag(False):
        ref = _slam_grads(gs, cls, "gradicp", c, dd, K, P, **kw)
    _assert_equal(a, b, cls)
    for name, x, y in zip(("colors", "depths", "intrinsics", "poses"), a, ref):
        e = rel_err(x.cpu(), y.cpu())
        print(cls, name, "det vs default rel err %.2e" % e)
        assert torch.isfinite(x).all() and e < 1e-3, (name, e)


def _maps_grads(gs, depth, K, poses, Ws):
    dd, kk, pp = (x.to(DEV).clone().requires_grad_(True) for x in (depth, K, poses))
    outs = gs.ops.vertex_normal_maps(dd, kk, pp)
    sum(((o * w.to(DEV)).sum() for o, w in zip(outs, Ws))).backward()
    torch.cuda.synchronize()
    return [x.grad.detach().clone() for x in (dd, kk, pp)]


@pytest.mark.gpu
def test_maps_node_is_bitwise_reproducible(gs, det_flag):
    """_MapsFn with L = 8 frames sharing each K (the default path adds their K terms with float atomics): two runs under
    the flag give the same bits; within 2e-4 of the flag-off run (the maps adjoint test's bound)."""
    from gradslam_amd.synthetic import make_sequence

    _, dd, K, P = make_sequence(2, 8, 48, 64, seed=2)
    g = torch.Generator().manual_seed(4)
    Ws = [torch.randn(2, 8, 48, 64, 3, generator=g) for _ in range(4)]
    with det_flag(True):
        a = _maps_grads(gs, dd, K, P, Ws)
        b = _maps_grads(gs, dd, K, P, Ws)
    with det_flag(False):
        ref = _maps_grads(gs, dd, K, P, Ws)
    _assert_equal(a, b, "maps")
    for name, x, y in zip(("depth", "K", "poses"), a, ref):
        e = rel_err(x.cpu(), y.cpu())
        print("maps", name, "det vs default rel err %.2e" % e)
        assert e < 2e-4, (name, e)


def _linearize_grads(gs, src, tgt, nrm, Ws):
    s, tg, n = (x.to(DEV).clone().requires_grad_(True) for x in (src, tgt, nrm))
    best = gs.ops.knn1_raw(s.detach(), tg.detach())
    H, gv, e = gs.ops.icp_linearize(s, tg, n, best, None)
    ((H * Ws[0].to(DEV)).sum() + (gv * Ws[1].to(DEV)).sum() + e * 0.5).backward()
    torch.cuda.synchronize()
    return [x.grad.detach().clone() for x in (s, tg, n)]


@pytest.mark.gpu
def test_linearize_node_is_bitwise_reproducible(gs, det_flag):
    """ops.icp_linearize with 65 536 sources associated to 64 targets (~1 000 per target): bitwise reproducible under the
    flag, within 1e-4 of the flag-off run (the linearise adjoint test's bound)."""
    src, _ = _surface(256, 256, 2)
    tgt, nrm = _surface(8, 8, 2)
    g = torch.Generator().manual_seed(5)
    Ws = [torch.randn(6, 6, generator=g), torch.randn(6, 1, generator=g)]
    with det_flag(True):
        a = _linearize_grads(gs, src, tgt, nrm, Ws)
        b = _linearize_grads(gs, src, tgt, nrm, Ws)
    with det_flag(False):
        ref = _linearize_grads(gs, src, tgt, nrm, Ws)
    _assert_equal(a, b, "linearize")
    errs = {name: rel_err(x.cpu(), y.cpu()) for name, x, y in zip(("src", "tgt", "nrm"), a, ref)}
    print("linearize det vs default rel err", errs)
    assert all(float(y.abs().max()) > 0 for y in ref) and all(e < 1e-4 for e in errs.values()), errs


@pytest.mark.gpu
def test_linearize_fold_with_non_finite_upstream_entries(gs, det_flag):
    """gs_icp_linearize_backward_det with 130 sources on 40 targets, +inf in the upstream gH[0][1] and NaN in gH[1][1].  With
    a = [n ; s x n] the row adjoint is a_bar_u = sum_w (gH[u][w] + gH[w][u]) a_w + ..., and a_bar_0, a_bar_1 are added to the
    x and y of the target normal's adjoint: every source of target j contributes (inf) n_j.y to x and a NaN to y.  So x of an
    associated target is the infinity of the sign of n_j.y, y is NaN, and every other element (z, the target adjoint, the rows
    of targets without a source) holds the bits of the same call with the two entries set to zero."""
    ns, nt = 130, 40
    g = torch.Generator().manual_seed(9)
    src = torch.rand(ns, 3, generator=g)
    tgt = torch.rand(nt, 3, generator=g)
    nrm = torch.randn(nt, 3, generator=g)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    gH, gg, ge = torch.randn(6, 6, generator=g), torch.randn(6, 1, generator=g), torch.tensor(0.5)
    bad, zero = gH.clone(), gH.clone()
    bad[0, 1], bad[1, 1], zero[0, 1], zero[1, 1] = float("inf"), float("nan"), 0.0, 0.0

    def run(up):
        s, tg, n = (x.to(DEV).clone().requires_grad_(True) for x in (src, tgt, nrm))
        best = gs.ops.knn1_raw(s.detach(), tg.detach())
        torch.autograd.backward(list(gs.ops.icp_linearize(s, tg, n, best, None)), [up.to(DEV), gg.to(DEV), ge.to(DEV)])
        return [x.grad.cpu().numpy() for x in (s, tg, n)], (best & 0xFFFFFFFF).cpu().numpy()

    with det_flag(True):
        (got_s, got_t, got_n), j = run(bad)
        (ref_s, ref_t, ref_n), _ = run(zero)
    assoc = np.zeros(nt, bool)
    assoc[j] = True
    assert 20 < assoc.sum() < nt and (np.bincount(j) > 1).any()  # shared targets, and targets without a source
    hit = np.zeros((nt, 3), bool)
    hit[assoc, :2] = True
    n_y = nrm.numpy()[:, 1]
    assert (n_y != 0).all()
    want_x = np.where(n_y > 0, np.float32(np.inf), np.float32(-np.inf))
    assert np.array_equal(got_n[assoc, 0], want_x[assoc]) and np.isnan(got_n[assoc, 1]).all()
    assert np.isposinf(got_n[hit]).any() and np.isneginf(got_n[hit]).any() and np.isnan(got_n[hit]).any()
    bits = lambda x: x.view(np.uint32)
    assert np.array_equal(bits(got_n)[~hit], bits(ref_n)[~hit]) and np.array_equal(bits(got_t), bits(ref_t))
    assert np.array_equal(bits(got_s), bits(ref_s))  # (gH's upper-left block reaches the normals only)
    assert (ref_n[assoc] != 0).all() and (ref_t[assoc] != 0).all() and not ref_n[~assoc].any()


@pytest.mark.gpu
def test_scheduling_independence(gs, det_flag):
    """The contention backward while a side stream keeps the GPU busy with matmuls: the same bits as the quiet run."""
    src, tgt, nrm, T0, W = _contention_scene()
    with det_flag(True):
        quiet = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, True)
    x = torch.randn(4096, 4096, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with det_flag(False):  # (the side work is plain load; the flag is read by the backward below)
        with torch.cuda.stream(side):
            y = x
            for _ in range(40):
                y = torch.tanh(y @ x) * 0.01
    with det_flag(True):
        busy = _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, True)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    _assert_equal(quiet, busy, "busy vs quiet")


@pytest.mark.gpu
def test_dispatch_follows_the_flag(gs, det_flag, monkeypatch):
    """Flag off: the backward nodes call only the existing entries; flag on: only the `_det` ones."""
    from gradslam_amd import ops

    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    default = {"gs_icp_point_to_plane_backward", "gs_icp_linearize_backward", "gs_vertex_normal_maps_backward"}
    src, tgt, nrm, T0, W = _contention_scene()
    src, tgt, nrm = src[:4096], tgt[:256], nrm[:256]
    from gradslam_amd.synthetic import make_sequence

    _, dd, K, P = make_sequence(1, 2, 24, 32, seed=1)
    Wm = [torch.ones(1, 2, 24, 32, 3)] * 4
    for on in (False, True):
        with det_flag(on):
            for run in (lambda: _icp_fwd_bwd(gs, src, tgt, nrm, T0, W, True, numiters=2),
                        lambda: _linearize_grads(gs, src, tgt, nrm, [torch.ones(6, 6), torch.ones(6, 1)]),
                        lambda: _maps_grads(gs, dd, K, P, Wm)):
                names.clear()
                run()
                bwd = {n for n in names if "backward" in n}
                assert bwd, names
                if on:
                    assert all(n.endswith("_det") for n in bwd), bwd
                else:
                    assert bwd <= default, bwd
