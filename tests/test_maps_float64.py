"""The vertex / normal maps kernel and its adjoint (csrc/gs_maps.hpp, csrc/maps.hip) against a float64 reference at tile
seams, with two small per-op seams of the same age (get_alpha, transform_points).

Reference: oracle.maps.all_maps on .double() casts of the same fp32 inputs; gradients from float64 autograd of
sum_i (out_i * w_i).sum().  Inputs: make_sequence, then intrinsics that differ per batch element (b = 1: fx and fy scaled,
fy negative, cx and cy shifted).  Shapes: CASES below, one line of reasons each.

Degenerate pixels.  fp32 and float64 must disagree at exactly one kind of pixel: a valid one (d > 0) whose horizontal
stencil neighbour (right; left in the last column) and vertical stencil neighbour (below; above in the last row) are both
invalid (d <= 0).  There dh == +-dv bit for bit, the fp32 cross product is an FMA residue normalised to a unit vector, and
float64 gives 0 (or a residue of its own).  Those pixels are left out of the N / gN comparisons and the upstream weights of N / gN are zero there,
so no residue reaches any gradient.  Nothing else is excluded anywhere.

Tolerances.  None is taken from the kernel.  Per case and compared quantity the yardstick is the error (max abs) of the
float32 CPU oracle against the float64 reference on the same inputs and weights, computed here.  The kernel may be off by
4 x that yardstick (it contracts FMAs where the CPU kernels may not, and the oracle's global maps go through the host
BLAS), or by 8 * 2^-24 * (largest reference magnitude of the quantity) where that floor is larger (the yardstick can come
out near one ulp by luck).

Recorded figures: max abs error against float64, "yard" = the float32 CPU oracle, "MI355X" = the kernel.  (An earlier
CPU survey of the same inputs: V, gV 4e-7; N, gN 1.6e-5; depth gradient 2.2e-5, K gradient 4.3e-5, pose gradient 1e-6 relative.)

    maps, worst of the five cases (70x257)          gradients, all four upstream gradients present
    quantity  largest |ref|  yard     MI355X        case    quantity  largest |ref|  yard     MI355X
    V         2.3            2.7e-7   2.7e-7        2x2     g_depth   5.5            1.6e-6   1.2e-6
    N         1.0            1.2e-5   1.2e-5                g_K       5.6            4.7e-7   7.1e-7
    gV        2.3            3.6e-7   3.6e-7                g_poses   10.5           5.4e-7   1.2e-6
    gN        1.0            1.2e-5   1.2e-5        5x65    g_depth   181            7.8e-4   7.8e-4
                                                            g_K       9.5            4.6e-6   1.1e-5
    plane (5 x 65), N against the closed form:              g_poses   43             3.1e-5   2.3e-5
              1.0            5.5e-6   5.5e-6        9x200   g_depth   596            8.0e-3   8.0e-3
                                                            g_K       12.6           1.5e-5   4.7e-5
    get_alpha, n = 2^20 + 300:                              g_poses   226            9.2e-5   5.9e-5
    alpha     1.0            8.3e-8   8.2e-8        37x131  g_depth   575            6.2e-3   6.2e-3
    g_points  4.3            4.8e-7   4.8e-7                g_K       5.6            3.1e-5   3.2e-5
                                                            g_poses   262            2.4e-4   9.3e-5
                                                    70x257  g_depth   1166           2.0e-2   2.0e-2
                                                            g_K       4.2            3.0e-5   2.6e-5
                                                            g_poses   848            1.7e-3   4.1e-4

The maps and the depth gradient follow the CPU oracle's rounding almost bit for bit; the K and pose gradients are sums over
the image in another order, so their errors differ from the yardstick's by the luck of the order (closest to its bound:
g_K at 9x200, 4.7e-5 of 5.9e-5 allowed).  The yardstick itself depends on the host, whose BLAS carries its sums
(g_K at 9x200 gave 1.5e-5 on one host and 3.5e-5 on another; neither moved with the thread count).  transform_points: the bounds are derived (see
test_transform_points_vs_float64), not measured.
"""
import functools

import pytest
import torch

DEV = "cuda:0"
U = 2.0 ** -24  # fp32 unit round-off
gpu = pytest.mark.gpu

# name: (B, L, H, W, seed, dropout, band, negative depths)
CASES = {
    "2x2": (2, 1, 2, 2, 0, 0.0, 0, 0),           # the smallest legal image: both replicated differences from the only pair
    "5x65": (1, 1, 5, 65, 6, 0.05, 2, 0),        # last row and last column alone in their tile (tx == 0 / ty == 0 global reads)
    "9x200": (1, 2, 9, 200, 0, 0.05, 3, 6),      # last row alone in the third tile row; L = 2 with one K; a few d < 0
    "37x131": (2, 3, 37, 131, 0, 0.05, 2, 0),    # ragged both ways; B, L > 1 with different K
    "70x257": (2, 2, 70, 257, 0, 0.05, 3, 0),    # column 256 alone in tile 5; 71 blocks > the 32 groups of vn_bwd_final_k
}
ALL = tuple(CASES)
HOLED = tuple(n for n in ALL if CASES[n][5] > 0)
K_SLOTS = ((0, 0), (0, 2), (1, 1), (1, 2))
MAPS = ("V", "N", "gV", "gN")
GRADS = ("g_depth", "g_K", "g_poses")


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ------------------------------------------------------------------ inputs, reference, yardstick (CPU, computed once)
def degenerate_mask(depth):
    """(B,L,H,W,1) bool: d > 0 and both stencil neighbours d <= 0 (the exact rule of the module docstring)."""
    d = depth[..., 0]
    inv = d <= 0
    hn = torch.cat([inv[..., :, 1:], inv[..., :, -2:-1]], -1)
    vn = torch.cat([inv[..., 1:, :], inv[..., -2:-1, :]], -2)
    return ((d > 0) & hn & vn).unsqueeze(-1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(depth, K, poses, degenerate, weights[4]): fp32 CPU tensors shared by every test -- never modified."""
    from gradslam_amd.synthetic import make_sequence

    B, L, H, W, seed, dropout, band, n_neg = CASES[name]
    _, depth, K, P = make_sequence(B, L, H, W, seed=seed, dropout=dropout, band=band)
    K = K.clone()
    if B > 1:
        K[1, 0, 0, 0] *= 1.1
        K[1, 0, 1, 1] *= -0.9
        K[1, 0, 0, 2] += 1.5
        K[1, 0, 1, 2] -= 0.75
    g = torch.Generator().manual_seed(100 + seed)
    if n_neg:
        flat = depth.view(-1)
        valid = torch.nonzero(flat > 0)[:, 0]
        pick = valid[torch.randperm(valid.numel(), generator=g)[:n_neg]]
        flat[pick] = -flat[pick]
    deg = degenerate_mask(depth)
    w = [torch.randn(B, L, H, W, 3, generator=g) for _ in range(4)]
    keep = (~deg).float()
    w[1], w[3] = w[1] * keep, w[3] * keep
    return depth, K, P, deg, tuple(w)


def _oracle(name, dtype, subset, poses):
    """The oracle in `dtype`: the four maps and the gradients of sum_{i in subset} (out_i * w_i).sum()."""
    from oracle import maps

    depth0, K0, P0, _, w = inputs(name)
    depth, K = (x.to(dtype).clone().requires_grad_(True) for x in (depth0, K0))  # (.to alone would hand back the shared input)
    P = P0.to(dtype).clone().requires_grad_(True) if poses else None
    outs = maps.all_maps(depth, K, P)
    loss = sum((outs[i] * w[i].to(dtype)).sum() for i in subset)
    leaves = (depth, K) + ((P,) if poses else ())
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    out = {n: o.detach() for n, o in zip(MAPS, outs)}
    out.update({n: g for n, g in zip(GRADS, grads)})
    return out


@functools.lru_cache(maxsize=None)
def reference(name, subset=(0, 1, 2, 3), poses=True):
    """(float64 reference, float32 CPU oracle) of every quantity."""
    return _oracle(name, torch.float64, subset, poses), _oracle(name, torch.float32, subset, poses)


def max_err(a, ref, mask=None):
    e = (a.double().cpu() - ref.double()).abs()
    if mask is not None:
        e = e * mask
    return float(e.max())


def bound_of(yard, ref_max, floor_ulps=8):
    return max(4.0 * yard, floor_ulps * U * ref_max)


def check(tag, q, got, name, subset=(0, 1, 2, 3), poses=True, extra=0.0):
    """`got` (the kernel's) against the float64 reference of quantity q within the yardstick bound (+ `extra`, a derived term)."""
    ref64, ref32 = reference(name, subset, poses)
    mask = (~inputs(name)[3]).double() if q in ("N", "gN") else None
    yard = max_err(ref32[q], ref64[q], mask)
    ref_max = float(ref64[q].abs().max())
    bound = bound_of(yard, ref_max) + extra
    err = max_err(got, ref64[q], mask)
    print("{} {} {}: ref max {:.3e} yard {:.3e} kernel {:.3e} bound {:.3e}".format(tag, name, q, ref_max, yard, err, bound))
    assert torch.isfinite(got).all(), (tag, name, q)
    assert err <= bound, (tag, name, q, err, bound)


def dev(x):
    return None if x is None else x.to(DEV)


# ------------------------------------------------------------------ CPU part
def test_degenerate_share_is_small_and_the_rule_is_exercised():
    for name in ALL:
        depth, _, _, deg, w = inputs(name)
        n_valid, n_deg = int((depth > 0).sum()), int(deg.sum())
        print(name, "valid", n_valid, "degenerate", n_deg, "share", n_deg / n_valid)
        assert n_deg <= 0.02 * n_valid, name
        assert (n_deg >= 1) == (name in HOLED), name
        assert not bool((w[1] * deg).any()) and not bool((w[3] * deg).any())
    assert int((inputs("9x200")[0] < 0).sum()) == CASES["9x200"][7]
    K = inputs("37x131")[1]
    assert K[1, 0, 1, 1] < 0 < K[0, 0, 1, 1] and not torch.equal(K[0], K[1])


def plane_case(dtype):
    """A plane n . X = c seen through K (negative fy) at 5 x 65: (depth, K, n), depth exact in `dtype` from float64."""
    from gradslam_amd.synthetic import make_intrinsics

    H, W = 5, 65
    K = make_intrinsics(H, W).clone()
    K[0, 0, 1, 1] *= -0.9
    n = torch.tensor([0.3, -0.2, 1.0], dtype=torch.float64)
    n = n / n.norm()
    Kd = K[0, 0].double()
    a, c = 1.0 / (Kd[0, 0] + 1e-6), -Kd[0, 2] / (Kd[0, 0] + 1e-6)
    e, f = 1.0 / (Kd[1, 1] + 1e-6), -Kd[1, 2] / (Kd[1, 1] + 1e-6)
    hh, ww = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    r = torch.stack([a * ww + c, e * hh + f, torch.ones_like(ww)], -1)
    depth = 2.0 / (r * n).sum(-1)
    assert bool((depth > 0.5).all())
    return depth.view(1, 1, H, W, 1).to(dtype), K.to(dtype), n


def plane_sign(n):
    """The one sign s with N = s * n over the whole image (it depends on the signs of fx, fy only): read off the float64 oracle."""
    from oracle import maps

    depth, K, _ = plane_case(torch.float64)
    N = maps.all_maps(depth, K, None)[1]
    return float(torch.sign((N[0, 0, 2, 30] * n).sum())), N


def test_plane_closed_form_in_float64():
    """The reference itself: on an exact plane every stencil difference lies in the plane, the replicated ones of the last
    row and column too, so the float64 oracle's normal is +-n everywhere to float64 rounding."""
    _, _, n = plane_case(torch.float64)
    s, N = plane_sign(n)
    err = float((N - s * n).abs().max())
    print("plane: float64 oracle vs closed form", err)
    assert abs(s) == 1.0 and err < 1e-9


# ------------------------------------------------------------------ forward
@gpu
@pytest.mark.parametrize("name", ALL)
def test_forward_maps_vs_float64(gs, name):
    depth, K, P, _, _ = inputs(name)
    outs = gs.ops.vertex_normal_maps_raw(dev(depth), dev(K), dev(P))
    invalid = (depth <= 0).expand(-1, -1, -1, -1, 3)
    assert name == "2x2" or bool(invalid.any())
    for q, o in zip(MAPS, outs):
        check("fwd", q, o, name)
        assert bool((o.cpu()[invalid] == 0).all()), (name, q)


@gpu
@pytest.mark.parametrize("name", ["5x65", "37x131"])
def test_forward_output_subsets_are_the_same_bits(gs, name):
    depth, K, P = (dev(x) for x in inputs(name)[:3])
    V, N, gV, gN = gs.ops.vertex_normal_maps_raw(depth, K, P)
    lV, lN, x, y = gs.ops.vertex_normal_maps_raw(depth, K, P, want_local=True, want_global=False)
    assert x is None and y is None and torch.equal(lV, V) and torch.equal(lN, N)
    x, y, ggV, ggN = gs.ops.vertex_normal_maps_raw(depth, K, P, want_local=False, want_global=True)
    assert x is None and y is None and torch.equal(ggV, gV) and torch.equal(ggN, gN)
    _, _, nV, nN = gs.ops.vertex_normal_maps_raw(depth, K, None)
    assert torch.equal(nV, V) and torch.equal(nN, N)
    _, _, nV, nN = gs.ops.vertex_normal_maps_raw(depth, K, None, want_local=False, want_global=True)
    assert torch.equal(nV, V) and torch.equal(nN, N)


@gpu
def test_forward_plane_normal_is_the_closed_form(gs):
    """N = +-n on a plane: the reference is the closed form, the yardstick the float32 CPU oracle on the same fp32 depth."""
    from oracle import maps

    depth, K, n = plane_case(torch.float32)
    s, _ = plane_sign(n)
    target = (s * n).view(1, 1, 1, 1, 3)
    N32 = maps.all_maps(depth, K, None)[1]
    N = gs.ops.vertex_normal_maps_raw(dev(depth), dev(K), None, want_global=False)[1].cpu()
    for tag, sl in (("interior", (Ellipsis, slice(0, -1), slice(0, -1), slice(None))), ("whole image", (Ellipsis,))):
        yard = float((N32.double() - target)[sl].abs().max())
        err = float((N.double() - target)[sl].abs().max())
        bound = bound_of(yard, 1.0)
        print("plane {}: yard {:.3e} kernel {:.3e} bound {:.3e}".format(tag, yard, err, bound))
        assert err <= bound, tag


# ------------------------------------------------------------------ backward
def kernel_grads(gs, name, subset=(0, 1, 2, 3), poses=True):
    depth, K, P, _, w = inputs(name)
    g = [dev(w[i]) if i in subset else None for i in range(4)]
    return gs.ops.vertex_normal_maps_backward_raw(dev(depth), dev(K), dev(P) if poses else None, *g)


def check_grads(tag, got, name, subset=(0, 1, 2, 3), poses=True):
    g_depth, g_K, g_P = got
    check(tag, "g_depth", g_depth, name, subset, poses)
    check(tag, "g_K", g_K, name, subset, poses)
    other = torch.ones(4, 4, dtype=torch.bool)
    for i, j in K_SLOTS:
        other[i, j] = False
    assert bool((g_K.cpu()[..., other] == 0).all()), (tag, name)
    if poses:
        check(tag, "g_poses", g_P, name, subset, poses)
        assert bool((g_P.cpu()[..., 3, :] == 0).all()), (tag, name)
    else:
        assert g_P is None


@gpu
@pytest.mark.parametrize("name", ALL)
def test_backward_all_four_vs_float64(gs, name):
    """Through the autograd node (ops.vertex_normal_maps), all four upstream gradients at once."""
    depth0, K0, P0, _, w = inputs(name)
    depth, K, P = (dev(x).requires_grad_(True) for x in (depth0, K0, P0))
    outs = gs.ops.vertex_normal_maps(depth, K, P)
    sum((o * dev(wi)).sum() for o, wi in zip(outs, w)).backward()
    check_grads("bwd", (depth.grad, K.grad, P.grad), name)
    raw = kernel_grads(gs, name)
    for a, b in zip(raw[::2], (depth.grad, P.grad)):  # one addition into zeros per element: the same bits
        assert torch.equal(a, b.view_as(a))
    check_grads("bwd raw", raw, name)


def c_backward(gs, name, subset, entry="gs_vertex_normal_maps_backward"):
    """The C entry point with a workspace of this test's own, every word of it a NaN (0xFF bytes)."""
    nv = gs._native
    depth, K, P = (dev(x).contiguous() for x in inputs(name)[:3])
    w = inputs(name)[4]
    g = [dev(w[i]).contiguous() if i in subset else None for i in range(4)]
    B, L, H, W = depth.shape[:4]
    n = nv.ws_bytes(entry + "_ws_bytes", B, L, H, W)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)
    assert bool(torch.isnan(ws.view(torch.float32)).all())
    out = [torch.zeros_like(x) for x in (depth, K, P)]
    nv.call(entry, nv.ptr(depth), nv.ptr(K), nv.ptr(P), B, L, H, W, *[nv.ptr(x) for x in g], *[nv.ptr(x) for x in out], nv.ptr(ws), n,
            nv.stream())
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=MAPS)
@pytest.mark.parametrize("name", ["37x131", "70x257"])
def test_backward_each_upstream_alone_vs_float64(gs, name, which):
    """One upstream gradient, the others absent (NULL).  Vertices only: pass 1 does not run, so nothing of the workspace's
    tail is written -- and nothing of it may be read: the workspace is all NaNs."""
    subset = (which,)
    if which in (0, 2):
        got = c_backward(gs, name, subset)
        check_grads("alone/C " + MAPS[which], got, name, subset)
        raw = kernel_grads(gs, name, subset)  # the same bits but for K, whose L terms arrive by atomics in any order
        assert torch.equal(got[0], raw[0]) and torch.equal(got[2], raw[2])
    else:
        check_grads("alone " + MAPS[which], kernel_grads(gs, name, subset), name, subset)
        check_grads("alone/C " + MAPS[which], c_backward(gs, name, subset), name, subset)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_backward_without_poses_vs_float64(gs, name):
    check_grads("no poses", kernel_grads(gs, name, poses=False), name, poses=False)


@functools.lru_cache(maxsize=None)
def k_terms_abs_sum(name):
    """sum_l |the K gradient of frame (b, l)| in float64, (B,1,4,4): what bounds the partial sums of the L atomic additions."""
    from oracle import maps

    depth0, K0, P0, _, w = inputs(name)
    tot = torch.zeros_like(K0, dtype=torch.float64)
    for l in range(depth0.shape[1]):
        K = K0.double().requires_grad_(True)
        outs = maps.all_maps(depth0[:, l:l + 1].double(), K, P0[:, l:l + 1].double())
        (gK,) = torch.autograd.grad(sum((o * wi[:, l:l + 1].double()).sum() for o, wi in zip(outs, w)), (K,))
        tot += gK.abs()
    return tot


@gpu
@pytest.mark.parametrize("name", ["9x200", "37x131"])
def test_backward_into_adds_once_per_element(gs, name):
    depth0, K0, P0, _, w = inputs(name)
    depth, K, P = dev(depth0), dev(K0), dev(P0)
    g = torch.Generator().manual_seed(5)
    pre = [torch.randn(x.shape, generator=g).to(DEV) for x in (depth0, K0, P0)]
    raw = kernel_grads(gs, name)
    into = [p.clone() for p in pre]
    gs.ops.vertex_normal_maps_backward_into(depth, K, P, *[dev(x) for x in w], *into)
    assert torch.equal(into[0], pre[0] + raw[0])
    assert torch.equal(into[2], pre[2] + raw[2])
    # K: p + t_1 + ... + t_L by atomics: L roundings, each at most 2^-24 * |a partial sum| <= 2^-24 * (|p| + sum_l |t_l|), on top
    # of the error of the terms themselves (the bound of the raw call)
    L = depth0.shape[1]
    extra = float((L * U * (pre[1].cpu().double().abs() + k_terms_abs_sum(name))).max())
    check("into", "g_K", into[1].cpu().double() - pre[1].cpu().double(), name, extra=extra)
    other = torch.ones(4, 4, dtype=torch.bool)
    for i, j in K_SLOTS:
        other[i, j] = False
    assert torch.equal(into[1][..., other.to(DEV)], pre[1][..., other.to(DEV)])


@gpu
@pytest.mark.parametrize("name", ["2x2", "5x65", "37x131", "70x257"])
def test_backward_deterministic_entry(gs, name):
    L = CASES[name][1]
    default = kernel_grads(gs, name)
    old = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert gs.ops.deterministic()
        det = kernel_grads(gs, name)
        det2 = kernel_grads(gs, name)
        det_c = c_backward(gs, name, (0, 1, 2, 3), entry="gs_vertex_normal_maps_backward_det")
    finally:
        torch.use_deterministic_algorithms(old)
    check_grads("det", det, name)
    check_grads("det/C", det_c, name)
    assert torch.equal(det[0], default[0]) and torch.equal(det[2], default[2])
    if L == 1:
        assert torch.equal(det[1], default[1])
    for a, b, c in zip(det, det2, det_c):
        assert torch.equal(a, b) and torch.equal(a, c)


# ------------------------------------------------------------------ get_alpha
ALPHA_SIGMA, ALPHA_EPS = 0.6, 1e-7


def alpha_points(n):
    """n points, alternately clearly above and clearly below the lower clamp (float64 alpha outside [eps / 2, 2 eps])."""
    g = torch.Generator().manual_seed(n)
    dirs = torch.randn(n, 3, generator=g, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    r = torch.where(torch.arange(n) % 2 == 0, 0.05 + 3.15 * u, 3.6 + 2.4 * u)
    return (dirs * r[:, None]).float(), torch.randn(n, generator=g)


def alpha_statements(p, sigma, eps):
    return torch.clamp(torch.exp(-torch.sum(p ** 2, -1) / (2 * (sigma ** 2))), eps, 1.01)


@gpu
@pytest.mark.parametrize("n", [1, 255, 257, 2 ** 20 + 300])
def test_get_alpha_forward_and_gradient_vs_float64(gs, n):
    """n = 2^20 + 300: the first size at which the grid-stride loops of alpha_k / alpha_bwd_k (4096 x 256 threads) make a
    second trip.  Yardstick: torch CPU float32 of the same statements; margin 4 (the device expf is not the host's), floor 4 ulp."""
    p0, g0 = alpha_points(n)
    res = {}
    for dtype in (torch.float64, torch.float32):
        p = p0.to(dtype).clone().requires_grad_(True)
        a = alpha_statements(p, ALPHA_SIGMA, ALPHA_EPS)
        a.backward(g0.to(dtype))
        res[dtype] = (a.detach(), p.grad)
    a64, gp64 = res[torch.float64]
    raw64 = torch.exp(-torch.sum(p0.double() ** 2, -1) / (2 * ALPHA_SIGMA ** 2))
    passing, clamped = raw64 > 2 * ALPHA_EPS, raw64 < ALPHA_EPS / 2
    assert bool((passing | clamped).all()) and bool(passing.any()) and (n == 1 or bool(clamped.any()))  # (n = 1: the one point passes)
    p = dev(p0).requires_grad_(True)
    a = gs.ops.get_alpha_lastdim(p, ALPHA_SIGMA, ALPHA_EPS)
    a.backward(dev(g0))
    for q, got, ref, f32 in (("alpha", a.detach(), a64, res[torch.float32][0]), ("g_points", p.grad, gp64, res[torch.float32][1])):
        yard, ref_max = max_err(f32, ref), float(ref.abs().max())
        err, bound = max_err(got, ref), bound_of(max_err(f32, ref), ref_max, floor_ulps=4)
        print("alpha n={} {}: ref max {:.3e} yard {:.3e} kernel {:.3e} bound {:.3e}".format(n, q, ref_max, yard, err, bound))
        assert err <= bound, q
    assert bool((a.detach().cpu()[clamped] == torch.tensor(ALPHA_EPS, dtype=torch.float32)).all())
    assert bool((p.grad.cpu()[clamped] == 0).all()) and bool((gp64[clamped] == 0).all())
    assert bool((p.grad.cpu()[passing & (g0 != 0)] != 0).any(-1).all())


# ------------------------------------------------------------------ transform_points
def transform_case(n):
    g = torch.Generator().manual_seed(n)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = q
    T[:3, 3] = torch.tensor([0.7, -1.3, 2.1], dtype=torch.float64)
    return 2.0 * torch.randn(n, 3, generator=g), T.float(), torch.randn(n, 3, generator=g)


@gpu
@pytest.mark.parametrize("n", [1, 257, 524288 + 300])
def test_transform_points_vs_float64(gs, n):
    """n = 524288 + 300: the second trip of transform_k (2048 x 256 threads).  Derived bounds: a component of R p + t is three
    products and three additions, every rounding relative to a partial sum of magnitude <= sum_j |R_ij| |p_j| + |t_i|, hence
    4 * 2^-24 * that; the same for R^T g.  The T adjoint is a float32 sum of n terms: n * 2^-24 * sum |g| |p|."""
    p0, T0, g0 = transform_case(n)
    pd, Td, gd = p0.double(), T0.double(), g0.double()
    R, t = Td[:3, :3], Td[:3, 3]
    p, T = dev(p0).requires_grad_(True), dev(T0).requires_grad_(True)
    out = gs.ops.transform_points(p, T)
    out.backward(dev(g0))
    cases = (("out", out.detach(), pd @ R.t() + t, 4 * U * (pd.abs() @ R.abs().t() + t.abs())),
             ("g_points", p.grad, gd @ R, 4 * U * (gd.abs() @ R.abs())),
             ("g_R", T.grad[:3, :3], gd.t() @ pd, n * U * (gd.abs().t() @ pd.abs())),
             ("g_t", T.grad[:3, 3], gd.sum(0), n * U * gd.abs().sum(0)))
    for q, got, ref, bound in cases:
        excess = ((got.double().cpu() - ref).abs() - bound).max()
        print("transform n={} {}: max err {:.3e} max bound {:.3e}".format(n, q, float((got.double().cpu() - ref).abs().max()), float(bound.max())))
        assert torch.isfinite(got).all() and excess <= 0, q
    assert bool((T.grad[3] == 0).all())


@gpu
def test_transform_points_device_count_below_max_n(gs):
    nv = gs._native
    p0, T0, _ = transform_case(300)
    p, T = dev(p0).contiguous(), dev(T0).contiguous()
    sentinel = -1234.5
    out = torch.full_like(p, sentinel)
    count = torch.full((1,), 100, dtype=torch.int32, device=DEV)
    nv.call("gs_transform_points", nv.ptr(p), nv.ptr(count), 300, nv.ptr(T), nv.ptr(out), nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(out[100:], torch.full_like(out[100:], sentinel))
    assert torch.equal(out[:100], gs.ops.transform_points(p[:100].contiguous(), T))
    ref = p0[:100].double() @ T0[:3, :3].double().t() + T0[:3, 3].double()
    bound = 4 * U * (p0[:100].double().abs() @ T0[:3, :3].double().abs().t() + T0[:3, 3].double().abs())
    assert bool(((out[:100].double().cpu() - ref).abs() <= bound).all())
