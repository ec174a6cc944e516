"""The per-op ICP linearisation (gs_knn1_unpack, gs_icp_linearize, gs_icp_rows, gs_icp_linearize_backward and its
deterministic form) against a plain restatement of the operation, on hand-made nearest-neighbour keys.

`best` is an INPUT of these kernels: key = (float32 bits of d2) << 32 | j, or KEY_NONE = ~0 for "no target".  Building
the keys on the host gives exact control of the threshold verdict (strict d2 < thresh), of the target index and of the
fan-in, with no nearest-neighbour tie in the way.  One case takes its keys from ops.knn1_raw to show that the pieces fit.

The restatement (`_rows`, `_sums`) is make_row / accumulate_row / expand44 in torch:
    a = [n ; s x n],  b = (n.x (d.x - s.x) + n.y (d.y - s.y)) + n.z (d.z - s.z),
    row i kept  iff  i < ns  and  key != KEY_NONE  and  (thresh < 0 or d2 < thresh),
    H = sum a a^T,  g = sum a b,  e = sum b^2,  count.

Two kinds of comparison, neither measured on the code under test:
  * integer-lattice inputs (coordinates and normals from {-1, 0, 1}): every product and every partial sum is an integer
    below 2^24, so float32 arithmetic is exact in ANY order and the kernels owe the float64 result bit for bit.  The
    condition (sum of absolute values < 2^24 behind every accumulator and every gradient element) is asserted on the CPU.
  * real-valued inputs: the rows are the kernel's bits (float32 elementwise, asserted), and each sum lies within
    2 h 2^-24 sum|term| of the float64 sum, h = the number of additions a term can pass through in the reduction tree
    (computed from the launch constants below); gradients within 64 roundings of the row algebra plus the fan-in.
"""
import functools
import math

import pytest
import torch

DEV = "cuda:0"

KEY_NONE = -1                 # ~0 as the int64 ops.knn1_raw returns
LIN_T, LIN_MAXB, RP_LOADS = 256, 1024, 16   # gs_icp_assoc.hpp / gs_icp_reduce.hpp
NT = 97
TH = 2.0                      # the hand-made squared distance that doubles as threshold
U = 2.0 ** -24                # float32 unit roundoff
EXACT = 2.0 ** 24

# wave and block seams of LIN_T; 32 / 33 partial rows; one / two rounds of reduce_partials; the block cap and grid stride
SIZES = [1, 63, 64, 65, 255, 256, 257, 256 * 31 + 1, 256 * 32, 256 * 32 + 1, 256 * 512, 256 * 512 + 1, 262144, 262145, 300000]
assert LIN_T * LIN_MAXB == 262144 and 32 * RP_LOADS == 512
BWD_CASES = [(1, 1), (1, 97), (257, 1), (257, 97), (65536, 1), (65536, 97)]


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ---------------------------------------------------------------------------------------------- keys and inputs
def _pack(d2, j):
    """(float32 bits of d2 << 32) | j as int64; d2 >= 0, so the sign bit stays clear."""
    return (d2.to(torch.float32).view(torch.int32).to(torch.int64) << 32) | j.to(torch.int64)


def _unpack(keys):
    none = keys == KEY_NONE
    j = torch.where(none, torch.zeros_like(keys), keys & 0xFFFFFFFF)
    d2 = (keys >> 32).to(torch.int32).view(torch.float32)
    return none, j, d2


def _around(x):
    x = torch.tensor(x, dtype=torch.float32)
    return torch.nextafter(x, torch.tensor(0.0)), x, torch.nextafter(x, torch.tensor(float("inf")))


def _threshold_keys(ns, nt, g):
    """Keys whose d2 is TH, the float32 below or the float32 above (about a third each); one row in sixteen has no target.
    Rows 0 and ns - 1 sit ON the threshold: the strict rule rejects them, a seam error cannot hide behind a kept row."""
    below, at, above = _around(TH)
    d2 = torch.stack([below, at, above])[torch.randint(0, 3, (ns,), generator=g)]
    d2[0], d2[ns - 1] = at, at
    keys = _pack(d2, torch.randint(0, nt, (ns,), generator=g))
    keys[torch.arange(ns) % 16 == 5] = KEY_NONE
    return keys


@functools.lru_cache(maxsize=None)
def _lattice(ns, nt, thresholded):
    """float32 CPU (src, tgt, nrm, keys, thresh): integer coordinates, normals NOT of unit length."""
    g = torch.Generator().manual_seed(100003 * ns + 17 * nt + int(thresholded))
    src, tgt, nrm = (torch.randint(-1, 2, (n, 3), generator=g).float() for n in (ns, nt, nt))
    tgt[0], nrm[0] = torch.tensor([1.0, 0.0, -1.0]), torch.tensor([1.0, -1.0, 1.0])  # (nt = 1 must not draw a zero normal)
    if thresholded:
        return src, tgt, nrm, _threshold_keys(ns, nt, g), TH
    d2 = torch.stack(_around(TH))[torch.randint(0, 3, (ns,), generator=g)]  # (ignored without a threshold)
    return src, tgt, nrm, _pack(d2, torch.randint(0, nt, (ns,), generator=g)), None


@functools.lru_cache(maxsize=None)
def _real(ns, nt, nscale, thresh):
    """Random clouds, normals of length nscale; d2 uniform in [0, 1) (hand-made: the kernels only compare it)."""
    g = torch.Generator().manual_seed(7919 * ns + nt)
    src, tgt = torch.rand(ns, 3, generator=g) * 2 - 1, torch.rand(nt, 3, generator=g) * 2 - 1
    nrm = torch.randn(nt, 3, generator=g, dtype=torch.float64)
    nrm = (nrm / nrm.norm(dim=-1, keepdim=True) * nscale).float()
    keys = _pack(torch.rand(ns, generator=g), torch.randint(0, nt, (ns,), generator=g))
    keys[torch.arange(ns) % 16 == 5] = KEY_NONE
    return src, tgt, nrm, keys, thresh


def _c_thresh(thresh):
    return -1.0 if thresh is None else float(thresh)


# ---------------------------------------------------------------------------------------------- the restatement
def _rows(src, tgt, nrm, keys, thresh, ns=None, dtype=torch.float64):
    """A (n,6), b (n,), keep (n,) bool, j (n,) in `dtype` elementwise arithmetic; rejected rows hold +0."""
    n_max = src.shape[0]
    none, j, d2 = _unpack(keys)
    keep = (torch.arange(n_max) < (n_max if ns is None else ns)) & ~none
    if thresh is not None and thresh >= 0:
        keep = keep & (d2 < torch.tensor(thresh, dtype=torch.float32))
    elif thresh is not None:
        raise ValueError("negative thresholds mean None at the C ABI only")
    s, d, n = src.to(dtype), tgt.to(dtype)[j], nrm.to(dtype)[j]
    sx, sy, sz = s.unbind(1)
    nx, ny, nz = n.unbind(1)
    dx, dy, dz = d.unbind(1)
    a = torch.stack([nx, ny, nz, nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy], 1)
    b = (nx * (dx - sx) + ny * (dy - sy)) + nz * (dz - sz)
    zero = torch.zeros((), dtype=dtype)
    return torch.where(keep[:, None], a, zero), torch.where(keep, b, zero), keep, j


def _sums(A, b, keep):
    """(44,) float64: H | g | e | count, and the same with every term replaced by its absolute value."""
    A, b = A.double(), b.double()
    cnt = keep.sum().double().view(1)
    out = torch.cat([(A.T @ A).reshape(-1), A.T @ b, (b @ b).view(1), cnt])
    Aa, ba = A.abs(), b.abs()
    return out, torch.cat([(Aa.T @ Aa).reshape(-1), Aa.T @ ba, (ba @ ba).view(1), cnt])


def _ref44(case, ns=None):
    src, tgt, nrm, keys, thresh = case
    return _sums(*_rows(src, tgt, nrm, keys, thresh, ns)[:3])


def _autograd_ref(case, gH, gg, ge, ns=None):
    """float64 autograd through the restatement with the selection (keep, j) frozen -> (g_src, g_tgt, g_nrm)."""
    src, tgt, nrm, keys, thresh = case
    n = src.shape[0] if ns is None else ns
    s = src[:n].double().requires_grad_(True)         # (rows beyond the count never enter: they may hold NaN)
    t, m = tgt.double().requires_grad_(True), nrm.double().requires_grad_(True)
    A, b, _, _ = _rows(s, t, m, keys[:n], thresh)
    loss = ((A.T @ A) * gH.double()).sum() + ((A.T @ b) * gg.double().view(-1)).sum() + (b @ b) * ge.double()
    grads = torch.autograd.grad(loss, (s, t, m), allow_unused=True)
    return tuple(torch.zeros_like(x) if g is None else g for x, g in zip((s, t, m), grads))


def _adjoint_rows(G43, s, d, n, absolute=False):
    """linearize_bwd_k's row algebra in float64 -> per-row (s_bar, d_bar, n_bar).  absolute=True evaluates the same
    expression on absolute values with every subtraction turned into an addition: an upper bound of the magnitude of
    every intermediate, which is what a rounding-error bound scales with."""
    sg = 1.0 if absolute else -1.0
    G, s, d, n = (x.double().abs() if absolute else x.double() for x in (G43, s, d, n))
    gH, gg, ge = G[:36].view(6, 6), G[36:42], G[42]
    sx, sy, sz = s.unbind(1)
    nx, ny, nz = n.unbind(1)
    dm = d + sg * s
    a = torch.stack([nx, ny, nz, nz * sy + sg * ny * sz, nx * sz + sg * nz * sx, ny * sx + sg * nx * sy], 1)
    b = (n * dm).sum(1)
    ab = a @ (gH + gH.T) + b[:, None] * gg[None, :]
    bb = 2.0 * ge * b + a @ gg
    an, (cx, cy, cz) = ab[:, :3], ab[:, 3:].unbind(1)
    s_bar = torch.stack([ny * cz + sg * nz * cy, nz * cx + sg * nx * cz, nx * cy + sg * ny * cx], 1) + sg * bb[:, None] * n
    n_bar = an + torch.stack([cy * sz + sg * cz * sy, cz * sx + sg * cx * sz, cx * sy + sg * cy * sx], 1) + bb[:, None] * dm
    return s_bar, bb[:, None] * n, n_bar


def _abs_grads(case, G43, ns=None):
    """(|g_src| bound (n,3), sum of |contribution| bounds per target element for g_tgt and g_nrm (nt,3), fan-in (nt,))."""
    src, tgt, nrm, keys, thresh = case
    n_rows = src.shape[0] if ns is None else ns
    _, _, keep, j = _rows(src[:n_rows], tgt, nrm, keys[:n_rows], thresh)
    s_bar, d_bar, n_bar = _adjoint_rows(G43, src[:n_rows], tgt[j], nrm[j], absolute=True)
    k = keep.double()[:, None]
    nt = tgt.shape[0]
    z = lambda: torch.zeros(nt, 3, dtype=torch.float64)
    return (s_bar * k, z().index_add_(0, j, d_bar * k), z().index_add_(0, j, n_bar * k),
            torch.zeros(nt, dtype=torch.float64).index_add_(0, j, keep.double()))


def _upstream(seed, lattice):
    g = torch.Generator().manual_seed(seed)
    if lattice:  # {-1, 0, 1}; gH is not symmetric, and ge is the non-zero 1 so that "ge alone" is a test
        gH, gg = (torch.randint(-1, 2, shape, generator=g).float() for shape in ((6, 6), (6, 1)))
        gH[0, 1], gH[1, 0] = 1.0, -1.0
        return gH, gg, torch.tensor(1.0)
    return torch.randn(6, 6, generator=g), torch.randn(6, 1, generator=g), torch.randn((), generator=g)


def _g43(gH, gg, ge):
    return torch.cat([gH.reshape(-1), gg.reshape(-1), ge.reshape(-1)]).float()


def _h(ns):
    """Additions a term can pass through: the thread's own loop, 6 butterfly levels, 4 waves, the rows one thread of
    reduce_partials adds, its 32 group sums."""
    nb = min(max(math.ceil(ns / LIN_T), 1), LIN_MAXB)
    return math.ceil(ns / (LIN_T * nb)) + 6 + 4 + math.ceil(nb / 32) + 32


# ---------------------------------------------------------------------------------------------- CPU: the conditions
def test_lattice_sums_stay_exact_in_float32():
    """The condition under which bitwise equality is owed: behind each of the 29 accumulators (and so behind each of the
    44 output words) the sum of ABSOLUTE values is below 2^24, so every partial sum in any order is an exactly
    representable integer.  Checked for every lattice input the GPU tests use."""
    for ns in SIZES + [300]:
        for thresholded in (False, True):
            case = _lattice(ns, NT, thresholded)
            ref, ref_abs = _ref44(case)
            assert float(ref_abs.max()) < EXACT, (ns, thresholded, float(ref_abs.max()))
            assert torch.equal(ref, ref.round()) and float(ref[43]) <= ns
            keep = _rows(*case)[2]
            if thresholded:
                assert not keep[0] and not keep[ns - 1]
                if ns >= 255:
                    _, _, d2 = _unpack(case[3])
                    below, at, above = _around(TH)
                    assert all(int((d2 == v).sum()) > ns // 5 for v in (below, at, above))
                    assert 0 < int(keep.sum()) < ns // 2 and int((case[3] == KEY_NONE).sum()) > 0
                    assert torch.equal(keep, (d2 == below) & (case[3] != KEY_NONE))
            else:
                assert bool(keep.all())


def test_lattice_gradients_stay_exact_in_float32():
    """Likewise for the reverse pass: every gradient element is an integer whose contributions' absolute values add up
    to less than 2^24 (65 536 rows on one target included), so atomics in any order and the fixed-point fold agree with
    float64 exactly."""
    for ns, nt in BWD_CASES + [(300, NT)]:
        for thresholded in (False, True):
            case = _lattice(ns, nt, thresholded)
            gH, gg, ge = _upstream(ns + nt, lattice=True)
            assert not torch.equal(gH, gH.T)
            a_src, a_tgt, a_nrm, _ = _abs_grads(case, _g43(gH, gg, ge))
            worst = max(float(x.max()) for x in (a_src, a_tgt, a_nrm))
            assert worst < EXACT, (ns, nt, thresholded, worst)
            for x in _autograd_ref(case, gH, gg, ge):
                assert torch.equal(x, x.round())


def test_explicit_adjoint_is_the_autograd_gradient():
    """_adjoint_rows (used for the error bounds only) is the gradient autograd derives from the restatement, and its
    absolute evaluation dominates it."""
    case = _real(8193, NT, 1.0, 0.5)
    src, tgt, nrm, keys, thresh = case
    gH, gg, ge = _upstream(3, lattice=False)
    ref_s, ref_t, ref_n = _autograd_ref(case, gH, gg, ge)
    _, _, keep, j = _rows(*case)
    assert 0.3 < float(keep.float().mean()) < 0.6
    k = keep.double()[:, None]
    G = _g43(gH, gg, ge)
    s_bar, d_bar, n_bar = _adjoint_rows(G, src, tgt[j], nrm[j])
    z = lambda: torch.zeros(NT, 3, dtype=torch.float64)
    mine = (s_bar * k, z().index_add_(0, j, d_bar * k), z().index_add_(0, j, n_bar * k))
    a_src, a_tgt, a_nrm, fan = _abs_grads(case, G)
    assert int(fan.sum()) == int(keep.sum())
    for got, ref, bound in zip(mine, (ref_s, ref_t, ref_n), (a_src, a_tgt, a_nrm)):
        assert bool(((got - ref).abs() <= 1e-12 * bound).all())
        assert bool((ref.abs() <= bound * (1 + 1e-12)).all())


# ---------------------------------------------------------------------------------------------- raw ABI helpers
def _dev(case):
    src, tgt, nrm, keys, _ = case
    return src.to(DEV), tgt.to(DEV), nrm.to(DEV), keys.to(DEV)


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _raw_linearize(nv, src, tgt, nrm, keys, ns_dev, max_ns, thresh, short=0):
    out = torch.full((44,), float("nan"), device=DEV)
    need = nv.ws_bytes("gs_icp_linearize_ws_bytes", max_ns)
    ws = nv.workspace(need, DEV, "linearize_test")
    nv.call("gs_icp_linearize", nv.ptr(src), nv.ptr(ns_dev), max_ns, nv.ptr(tgt), nv.ptr(nrm), nv.ptr(keys), _c_thresh(thresh),
            nv.ptr(out), nv.ptr(ws), need - short, nv.stream())
    return out


def _raw_rows(nv, src, tgt, nrm, keys, ns_dev, max_ns, thresh, A, b, keep):
    nv.call("gs_icp_rows", nv.ptr(src), nv.ptr(ns_dev), max_ns, nv.ptr(tgt), nv.ptr(nrm), nv.ptr(keys), _c_thresh(thresh),
            nv.ptr(A), nv.ptr(b), nv.ptr(keep), nv.stream())


def _raw_backward(nv, det, src, tgt, nrm, keys, ns_dev, max_ns, thresh, gout, g_src, g_tgt, g_nrm):
    nt = tgt.shape[0]
    if det:
        ws = nv.workspace(nv.ws_bytes("gs_icp_linearize_backward_det_ws_bytes", max_ns, nt), DEV, "linearize_bwd_det_test")
        nt_dev = _i32(nt)
        nv.call("gs_icp_linearize_backward_det", nv.ptr(src), nv.ptr(ns_dev), max_ns, nv.ptr(tgt), nv.ptr(nrm), nv.ptr(nt_dev), nt,
                nv.ptr(keys), _c_thresh(thresh), nv.ptr(gout), nv.ptr(g_src), nv.ptr(g_tgt), nv.ptr(g_nrm), nv.ptr(ws), ws.numel(),
                nv.stream())
    else:
        nv.call("gs_icp_linearize_backward", nv.ptr(src), nv.ptr(ns_dev), max_ns, nv.ptr(tgt), nv.ptr(nrm), nv.ptr(keys),
                _c_thresh(thresh), nv.ptr(gout), nv.ptr(g_src), nv.ptr(g_tgt), nv.ptr(g_nrm), nv.stream())
    torch.cuda.synchronize()


def _bits(x):
    return x.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- a) + b) lattice, forward
@pytest.mark.gpu
@pytest.mark.parametrize("ns", SIZES)
def test_linearize_lattice_is_exact(gs, ns):
    """gs_icp_linearize returns the float64 restatement exactly, all 44 words, whatever its reduction tree."""
    from gradslam_amd import ops

    for thresholded in (False, True):
        case = _lattice(ns, NT, thresholded)
        ref, _ = _ref44(case)
        src, tgt, nrm, keys = _dev(case)
        got = ops.icp_linearize_raw(src, tgt, nrm, keys, case[4]).cpu().double()
        assert torch.equal(got, ref), (ns, thresholded, (got - ref).abs().max(), got[43], ref[43])
        assert torch.equal(got[:36].view(6, 6), got[:36].view(6, 6).T)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", SIZES)
def test_rows_lattice_are_exact(gs, ns):
    """ops.icp_rows_raw on the same inputs: A, b and keep are the restatement's bits (rejected rows hold +0), and the
    sums rebuilt from them in float64 are gs_icp_linearize's output."""
    from gradslam_amd import ops

    for thresholded in (False, True):
        case = _lattice(ns, NT, thresholded)
        rA, rb, rkeep, _ = _rows(*case, dtype=torch.float32)
        src, tgt, nrm, keys = _dev(case)
        A, b, keep = (x.cpu() for x in ops.icp_rows_raw(src, tgt, nrm, keys, case[4]))
        assert keep.dtype == torch.uint8 and torch.equal(keep, rkeep.to(torch.uint8)), (ns, thresholded)
        assert torch.equal(_bits(A), _bits(rA)) and torch.equal(_bits(b), _bits(rb)), (ns, thresholded)
        assert not _bits(A)[~rkeep].any() and not _bits(b)[~rkeep].any()
        rebuilt, _ = _sums(A, b, keep.bool())
        assert torch.equal(rebuilt, ops.icp_linearize_raw(src, tgt, nrm, keys, case[4]).cpu().double()), (ns, thresholded)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 257, 256 * 32 + 1])
def test_gauss_newton_solve_compacts_the_kept_rows(gs, ns):
    """odometry.icputils.gauss_newton_solve without gradients: A, b and idx are the kept rows of gs_icp_rows on the keys
    of gs_knn1, in order.  (Lattice points on four targets: squared distances are small integers, 2.0 among them, and the
    rule is strict.)"""
    from gradslam_amd import ops
    from gradslam_amd.odometry.icputils import gauss_newton_solve

    src, tgt, nrm, _ = _dev(_lattice(ns, 4, False))
    best = ops.knn1_raw(src, tgt)
    d2, idx = ops.knn1_unpack(best)
    for thresh in (None, TH):
        A, b, keep = ops.icp_rows_raw(src, tgt, nrm, best, thresh)
        k = keep.bool()
        if thresh is not None:
            assert torch.equal(k, d2 < thresh)
            if ns > 1:
                assert bool((d2 == thresh).any()) and bool(k.any())
        with torch.no_grad():
            gA, gb, gidx = gauss_newton_solve(src[None], tgt[None], nrm[None], thresh)
        assert gA.shape == (int(k.sum()), 6) and gb.shape == (int(k.sum()), 1)
        assert torch.equal(_bits(gA), _bits(A[k])) and torch.equal(_bits(gb.view(-1)), _bits(b[k])) and torch.equal(gidx, idx[k])


# ---------------------------------------------------------------------------------------------- c) real values
@pytest.mark.gpu
@pytest.mark.parametrize("ns,nscale,thresh", [(257, 1.0, None), (8193, 1.0, 0.5), (131073, 1.0, None), (8193, 1e-3, None),
                                              (8193, 1e3, 0.5)])
def test_linearize_real_values_within_the_reduction_bound(gs, ns, nscale, thresh):
    """The rows are float32 elementwise arithmetic (asserted bitwise); each of the 43 sums lies within
    2 h 2^-24 sum|term| of their float64 sum, count exactly."""
    from gradslam_amd import ops

    case = _real(ns, NT, nscale, thresh)
    rA, rb, rkeep, _ = _rows(*case, dtype=torch.float32)
    ref, ref_abs = _sums(rA, rb, rkeep)
    src, tgt, nrm, keys = _dev(case)
    A, b, keep = (x.cpu() for x in ops.icp_rows_raw(src, tgt, nrm, keys, thresh))
    assert torch.equal(keep.bool(), rkeep) and torch.equal(_bits(A), _bits(rA)) and torch.equal(_bits(b), _bits(rb))
    got = ops.icp_linearize_raw(src, tgt, nrm, keys, thresh).cpu().double()
    h = _h(ns)
    tol = 2.0 * h * U * ref_abs[:43]
    err = (got[:43] - ref[:43]).abs()
    print("ns %d scale %g h %d worst err / tol %.3f" % (ns, nscale, h, float((err / tol).max())))
    assert float(got[43]) == float(ref[43]) and 0 < float(ref[43]) < ns
    assert bool((err <= tol).all()), (err / tol).max()


@pytest.mark.gpu
def test_keys_of_knn1_feed_the_linearisation(gs):
    """Keys from ops.knn1_raw on a random cloud: d2 is the float32 (dx^2 + dy^2) + dz^2 to the target the index names,
    and the minimum over all targets; with the median d2 as threshold (a value a key holds, so the strict rule has a
    row to reject) the sums are within the bound of the restatement on those keys."""
    from gradslam_amd import ops

    ns = 1000
    src, tgt, nrm, _, _ = _real(ns, NT, 1.0, None)
    keys = ops.knn1_raw(src.to(DEV), tgt.to(DEV)).cpu()
    none, j, d2 = _unpack(keys)
    diff = src[:, None, :] - tgt[None, :, :]
    all_d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    assert not none.any() and torch.equal(_bits(d2), _bits(all_d2.gather(1, j[:, None]).view(-1)))
    assert torch.equal(d2, all_d2.min(dim=1).values)
    thresh = float(d2.median())
    case = (src, tgt, nrm, keys, thresh)
    rA, rb, rkeep, _ = _rows(*case, dtype=torch.float32)
    assert int(rkeep.sum()) == int((d2 < thresh).sum()) < int((d2 <= thresh).sum())
    ref, ref_abs = _sums(rA, rb, rkeep)
    got = ops.icp_linearize_raw(*_dev(case), thresh).cpu().double()
    assert float(got[43]) == float(ref[43])
    assert bool(((got[:43] - ref[:43]).abs() <= 2.0 * _h(ns) * U * ref_abs[:43]).all())


# ---------------------------------------------------------------------------------------------- d) contracts
@pytest.mark.gpu
@pytest.mark.parametrize("ns_dev", [0, 1, 200, 300])
def test_device_count_below_max_ns(gs, ns_dev):
    """Rows at and beyond the device count are neither read (their sources are NaN) nor written (sentinels intact), by
    the forward kernels and by both backward entries; ns_dev = 300 is the plain case next to them."""
    from gradslam_amd import _native as nv

    max_ns = 300
    for thresholded in (False, True):
        case = _lattice(max_ns, NT, thresholded)
        thresh = case[4]
        src, tgt, nrm, keys = _dev(case)
        src = src.clone()
        src[ns_dev:] = float("nan")
        d_ns = _i32(ns_dev)
        ref, _ = _ref44(case, ns_dev)
        got = _raw_linearize(nv, src, tgt, nrm, keys, d_ns, max_ns, thresh).cpu().double()
        assert torch.equal(got, ref), (ns_dev, thresholded)

        A, b = torch.full((max_ns, 6), -5.0, device=DEV), torch.full((max_ns,), -5.0, device=DEV)
        keep = torch.full((max_ns,), 77, dtype=torch.uint8, device=DEV)
        _raw_rows(nv, src, tgt, nrm, keys, d_ns, max_ns, thresh, A, b, keep)
        rA, rb, rkeep, _ = _rows(*case, ns=ns_dev, dtype=torch.float32)
        A, b, keep = A.cpu(), b.cpu(), keep.cpu()
        assert torch.equal(_bits(A[:ns_dev]), _bits(rA[:ns_dev])) and torch.equal(_bits(b[:ns_dev]), _bits(rb[:ns_dev]))
        assert torch.equal(keep[:ns_dev], rkeep[:ns_dev].to(torch.uint8))
        assert bool((A[ns_dev:] == -5.0).all()) and bool((b[ns_dev:] == -5.0).all()) and bool((keep[ns_dev:] == 77).all())

        gH, gg, ge = _upstream(ns_dev + 1, lattice=True)
        gout = _g43(gH, gg, ge).to(DEV)
        ref_s, ref_t, ref_n = _autograd_ref(case, gH, gg, ge, ns_dev)
        for det in (False, True):
            g_src = torch.full((max_ns, 3), -5.0, device=DEV)
            g_tgt, g_nrm = (torch.zeros((NT, 3), device=DEV) if not det else torch.full((NT, 3), float("nan"), device=DEV)
                            for _ in range(2))
            _raw_backward(nv, det, src, tgt, nrm, keys, d_ns, max_ns, thresh, gout, g_src, g_tgt, g_nrm)
            assert bool((g_src[ns_dev:] == -5.0).all()), (ns_dev, det)
            assert torch.equal(g_src[:ns_dev].cpu().double(), ref_s), (ns_dev, det)
            assert torch.equal(g_tgt.cpu().double(), ref_t) and torch.equal(g_nrm.cpu().double(), ref_n), (ns_dev, det)


@pytest.mark.gpu
def test_all_keys_none(gs):
    """Every key KEY_NONE (what gs_knn1 writes for nt = 0): 44 zeros, keep all zero, every gradient zero -- next to the
    same call with real keys, which is none of that."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    ns = 300
    case = _lattice(ns, NT, False)
    src, tgt, nrm, keys = _dev(case)
    none = torch.full_like(keys, KEY_NONE)
    assert torch.equal(ops.knn1_raw(src, tgt, nt_dev=_i32(0)), none)
    gout = _g43(*_upstream(5, lattice=True)).to(DEV)
    for k, empty in ((keys, False), (none, True)):
        out = ops.icp_linearize_raw(src, tgt, nrm, k, None)
        A, b, keep = ops.icp_rows_raw(src, tgt, nrm, k, None)
        assert (not out.any()) == empty and (not keep.any()) == empty and (not A.any()) == empty and (not b.any()) == empty
        for det in (False, True):
            g_src = torch.full((ns, 3), float("nan"), device=DEV)
            g_tgt, g_nrm = (torch.zeros((NT, 3), device=DEV) if not det else torch.full((NT, 3), float("nan"), device=DEV)
                            for _ in range(2))
            _raw_backward(nv, det, src, tgt, nrm, k, _i32(ns), ns, None, gout, g_src, g_tgt, g_nrm)
            assert all((not _bits(x).any()) == empty for x in (g_src, g_tgt, g_nrm)), det
            assert all(bool(torch.isfinite(x).all()) for x in (g_src, g_tgt, g_nrm)), det


@pytest.mark.gpu
def test_max_ns_zero_with_real_buffers(gs):
    """max_ns = 0: gs_icp_linearize still produces its 44 words (zeros); the rows and both backward entries succeed and
    write nothing."""
    from gradslam_amd import _native as nv

    src, tgt, nrm, keys = _dev(_lattice(64, NT, False))
    d_ns = _i32(0)
    out = _raw_linearize(nv, src, tgt, nrm, keys, d_ns, 0, None)
    assert out.shape == (44,) and not _bits(out).any()
    A, b = torch.full((64, 6), -5.0, device=DEV), torch.full((64,), -5.0, device=DEV)
    keep = torch.full((64,), 77, dtype=torch.uint8, device=DEV)
    _raw_rows(nv, src, tgt, nrm, keys, d_ns, 0, None, A, b, keep)
    assert bool((A == -5.0).all()) and bool((b == -5.0).all()) and bool((keep == 77).all())
    gout = _g43(*_upstream(6, lattice=True)).to(DEV)
    for det in (False, True):
        g_src, g_tgt, g_nrm = (torch.full((n, 3), -5.0, device=DEV) for n in (64, NT, NT))
        _raw_backward(nv, det, src, tgt, nrm, keys, d_ns, 0, None, gout, g_src, g_tgt, g_nrm)
        assert all(bool((x == -5.0).all()) for x in (g_src, g_tgt, g_nrm)), det


@pytest.mark.gpu
def test_linearize_refuses_a_short_workspace(gs):
    from gradslam_amd import _native as nv

    src, tgt, nrm, keys = _dev(_lattice(64, NT, False))
    assert nv.ws_bytes("gs_icp_linearize_ws_bytes", 64) >= LIN_MAXB * 29 * 4
    with pytest.raises(RuntimeError) as e:
        _raw_linearize(nv, src, tgt, nrm, keys, _i32(64), 64, None, short=1)
    assert "gs_icp_linearize" in str(e.value) and "workspace too small" in str(e.value) and "code -2" in str(e.value)
    assert torch.equal(_raw_linearize(nv, src, tgt, nrm, keys, _i32(64), 64, None).cpu().double(), _ref44(_lattice(64, NT, False))[0])


@pytest.mark.gpu
def test_knn1_unpack_returns_the_keys_bits(gs):
    """dist2 is the key's upper word reinterpreted, idx its lower word zero-extended; either output may be NULL; rows at
    and beyond the device count are left alone."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    n, n_dev = 700, 513
    g = torch.Generator().manual_seed(4)
    d2 = torch.rand(n, generator=g) * 10.0
    d2[:4] = torch.tensor([0.0, float("inf"), 1e-45, 3.0e38])
    j = torch.randint(0, 2 ** 31 - 1, (n,), generator=g)
    j[4], j[5] = 0, 2 ** 31 - 1
    keys = _pack(d2, j)
    keys[6] = KEY_NONE
    want_bits, want_idx = (keys >> 32).to(torch.int32), keys & 0xFFFFFFFF
    got_d2, got_idx = ops.knn1_unpack(keys.to(DEV))
    assert torch.equal(_bits(got_d2).cpu(), want_bits) and torch.equal(got_idx.cpu(), want_idx)
    assert int(got_idx[6]) == 0xFFFFFFFF and int(_bits(got_d2)[6]) == -1
    for want_d2, want_i in ((True, False), (False, True), (True, True)):
        o_d2, o_idx = torch.full((n,), -5.0, device=DEV), torch.full((n,), -5, dtype=torch.int64, device=DEV)
        nv.call("gs_knn1_unpack", nv.ptr(keys.to(DEV)), nv.ptr(_i32(n_dev)), n, nv.ptr(o_d2) if want_d2 else None,
                nv.ptr(o_idx) if want_i else None, nv.stream())
        o_d2, o_idx = o_d2.cpu(), o_idx.cpu()
        assert torch.equal(_bits(o_d2[:n_dev]), want_bits[:n_dev]) if want_d2 else bool((o_d2 == -5.0).all())
        assert torch.equal(o_idx[:n_dev], want_idx[:n_dev]) if want_i else bool((o_idx == -5).all())
        assert bool((o_d2[n_dev:] == -5.0).all()) and bool((o_idx[n_dev:] == -5).all())


@pytest.mark.gpu
def test_zero_and_negative_user_thresholds_keep_nothing(gs):
    """ops._thresh: only None means "no threshold"; 0.0 keeps nothing (the rule is strict, d2 = 0 included) and a negative
    user threshold is clamped to 0.0, not passed to the C ABI where it would mean None."""
    from gradslam_amd import ops

    src, tgt, nrm, keys, _ = _lattice(300, NT, False)
    keys = keys.clone()
    keys[::2] = _pack(torch.zeros(150), keys[::2] & 0xFFFFFFFF)
    src, tgt, nrm, keys = src.to(DEV), tgt.to(DEV), nrm.to(DEV), keys.to(DEV)
    assert float(ops.icp_linearize_raw(src, tgt, nrm, keys, None)[43]) == 300.0
    assert float(ops.icp_linearize_raw(src, tgt, nrm, keys, 1e-30)[43]) == 150.0
    for thresh in (0.0, -0.0, -3.0):
        assert not ops.icp_linearize_raw(src, tgt, nrm, keys, thresh).any(), thresh
        A, b, keep = ops.icp_rows_raw(src, tgt, nrm, keys, thresh)
        assert not keep.any() and not A.any() and not b.any(), thresh


# ---------------------------------------------------------------------------------------------- e) the reverse pass
def _node_grads(ops, case, ups, det):
    """Gradients of ops.icp_linearize's outputs weighted by `ups` = (gH, gg, ge), any of them None."""
    src, tgt, nrm, keys = _dev(case)
    s, t, n = (x.clone().requires_grad_(True) for x in (src, tgt, nrm))
    old = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det)
    try:
        outs = ops.icp_linearize(s, t, n, keys, case[4])
        pairs = [(o, u.to(DEV).view(o.shape)) for o, u in zip(outs, ups) if u is not None]
        torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(old)
    return [x.grad.cpu() for x in (s, t, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("ns,nt", BWD_CASES)
def test_backward_lattice_is_exact(gs, ns, nt):
    """g_src, g_tgt and g_nrm equal the float64 gradient exactly -- through the autograd node under both settings of
    torch.use_deterministic_algorithms and through the two raw entries, which therefore agree bit for bit; rejected and
    KEY_NONE rows get a zero g_src, targets no kept row points to get zero."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    for thresholded in (False, True):
        case = _lattice(ns, nt, thresholded)
        gH, gg, ge = _upstream(ns + nt, lattice=True)
        ref = [x.float() for x in _autograd_ref(case, gH, gg, ge)]
        _, _, keep, j = _rows(*case)
        hit = torch.zeros(nt, dtype=torch.bool)
        hit[j[keep]] = True
        assert not ref[0][~keep].any() and not ref[1][~hit].any() and not ref[2][~hit].any()
        if ns > 1 and not thresholded:
            assert all(bool(x.any()) for x in ref)
        results = {("node", det): _node_grads(ops, case, (gH, gg, ge), det) for det in (False, True)}
        src, tgt, nrm, keys = _dev(case)
        gout = _g43(gH, gg, ge).to(DEV)
        for det in (False, True):
            g_src = torch.full((ns, 3), float("nan"), device=DEV)
            g_tgt, g_nrm = (torch.zeros((nt, 3), device=DEV) if not det else torch.full((nt, 3), float("nan"), device=DEV)
                            for _ in range(2))
            _raw_backward(nv, det, src, tgt, nrm, keys, _i32(ns), ns, case[4], gout, g_src, g_tgt, g_nrm)
            results[("raw", det)] = [g_src.cpu(), g_tgt.cpu(), g_nrm.cpu()]
        for key, got in results.items():
            for name, x, r in zip(("src", "tgt", "nrm"), got, ref):
                assert torch.equal(x, r), (key, thresholded, name, (x - r).abs().max())
            assert not _bits(got[0])[~keep].any(), (key, thresholded)


@pytest.mark.gpu
def test_backward_real_values_within_the_rounding_bound(gs):
    """8193 rows on 97 targets, the threshold rejecting about half: g_src within 64 roundings of the row algebra's
    magnitude, g_tgt / g_nrm within (fan-in + 64) roundings of the summed magnitudes of their contributions."""
    from gradslam_amd import ops

    case = _real(8193, NT, 1.0, 0.5)
    gH, gg, ge = _upstream(3, lattice=False)
    ref = _autograd_ref(case, gH, gg, ge)
    a_src, a_tgt, a_nrm, fan = _abs_grads(case, _g43(gH, gg, ge))
    keep = _rows(*case)[2]
    assert 0.3 < float(keep.float().mean()) < 0.6 and float(fan.min()) > 8
    tols = (64 * U * a_src, (fan[:, None] + 64) * U * a_tgt, (fan[:, None] + 64) * U * a_nrm)
    for det in (False, True):
        got = _node_grads(ops, case, (gH, gg, ge), det)
        for name, x, r, tol in zip(("src", "tgt", "nrm"), got, ref, tols):
            err = (x.double() - r).abs()
            print("det %d g_%s worst err / tol %.3f" % (det, name, float((err / tol.clamp_min(1e-300)).max())))
            assert bool((err <= tol).all()), (det, name)
        assert not _bits(got[0])[~keep].any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2])
def test_backward_with_one_upstream_alone(gs, which):
    """gH only, gg only, ge only on the 257-row lattice case: the node fills the missing upstreams with zeros."""
    from gradslam_amd import ops

    case = _lattice(257, NT, True)
    full = _upstream(257 + which, lattice=True)
    ups = tuple(u if k == which else None for k, u in enumerate(full))
    ref = _autograd_ref(case, *(u if k == which else torch.zeros_like(u) for k, u in enumerate(full)))
    assert any(bool(x.any()) for x in ref)
    for det in (False, True):
        got = _node_grads(ops, case, ups, det)
        for x, r in zip(got, ref):
            assert torch.equal(x.double(), r), (which, det)
