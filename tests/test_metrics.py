"""gs.metrics: chamfer distance, nearest neighbours, reconstruction figures (one HIP call, gs_chamfer) and trajectory errors.

The search is the ICP's exact 1-NN search, so its keys must equal the brute-force scan's bit for bit, whatever the row order
and with or without the cell-grid bucketing of the targets.  Statistics are fp64 sums of per-point fp32 values: any summation
order stays within n 2^-52 of the float64 reference.  Gradient bounds count fp32 roundings (U = 2^-24) and are stated per test.
"""
import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops
from gradslam_amd.structures.utils import pointclouds_from_rgbdimages
from gradslam_amd.synthetic import make_sequence

DEV = "cuda:0"
U = 2.0 ** -24  # unit roundoff of fp32
KEY_NONE = -1
SENTINEL = 0x5A5A5A5A5A5A5A5A
NEW_SYMBOLS = {"gs_chamfer_ws_bytes": 3, "gs_chamfer": 15, "gs_chamfer_backward_ws_bytes": 3, "gs_chamfer_backward": 16,
               "gs_chamfer_backward_det_ws_bytes": 3, "gs_chamfer_backward_det": 16}


def _align256(n):
    return -(-n // 256) * 256


def _cells(n):
    g = 1
    while g < 64 and 16 * g * g < n:
        g += 1
    return g ** 3


# ------------------------------------------------------------------ CPU: ABI and error contracts
def test_metrics_symbols_load():
    lib = nv.lib()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
    assert lib.gs_abi_version() == 3
    assert gs.metrics.chamfer_distance is not None and hasattr(ops, "_ChamferFn")


@pytest.mark.parametrize("B,Na,Nb", [(1, 1, 1), (1, 130, 49), (2, 5000, 3000), (3, 327, 1000), (1, 307200, 307200)])
def test_chamfer_workspace_sizes_follow_the_layout(B, Na, Nb):
    """The layout documented in include/gradslam_hip.h, piece by piece, each rounded up to 256 bytes."""
    lib = nv.lib()
    fwd = sum(_align256(12 * B * N) + 2 * _align256(4 * B * N) + _align256(24 * B * -(-N // 16)) for N in (Na, Nb))
    fwd += _align256(64 * B) + sum(_align256(4 * B * (_cells(N) + 1)) for N in (Na, Nb))
    fwd += sum(_align256(32 * B * -(-N // 64)) for N in (Na, Nb))
    assert lib.gs_chamfer_ws_bytes(B, Na, Nb) == fwd
    M = max(Na, Nb)
    det = _align256(32 * B * Na) + _align256(32 * B * Nb) + _align256(4) + _align256(4 * M) + _align256(96 * M)
    assert lib.gs_chamfer_backward_det_ws_bytes(B, Na, Nb) == det
    assert lib.gs_chamfer_backward_ws_bytes(B, Na, Nb) == 0  # float atomics into the outputs: no scratch
    for bad in (0, -1):
        assert lib.gs_chamfer_ws_bytes(bad, Na, Nb) == 0 and lib.gs_chamfer_backward_det_ws_bytes(bad, Na, Nb) == 0


def test_chamfer_refuses_bad_arguments_before_any_device_work():
    """NULL pointers and non-positive sizes return -1, a missing or short workspace -2 (the pointers below are never read:
    every check happens on the host before the first launch)."""
    lib = nv.lib()
    P = 4096  # a non-NULL stand-in
    inf = float("inf")
    ok_fwd = [P, P, 10, P, P, 7, 1, inf, 1, P, P, P, P, 1 << 20, None]
    for pos in (0, 1, 3, 4, 9, 10, 11):  # a, a_counts, b, b_counts, stats, keys_ab, keys_ba
        args = list(ok_fwd)
        args[pos] = None
        assert lib.gs_chamfer(*args) == -1, pos
    for pos, bad in ((2, 0), (2, -4), (5, 0), (6, 0), (6, -1)):  # Na_max, Nb_max, B
        args = list(ok_fwd)
        args[pos] = bad
        assert lib.gs_chamfer(*args) == -1, pos
    args = list(ok_fwd)
    args[12], args[13] = None, 0
    assert lib.gs_chamfer(*args) == -2
    args = list(ok_fwd)
    args[13] = lib.gs_chamfer_ws_bytes(1, 10, 7) - 1
    assert lib.gs_chamfer(*args) == -2
    assert b"gs_chamfer" in lib.gs_last_error()

    ok_bwd = [P, P, 10, P, P, 7, 1, P, P, P, P, P, P, P, 1 << 20, None]
    for fn in (lib.gs_chamfer_backward, lib.gs_chamfer_backward_det):
        for pos in (0, 1, 3, 4, 7, 8, 9, 10, 11, 12):
            args = list(ok_bwd)
            args[pos] = None
            assert fn(*args) == -1, pos
        for pos, bad in ((2, 0), (5, -1), (6, 0)):
            args = list(ok_bwd)
            args[pos] = bad
            assert fn(*args) == -1, pos
    args = list(ok_bwd)
    args[13], args[14] = None, 0
    assert lib.gs_chamfer_backward_det(*args) == -2
    args = list(ok_bwd)
    args[14] = lib.gs_chamfer_backward_det_ws_bytes(1, 10, 7) - 1
    assert lib.gs_chamfer_backward_det(*args) == -2
    assert b"gs_chamfer_backward_det" in lib.gs_last_error()


def test_metrics_front_error_contracts():
    pts = torch.rand(2, 10, 3)
    pc = gs.Pointclouds(pts)
    cnt = torch.full((2,), 10, dtype=torch.int32)
    for call in (lambda: gs.metrics.chamfer_distance(pc, pc), lambda: gs.metrics.nearest_neighbor(pc, pc),
                 lambda: gs.metrics.reconstruction_metrics(pc, pc, 0.1), lambda: ops.chamfer_raw(pts, pts, cnt, cnt),
                 lambda: ops.chamfer(pts, pts, cnt, cnt)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="Expected x to be of type gradslam.Pointclouds"):
        gs.metrics.chamfer_distance(pts, pc)
    with pytest.raises(TypeError, match="Expected y to be of type gradslam.Pointclouds"):
        gs.metrics.nearest_neighbor(pc, pts)
    with pytest.raises(TypeError, match="Expected gt to be of type gradslam.Pointclouds"):
        gs.metrics.reconstruction_metrics(pc, None, 0.1)
    with pytest.raises(ValueError, match="same batch size"):
        gs.metrics.chamfer_distance(pc, gs.Pointclouds(pts[:1]))
    with pytest.raises(ValueError, match="point_reduction"):
        gs.metrics.chamfer_distance(pc, pc, point_reduction="max")
    with pytest.raises(ValueError, match="batch_reduction"):
        gs.metrics.chamfer_distance(pc, pc, batch_reduction="median")
    T = torch.eye(4).repeat(2, 5, 1, 1)
    with pytest.raises(ValueError, match="align"):
        gs.metrics.absolute_trajectory_error(T, T, align="scale")
    with pytest.raises(ValueError, match="same shape"):
        gs.metrics.absolute_trajectory_error(T, T[:, :4])
    with pytest.raises(ValueError, match="delta"):
        gs.metrics.relative_pose_error(T, T, delta=5)


# ------------------------------------------------------------------ CPU: trajectory metrics
def _rot(rng, scale=1.0):
    w = rng.randn(3) * scale
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _traj(seed, B, L, scale=0.3):
    rng = np.random.RandomState(seed)
    T = np.tile(np.eye(4), (B, L, 1, 1))
    for b in range(B):
        cur = np.eye(4)
        for s in range(L):
            step = np.eye(4)
            step[:3, :3] = _rot(rng, scale)
            step[:3, 3] = rng.randn(3) * scale
            cur = cur @ step
            T[b, s] = cur
    return torch.from_numpy(T)


def test_ate_known_answers():
    gt = _traj(0, 2, 8)
    m = gs.metrics
    for align in ("none", "first", "rigid"):
        assert float(m.absolute_trajectory_error(gt, gt, align=align).abs().max()) <= 1e-6
    G = torch.eye(4, dtype=torch.float64)
    G[:3, :3] = torch.from_numpy(_rot(np.random.RandomState(1)))
    G[:3, 3] = torch.tensor([0.3, -1.2, 0.7], dtype=torch.float64)
    moved = G @ gt  # the whole trajectory under one rigid motion
    assert float(m.absolute_trajectory_error(moved, gt, align="rigid").abs().max()) <= 1e-6
    assert float(m.absolute_trajectory_error(moved, gt, align="first").abs().max()) <= 1e-6
    assert float(m.absolute_trajectory_error(moved, gt, align="none").min()) > 0.1
    off = torch.tensor([0.3, -0.4, 1.2], dtype=torch.float64)
    shifted = gt.clone()
    shifted[..., :3, 3] += off
    err = m.absolute_trajectory_error(shifted, gt, align="none")
    assert float((err - off.norm()).abs().max()) <= 1e-6
    assert err.shape == (2,)


def test_rpe_matches_a_numpy_restatement():
    est, gt = _traj(2, 2, 8), _traj(3, 2, 8)
    for delta in (1, 3):
        tr, ro = gs.metrics.relative_pose_error(est, gt, delta=delta)
        E, G = est.numpy(), gt.numpy()
        for b in range(2):
            te, ae = [], []
            for i in range(8 - delta):
                re = np.linalg.inv(E[b, i]) @ E[b, i + delta]
                rg = np.linalg.inv(G[b, i]) @ G[b, i + delta]
                err = np.linalg.inv(rg) @ re
                te.append(np.linalg.norm(err[:3, 3]))
                ae.append(np.arccos(np.clip((np.trace(err[:3, :3]) - 1) / 2, -1, 1)))
            assert abs(float(tr[b]) - np.sqrt(np.mean(np.square(te)))) <= 1e-9
            assert abs(float(ro[b]) - np.sqrt(np.mean(np.square(ae)))) <= 1e-9
    tr, ro = gs.metrics.relative_pose_error(gt, gt)
    assert float(tr.abs().max()) <= 1e-9 and float(ro.abs().max()) <= 1e-7 and torch.isfinite(ro).all()


def test_trajectory_metrics_gradcheck():
    gt = _traj(4, 1, 5)
    est = _traj(5, 1, 5).requires_grad_(True)
    m = gs.metrics
    for align in ("none", "first", "rigid"):
        assert torch.autograd.gradcheck(lambda e: m.absolute_trajectory_error(e, gt, align=align), (est,))
    assert torch.autograd.gradcheck(lambda e: m.relative_pose_error(e, gt, delta=1), (est,))
    assert torch.autograd.gradcheck(lambda e: m.relative_pose_error(e, gt, delta=2), (est,))


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    nv.lib()
    return DEV


def _padded(clouds, dev, fill=float("nan")):
    """list of (n_b, 3) CPU tensors -> ((B, max(N, 1), 3) padded with `fill`, (B,) int32 counts) on the device"""
    N = max(max(c.shape[0] for c in clouds), 1)
    out = torch.full((len(clouds), N, 3), fill, dtype=torch.float32)
    for b, c in enumerate(clouds):
        out[b, : c.shape[0]] = c
    return out.to(dev), torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32).to(dev)


def _chamfer(As, Bs, dev, reorder, tau2=float("inf")):
    """gs_chamfer on NaN-padded clouds into sentinel-filled key buffers"""
    a, ca = _padded(As, dev)
    b, cb = _padded(Bs, dev)
    keys = tuple(torch.full(x.shape[:2], SENTINEL, dtype=torch.int64, device=dev) for x in (a, b))
    stats, kab, kba = ops.chamfer_raw(a, b, ca, cb, tau2, reorder, out=keys)
    return a, b, ca, cb, stats, kab, kba


def _brute(src, tgt, dev):
    if src.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    if tgt.shape[0] == 0:
        return torch.full((src.shape[0],), KEY_NONE, dtype=torch.int64, device=dev)
    return ops.knn1_raw(src.to(dev), tgt.to(dev), brute_force=True)


def _check_keys(As, Bs, dev, reorder):
    _, _, _, _, _, kab, kba = _chamfer(As, Bs, dev, reorder)
    for b, (A, Bc) in enumerate(zip(As, Bs)):
        for keys, s, t in ((kab, A, Bc), (kba, Bc, A)):
            assert torch.equal(keys[b, : s.shape[0]], _brute(s, t, dev)), (b, s.shape, t.shape, reorder)
            assert bool((keys[b, s.shape[0]:] == SENTINEL).all())


def _rand(seed, n, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).rand(n, 3).astype(np.float32) * scale)


@pytest.mark.gpu
@pytest.mark.parametrize("reorder", [True, False])
@pytest.mark.parametrize("Na,Nb", [(1, 1), (63, 17), (64, 16), (65, 15), (130, 49), (327, 1000), (5000, 3000), (130, 65557)])
def test_keys_equal_brute_force_shapes(dev, Na, Nb, reorder):
    """Tile (64), chunk (16) and multi-block edges; 65 557 targets = 4 098 chunks cross the 4 096-chunk survivor-list round.
    Two batch elements, the second with the clouds swapped in size order and another seed."""
    As = [_rand(10 + Na, Na), _rand(11 + Na, min(Na, 200))]
    Bs = [_rand(20 + Nb, Nb), _rand(21 + Nb, min(Nb, 300), scale=2.0)]
    _check_keys(As, Bs, dev, reorder)


@pytest.fixture(scope="module")
def frame_cloud(dev):
    """the valid pixels of a 30x40 frame as an image-ordered cloud (CPU tensor)"""
    c, d, K, P = make_sequence(1, 1, 30, 40, seed=3)
    pc = pointclouds_from_rgbdimages(gs.RGBDImages(c.to(dev), d.to(dev), K.to(dev), P.to(dev)))
    return pc.points_padded[0].detach().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("reorder", [True, False])
@pytest.mark.parametrize("kind", ["image", "random", "shuffled", "duplicates", "identical", "plane"])
def test_keys_equal_brute_force_inputs(dev, frame_cloud, kind, reorder):
    src = _rand(40, 333, scale=2.0) + torch.tensor([-1.0, -1.0, 1.0])
    if kind == "image":
        tgt = frame_cloud
        src = frame_cloud[::3] + 0.01
    elif kind == "random":
        tgt = _rand(41, 1500, scale=2.0) + torch.tensor([-1.0, -1.0, 1.0])
    elif kind == "shuffled":
        tgt = frame_cloud[torch.from_numpy(np.random.RandomState(42).permutation(frame_cloud.shape[0]))]
        src = frame_cloud[::3] + 0.01
    elif kind == "duplicates":  # every target row exists three times: the lowest original row must win
        base = _rand(43, 400, scale=2.0) + torch.tensor([-1.0, -1.0, 1.0])
        tgt = torch.cat([base, base, base])[torch.from_numpy(np.random.RandomState(44).permutation(1200))]
    elif kind == "identical":
        tgt = torch.tensor([[0.25, -0.5, 1.5]]).repeat(100, 1)
    else:  # plane z = const: one axis without extent
        tgt = _rand(45, 900, scale=2.0)
        tgt[:, 2] = 1.25
    _check_keys([src, tgt], [tgt, src[:50]], dev, reorder)
    if kind in ("duplicates", "identical"):
        _, _, _, _, _, kab, _ = _chamfer([src], [tgt], dev, reorder)
        idx = (kab[0] & 0xFFFFFFFF).cpu()
        rows, first = tgt.numpy(), {}
        for j in range(rows.shape[0]):
            first.setdefault(rows[j].tobytes(), j)
        assert all(first[rows[int(j)].tobytes()] == int(j) for j in idx)


def _unpack(keys):
    k = keys.cpu().numpy().astype(np.int64)
    return (k >> 32).astype(np.uint32).view(np.float32), (k & 0xFFFFFFFF).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("reorder", [True, False])
def test_statistics_are_fp64_sums_of_the_fp32_values(dev, reorder):
    As, Bs = [_rand(50, 5000), _rand(51, 327)], [_rand(52, 3000), _rand(53, 1000)]
    tau = np.float32(0.03)
    tau2 = float(np.float32(tau * tau))
    _, _, _, _, stats, kab, kba = _chamfer(As, Bs, dev, reorder, tau2)
    stats2 = _chamfer(As, Bs, dev, reorder, tau2)[4]
    assert torch.equal(stats, stats2)
    stats = stats.cpu().numpy()
    for b in range(2):
        for d, (keys, n) in enumerate(((kab, As[b].shape[0]), (kba, Bs[b].shape[0]))):
            d2, _ = _unpack(keys[b, :n])
            ref2, ref1 = d2.astype(np.float64).sum(), np.sqrt(d2).astype(np.float64).sum()  # np.sqrt of fp32: correctly rounded
            assert np.sqrt(d2).dtype == np.float32
            bound = n * 2.0 ** -52
            print("stats b=%d d=%d rel err %.3e %.3e (bound %.3e)" % (b, d, abs(stats[b, d, 0] - ref2) / ref2,
                                                                     abs(stats[b, d, 1] - ref1) / ref1, bound))
            assert abs(stats[b, d, 0] - ref2) <= bound * ref2
            assert abs(stats[b, d, 1] - ref1) <= bound * ref1
            assert stats[b, d, 2] == float((d2 < np.float32(tau2)).sum())
            assert 0 < stats[b, d, 2] < n  # the threshold splits the points
            assert stats[b, d, 3] == float(d2.max())


@pytest.mark.gpu
def test_threshold_is_strict(dev):
    """d2 = 0.25 = tau2 exactly is NOT within the threshold (dist2 < dist_thresh, as in the ICP); the next threshold up is."""
    src, tgt = torch.zeros(1, 3), torch.tensor([[0.5, 0.0, 0.0], [2.0, 0.0, 0.0]])
    pc_s, pc_t = gs.Pointclouds(src.unsqueeze(0).to(dev)), gs.Pointclouds(tgt.unsqueeze(0).to(dev))
    at = gs.metrics.reconstruction_metrics(pc_s, pc_t, 0.5)
    above = gs.metrics.reconstruction_metrics(pc_s, pc_t, 0.5000001)
    assert float(at["precision"][0]) == 0.0 and float(above["precision"][0]) == 1.0
    assert float(at["accuracy"][0]) == 0.5 and float(at["hausdorff"][0]) == 2.0
    assert float(at["recall"][0]) == 0.0 and float(at["fscore"][0]) == 0.0
    t5 = np.float32(0.5)
    stats = ops.chamfer_raw(pc_s.points_padded, pc_t.points_padded, pc_s._counts_i32(), pc_t._counts_i32(), float(t5 * t5))[0]
    assert stats[0, 0].tolist() == [0.25, 0.5, 0.0, 0.25]


def _ref_grads(a, b, ca, cb, kab, kba, g2, g1):
    """float64 restatement of the reverse pass, gathered by the kernel's own indices.  Per cloud: the direct rows, the
    scattered rows, the sum of |contribution| per component of the scattered rows and the number of contributions per row."""
    A, Bm = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    na, nb = ca.cpu().numpy(), cb.cpu().numpy()
    G2, G1 = g2.cpu().numpy().astype(np.float64), g1.cpu().numpy().astype(np.float64)
    out = {}
    for d, (S, T, ns, nt, keys) in enumerate(((A, Bm, na, nb, kab), (Bm, A, nb, na, kba))):
        direct, scat, mass = np.zeros_like(S), np.zeros_like(T), np.zeros_like(T)
        k = np.zeros(T.shape[:2], dtype=np.int64)
        for bi in range(S.shape[0]):
            if ns[bi] == 0 or nt[bi] == 0:
                continue
            _, idx = _unpack(keys[bi, : ns[bi]])
            delta = S[bi, : ns[bi]] - T[bi, idx]
            dist = np.sqrt((delta ** 2).sum(-1))
            c = 2 * G2[bi, d] + np.where(dist > 0, G1[bi, d] / np.where(dist > 0, dist, 1.0), 0.0)
            v = c[:, None] * delta
            direct[bi, : ns[bi]] = v
            np.add.at(scat[bi], idx, -v)
            np.add.at(mass[bi], idx, np.abs(v))
            np.add.at(k[bi], idx, 1)
        out[d] = (direct, scat, mass, k)
    return out


def _backward(a, b, ca, cb, kab, kba, g2, g1, dev, det=False):
    """the reverse call into NaN-filled buffers: what comes back below the counts was written by the call"""
    out = (torch.full_like(a, float("nan")), torch.full_like(b, float("nan")))
    old = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det)
    try:
        return ops.chamfer_backward_raw(a, b, ca, cb, kab, kba, g2, g1, out=out)
    finally:
        torch.use_deterministic_algorithms(old)


def _valid(x, counts):
    """(B, N, 3) -> float64 numpy with the rows at or beyond the counts set to 0; asserts those rows are still NaN"""
    x = x.cpu().numpy().astype(np.float64)
    for b, n in enumerate(counts.cpu().tolist()):
        assert np.isnan(x[b, n:]).all(), "rows beyond the count were written"
        x[b, n:] = 0.0
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("det", [False, True])
def test_gradients_against_a_float64_restatement(dev, det):
    """Direction by direction (the other direction's adjoints zero), so that one cloud's adjoint is the direct part alone and
    the other's the scattered part alone.  Direct: < 10 fp32 roundings (difference, d2, square root, division, add, two
    products) -> 16 U |reference| per component.  Scattered row of k contributions: 16 U per term plus k U for the sum."""
    As, Bs = [_rand(60, 327, 2.0), _rand(61, 130, 2.0)], [_rand(62, 1000, 2.0), _rand(63, 49, 2.0)]
    As[0][5] = Bs[0][17]  # a source lying exactly on its target: d = 0
    a, b, ca, cb, _, kab, kba = _chamfer(As, Bs, dev, True)
    rng = np.random.RandomState(64)
    for d in (0, 1):
        g2 = torch.zeros(2, 2)
        g1 = torch.zeros(2, 2)
        g2[:, d] = torch.from_numpy(rng.rand(2).astype(np.float32))
        g1[:, d] = torch.from_numpy(rng.rand(2).astype(np.float32))
        g2, g1 = g2.to(dev), g1.to(dev)
        g_a, g_b = _backward(a, b, ca, cb, kab, kba, g2, g1, dev, det)
        direct, scat, mass, k = _ref_grads(a, b, ca, cb, kab, kba, g2, g1)[d]
        got_src, got_tgt = (_valid(g_a, ca), _valid(g_b, cb)) if d == 0 else (_valid(g_b, cb), _valid(g_a, ca))
        assert np.isfinite(got_src).all() and np.isfinite(got_tgt).all()
        err_d = np.abs(got_src - direct)
        print("det=%s d=%d direct max err/|ref| %.2f U, scattered max err/mass %.2f U" % (
            det, d, (err_d / np.maximum(np.abs(direct), 1e-300)).max() / U, (np.abs(got_tgt - scat) / np.maximum(mass, 1e-300)).max() / U))
        assert (err_d <= 16 * U * np.abs(direct)).all()
        assert (np.abs(got_tgt - scat) <= (16 + k[..., None]) * U * mass).all()
        assert np.abs(direct).max() > 0.1 and k.max() >= 2
    g_a = _backward(a, b, ca, cb, kab, kba, torch.ones(2, 2, device=dev), torch.ones(2, 2, device=dev), dev, det)[0]
    assert float(kab[0, 5] >> 32) == 0.0 and int(kab[0, 5] & 0xFFFFFFFF) == 17
    assert np.isfinite(_valid(g_a, ca)[0, 5]).all()
    only_a = _backward(a, b, ca, cb, kab, kba, torch.tensor([[1.0, 0.0]] * 2, device=dev), torch.tensor([[1.0, 0.0]] * 2, device=dev), dev, det)[0]
    assert (_valid(only_a, ca)[0, 5] == 0.0).all()  # d = 0: c delta = 0, no g1 / d


@pytest.mark.gpu
def test_many_to_one_scatter_is_reproducible_when_asked(dev):
    """4096 sources onto 8 targets.  With torch's deterministic flag the reverse pass gives the same bits twice; it agrees
    with the default (float atomics) within the bound of the scattered rows, here with the rows' own direct part as one
    more contribution: (16 + k + 1) U sum |contribution|."""
    As, Bs = [_rand(70, 4096, 2.0)], [_rand(71, 8, 2.0)]
    a, b, ca, cb, _, kab, kba = _chamfer(As, Bs, dev, True)
    rng = np.random.RandomState(72)
    g2, g1 = (torch.from_numpy(rng.rand(1, 2).astype(np.float32)).to(dev) for _ in range(2))
    ref = _ref_grads(a, b, ca, cb, kab, kba, g2, g1)
    want_b = ref[1][0] + ref[0][1]  # b: direct part of b -> a plus scattered part of a -> b
    mass_b = np.abs(ref[1][0]) + ref[0][2]
    k_b = ref[0][3][..., None] + 1
    want_a, mass_a, k_a = ref[0][0] + ref[1][1], np.abs(ref[0][0]) + ref[1][2], ref[1][3][..., None] + 1
    assert k_b.sum() == 4096 + 8 and k_b.min() > 100
    old = torch.are_deterministic_algorithms_enabled()
    try:
        det1 = _backward(a, b, ca, cb, kab, kba, g2, g1, dev, det=True)
        det2 = _backward(a, b, ca, cb, kab, kba, g2, g1, dev, det=True)
        assert torch.are_deterministic_algorithms_enabled() == old
    finally:
        torch.use_deterministic_algorithms(old)
    dflt = _backward(a, b, ca, cb, kab, kba, g2, g1, dev, det=False)
    for x, y in zip(det1, det2):
        assert torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0))  # (NaN = the untouched rows)
    for got in (det1, dflt):
        ga, gb = _valid(got[0], ca), _valid(got[1], cb)
        print("many-to-one: b err/mass %.2f U (k = %d)" % ((np.abs(gb - want_b) / mass_b).max() / U, k_b.max()))
        assert (np.abs(gb - want_b) <= (16 + k_b) * U * mass_b).all()
        assert (np.abs(ga - want_a) <= (16 + k_a) * U * mass_a).all()


@pytest.mark.gpu
@pytest.mark.parametrize("reorder", [True, False])
def test_ragged_batch_and_empty_sides(dev, reorder):
    """B = 3, counts (130, 0, 65) against (49, 20, 0): padding is NaN and never read, the elements with an empty side give
    zero statistics, KEY_NONE keys and zero gradients, and nothing at or beyond a count is written."""
    As = [_rand(80, 130), torch.zeros(0, 3), _rand(81, 65)]
    Bs = [_rand(82, 49), _rand(83, 20), torch.zeros(0, 3)]
    a, b, ca, cb, stats, kab, kba = _chamfer(As, Bs, dev, reorder)
    assert a.shape == (3, 130, 3) and b.shape == (3, 49, 3)
    assert torch.isfinite(stats).all() and bool((stats[1:] == 0).all()) and float(stats[0, :, 0].min()) > 0
    for keys, cl in ((kab, As), (kba, Bs)):
        for bi, c in enumerate(cl):
            n = c.shape[0]
            assert bool((keys[bi, n:] == SENTINEL).all())
            if bi > 0:
                assert bool((keys[bi, :n] == KEY_NONE).all())
    assert torch.equal(kab[0], _brute(As[0], Bs[0], dev)) and torch.equal(kba[0], _brute(Bs[0], As[0], dev))
    # the public unpacking: -1 beyond the count and for an empty other side
    pa, pb = gs.Pointclouds([x.to(dev) for x in As]), gs.Pointclouds([x.to(dev) for x in Bs])
    d2, idx = gs.metrics.nearest_neighbor(pa, pb, reorder=reorder)
    assert d2.shape == (3, 130) and idx.dtype == torch.int64
    assert torch.equal(idx[0], kab[0] & 0xFFFFFFFF) and bool((idx[1:] == -1).all()) and bool((d2[1:] == 0).all())
    cd = gs.metrics.chamfer_distance(pa, pb, batch_reduction=None, reorder=reorder)
    assert cd.shape == (3,) and float(cd[1]) == 0.0 and float(cd[2]) == 0.0 and float(cd[0]) > 0
    g = torch.ones(3, 2, device=dev)
    for det in (False, True):
        g_a, g_b = _backward(a, b, ca, cb, kab, kba, g, g, dev, det)
        va, vb = _valid(g_a, ca), _valid(g_b, cb)  # (asserts the rows beyond the counts are untouched)
        assert (va[1:] == 0).all() and (vb[1:] == 0).all()
        assert np.isfinite(va).all() and np.abs(va[0]).max() > 0 and np.abs(vb[0]).max() > 0


# ------------------------------------------------------------------ GPU: the public layer
@pytest.mark.gpu
def test_chamfer_distance_public_layer(dev):
    x, y = _rand(90, 700, 2.0), _rand(91, 450, 2.0)
    x2, y2 = _rand(92, 300, 2.0), _rand(93, 450, 2.0)
    pc = gs.Pointclouds(x.unsqueeze(0).to(dev))
    assert float(gs.metrics.chamfer_distance(pc, pc)) == 0.0
    d2, idx = gs.metrics.nearest_neighbor(pc, pc)
    assert torch.equal(idx[0], torch.arange(700, device=dev)) and bool((d2 == 0).all())
    px, py = gs.Pointclouds([x.to(dev), x2.to(dev)]), gs.Pointclouds([y.to(dev), y2.to(dev)])
    dxy, _ = gs.metrics.nearest_neighbor(px, py)
    dyx, _ = gs.metrics.nearest_neighbor(py, px)
    nx, ny = torch.tensor([700.0, 300.0], dtype=torch.float64, device=dev), torch.tensor([450.0, 450.0], dtype=torch.float64, device=dev)
    sxy, syx = dxy.double().sum(1), dyx.double().sum(1)  # padding holds 0
    want = (sxy / nx + syx / ny).mean()
    rel = lambda got, ref: abs(float(got) - float(ref)) / abs(float(ref))
    # fp64 sums rounded to fp32 once, then an fp32 division, an add and the batch mean: 8 U is generous
    assert rel(gs.metrics.chamfer_distance(px, py), want) <= 8 * U
    for reorder in (True, False):
        per_b = gs.metrics.chamfer_distance(px, py, batch_reduction=None, reorder=reorder)
        assert per_b.shape == (2,) and rel(per_b[1], sxy[1] / nx[1] + syx[1] / ny[1]) <= 8 * U
    assert torch.equal(gs.metrics.chamfer_distance(px, py, batch_reduction=None, reorder=True),
                       gs.metrics.chamfer_distance(px, py, batch_reduction=None, reorder=False))
    one = gs.metrics.chamfer_distance(px, py, single_directional=True, point_reduction="sum", batch_reduction="sum")
    assert rel(one, sxy.sum()) <= 8 * U
    unsq = gs.metrics.chamfer_distance(px, py, squared=False, point_reduction="sum", batch_reduction=None)
    assert rel(unsq[0], dxy[0].double().sqrt().sum() + dyx[0].double().sqrt().sum()) <= 8 * U
    stats = ops.chamfer_raw(px.points_padded, py.points_padded, px._counts_i32(), py._counts_i32())[0]
    assert torch.equal(unsq, (stats[..., 1].float()).sum(1))


@pytest.mark.gpu
def test_reconstruction_metrics_of_a_shifted_cloud(dev):
    """x coordinates are multiples of 2^-30 below 0.0056, so x + float32(0.01) -- a multiple of 2^-30 below 2^-6 -- is exact, the twin of every point lies at
    exactly float32(0.01) (sqrt(fl(t * t)) = t under correct rounding) and any nearer neighbour only lowers the means."""
    x = _rand(95, 2000, 2.0)
    x[:, 0] = torch.from_numpy(np.random.RandomState(96).randint(0, 6000000, 2000).astype(np.float32) * np.float32(2.0 ** -30))
    shifted = x + torch.tensor([0.01, 0.0, 0.0])
    assert bool(((shifted[:, 0].double() - x[:, 0].double()) == float(np.float32(0.01))).all())
    pred, gt = gs.Pointclouds(shifted.unsqueeze(0).to(dev)), gs.Pointclouds(x.unsqueeze(0).to(dev))
    m = gs.metrics.reconstruction_metrics(pred, gt, 0.02)
    assert sorted(m) == ["accuracy", "chamfer", "completeness", "fscore", "hausdorff", "precision", "recall"]
    assert all(v.shape == (1,) and not v.requires_grad for v in m.values())
    assert float(m["precision"]) == 1.0 and float(m["recall"]) == 1.0 and float(m["fscore"]) == 1.0
    lim = float(np.nextafter(np.float32(0.01), np.float32(1.0)))  # 0.01 (+1 ulp)
    assert 0 < float(m["accuracy"]) <= lim and 0 < float(m["completeness"]) <= lim and float(m["hausdorff"]) <= lim
    assert float(m["chamfer"]) <= 2 * lim * lim


@pytest.mark.gpu
def test_chamfer_gradient_reaches_the_depth_image(dev):
    c, d, K, P = make_sequence(1, 2, 48, 64, seed=5)
    depth = d[:, :1].to(dev).clone().requires_grad_(True)
    frame = gs.RGBDImages(c[:, :1].to(dev), depth, K.to(dev), P[:, :1].to(dev))
    with torch.no_grad():
        fixed = pointclouds_from_rgbdimages(gs.RGBDImages(c[:, 1:].to(dev), d[:, 1:].to(dev), K.to(dev), P[:, 1:].to(dev)))
    loss = gs.metrics.chamfer_distance(pointclouds_from_rgbdimages(frame), fixed)
    assert loss.ndim == 0 and float(loss) > 0
    loss.backward()
    g = depth.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert bool((g[depth.detach() == 0] == 0).all()) and int((depth.detach() == 0).sum()) > 0
