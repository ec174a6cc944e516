"""The deterministic folds (gs_detfold.hpp: ICP linearisation, ICP loop, chamfer) against their own contribution rows.

Under torch.use_deterministic_algorithms(True) the reverse passes store one row of eight 32-bit words per (launch, source) --
d_bar (3) | n_bar (3) | j (int, -1 = none) | pad -- and det_fold_run folds the rows into the targets by the rule of
gs_fixed128.hpp.  The rows are the fold's complete input and are still in the cached workspace after the call, so the reference
needs no restatement of any kernel's fp32 arithmetic: it is tests/helpers.fold_rule_f32 over the rows read back, with the
maximum over all float words of all rows with j >= 0 of the fold.  Every comparison is bitwise.  Where the rows sit comes from
the public size queries; a moved layout fails an offset / shape / content assertion."""
import numpy as np
import pytest
import torch

from tests.helpers import fold_rule_f32

DEV = "cuda:0"
ROW = 8  # words per contribution row


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


@pytest.fixture
def det_flag():
    """flag(on) switches torch.use_deterministic_algorithms; the state found on entry is restored whatever the test did."""
    old = torch.are_deterministic_algorithms_enabled()
    try:
        yield torch.use_deterministic_algorithms
    finally:
        torch.use_deterministic_algorithms(old)


def lg_of(n):
    return int(n - 1).bit_length()


def align256(n):
    return -(-n // 256) * 256


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """Bitwise, NaN comparing as NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


STALE = np.concatenate([np.full(6, 1e30, np.float32).view(np.int32), np.array([0, 0], np.int32)])  # six 1e30, j = 0, pad 0


def prepare_ws(gs, nbytes, tag, fill):
    """The cached workspace of `tag`, grown to what the call will ask for and filled: "stale" (every 8-word row reads as a
    contribution of 1e30 to target 0) or "zero"."""
    ws = gs._native.workspace(nbytes, DEV, tag)
    assert ws.numel() >= nbytes and ws.numel() % 32 == 0
    if fill == "stale":
        ws.view(torch.int32).view(-1, ROW).copy_(torch.from_numpy(STALE).to(DEV))
    else:
        ws.zero_()
    torch.cuda.synchronize()
    return ws


def read_rows(gs, ws, tag, offset, shape):
    """The rows at byte `offset` of the cached workspace (the tensor the call used) -> int32 numpy of shape + (8,)."""
    again = gs._native.workspace(1, DEV, tag)
    assert again.data_ptr() == ws.data_ptr() and offset % 256 == 0
    n = int(np.prod(shape)) * ROW * 4
    assert offset + n <= ws.numel()
    torch.cuda.synchronize()
    return ws[offset:offset + n].view(torch.int32).view(*shape, ROW).cpu().numpy()


def fold_of_rows(rows, nt, lg):
    """rows (..., 8) int32 of ONE fold -> (nt, 6) float32 by the rule: the maximum over the six float words of every row with
    j >= 0, target t the rule over the rows with j == t; targets without a row are +0.0."""
    rows = rows.reshape(-1, ROW)
    j = rows[:, 6]
    words = np.ascontiguousarray(rows[:, :6]).view(np.float32)
    call_terms = words[j >= 0]
    assert call_terms.size <= 100000
    out = np.zeros((nt, 6), np.float32)
    for t in range(nt):
        mine = words[j == t]
        for c in range(6):
            out[t, c] = fold_rule_f32(mine[:, c], lg, call_terms)
    return out


def assert_rows_are_fresh(rows, nt, need_some=True):
    """Every row holds j == -1 or 0 <= j < nt, with finite words where it contributes (no row still reads 1e30)."""
    j = rows[..., 6]
    assert ((j == -1) | ((j >= 0) & (j < nt))).all(), np.unique(j)[:10]
    w = np.ascontiguousarray(rows[..., :6]).view(np.float32)[j >= 0]
    assert np.isfinite(w).all() and (np.abs(w) < 1e29).all()
    assert (rows[..., 7][j >= 0] == 0).all()
    assert not need_some or (j >= 0).any()


def surface(n, seed, side=None):
    """n points (random, or a side x side grid) on z = f(x, y) over [0, 1]^2 with their unit normals."""
    g = torch.Generator().manual_seed(seed)
    if side is None:
        xy = torch.rand(n, 2, generator=g, dtype=torch.float64)
    else:
        u = (torch.arange(side, dtype=torch.float64) + 0.5) / side
        xy = torch.stack(torch.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    z = 0.05 * torch.sin(3 * x) + 0.03 * torch.cos(4 * y) + 0.02 * x * y
    zx = 0.15 * torch.cos(3 * x) + 0.02 * y
    zy = -0.12 * torch.sin(4 * y) + 0.02 * x
    nrm = torch.stack([-zx, -zy, torch.ones_like(z)], -1)
    return torch.stack([x, y, z], -1).float(), (nrm / nrm.norm(dim=-1, keepdim=True)).float()


# ------------------------------------------------------------------ the linearisation's fold
def _linearize(gs, src, tgt, nrm, best, ups, fill=None):
    """ops.icp_linearize forward + backward with the upstream adjoints `ups` -> (g_src, g_tgt, g_nrm) numpy, rows or None."""
    ns, nt = src.shape[0], tgt.shape[0]
    det = torch.are_deterministic_algorithms_enabled()
    ws = None
    if det:
        nbytes = gs._native.ws_bytes("gs_icp_linearize_backward_det_ws_bytes", ns, nt)
        assert nbytes >= align256(ns * ROW * 4)
        ws = prepare_ws(gs, nbytes, "linearize_bwd_det", fill or "zero")
    s, tg, n = (x.to(DEV).clone().requires_grad_(True) for x in (src, tgt, nrm))
    torch.autograd.backward(list(gs.ops.icp_linearize(s, tg, n, best, None)), [u.to(DEV) for u in ups])
    torch.cuda.synchronize()
    rows = read_rows(gs, ws, "linearize_bwd_det", 0, (ns,)) if det else None
    return [x.grad.cpu().numpy() for x in (s, tg, n)], rows


@pytest.mark.gpu
def test_linearize_outputs_are_the_fold_of_the_rows(gs, det_flag):
    """1500 sources on 40 targets.  (1) g_tgt / g_nrm are the rule over the rows read back; (2) a workspace whose every row
    read as a stale contribution gives the same bits as a zeroed one; (3) on duplicated targets (one source each) the outputs
    are the rows themselves -- so the rows are the contributions -- and the original outputs are the rule over those; the
    flag-off path on the duplicated inputs (one float atomic onto zero) gives the same bits."""
    ns, nt = 1500, 40
    g = torch.Generator().manual_seed(21)
    src, _ = surface(ns, 1)
    src = src + 0.01 * torch.randn(ns, 3, generator=g)
    tgt, nrm = surface(nt, 2)
    tgt[35:, 2] += 5.0  # five targets far from every source
    ups = [torch.randn(6, 6, generator=g), torch.randn(6, 1, generator=g), torch.randn((), generator=g)]
    best = gs.ops.knn1_raw(src.to(DEV), tgt.to(DEV))
    j = (best & 0xFFFFFFFF).cpu().numpy()
    assert (np.bincount(j, minlength=nt) > 1).any() and (np.bincount(j, minlength=nt) == 0).any()  # shared and empty targets
    lg = lg_of(ns)

    det_flag(True)
    (g_src, g_tgt, g_nrm), rows = _linearize(gs, src, tgt, nrm, best, ups, "stale")
    assert_rows_are_fresh(rows, nt)
    assert np.array_equal(rows[:, 6][rows[:, 6] >= 0], j[rows[:, 6] >= 0]) and (rows[:, 6] >= 0).sum() > ns // 2
    want = fold_of_rows(rows, nt, lg)
    assert same_bits(g_tgt, want[:, :3]) and same_bits(g_nrm, want[:, 3:])
    empty = np.bincount(j, minlength=nt) == 0
    assert not bits(g_tgt[empty]).any() and not bits(g_nrm[empty]).any() and g_tgt[~empty].any(axis=1).all()
    (z_src, z_tgt, z_nrm), z_rows = _linearize(gs, src, tgt, nrm, best, ups, "zero")
    assert same_bits(g_tgt, z_tgt) and same_bits(g_nrm, z_nrm) and same_bits(g_src, z_src)
    assert np.array_equal(rows[:, :7][rows[:, 6] >= 0], z_rows[:, :7][z_rows[:, 6] >= 0])

    # duplicated targets: source i alone on target i
    jt = torch.from_numpy(j).long()
    best2 = (best & ~0xFFFFFFFF) | torch.arange(ns, device=DEV)
    (d_src, d_tgt, d_nrm), d_rows = _linearize(gs, src, tgt[jt], nrm[jt], best2, ups, "stale")
    words = np.ascontiguousarray(rows[:, :6]).view(np.float32)
    valid = rows[:, 6] >= 0
    assert np.array_equal(d_rows[:, 6][valid], np.arange(ns)[valid]) and np.array_equal(d_rows[valid, :6], rows[valid, :6])
    dup = np.concatenate([d_tgt, d_nrm], axis=1)
    single = np.array([[fold_rule_f32(words[i, c:c + 1], lg, words[valid]) if valid[i] else 0.0 for c in range(6)] for i in range(ns)], np.float32)
    assert same_bits(dup, single)
    plain = (bits(single) == bits(words)) | ~valid[:, None] | (words == 0)  # (a fold of one term is that term, -0 -> +0 ...
    assert plain.mean() > 0.999, plain.mean()                            # ... unless it lies 102 - lg places below the maximum)
    refold = np.array([[fold_rule_f32(dup[j == t, c][valid[j == t]], lg, dup[valid]) for c in range(6)] for t in range(nt)], np.float32)
    assert same_bits(np.concatenate([g_tgt, g_nrm], axis=1), refold)
    det_flag(False)
    (a_src, a_tgt, a_nrm), _ = _linearize(gs, src, tgt[jt], nrm[jt], best2, ups)
    assert same_bits(a_tgt, d_tgt) and same_bits(a_nrm, d_nrm) and same_bits(a_src, d_src)


# ------------------------------------------------------------------ the ICP loop's fold
GRAD_PARAMS = (2.0, 1.0, 1.0, 200.0)  # lambda_max, B, B2, nu


def _loop_scene(ns=2000, nt_side=8):
    src, _ = surface(ns, 3)
    src = src + 0.004 * torch.randn(ns, 3, generator=torch.Generator().manual_seed(4))
    tgt, nrm = surface(0, 0, side=nt_side)
    return src, tgt, nrm


def _pose(angle, shift):
    T = torch.eye(4)
    c, s = float(np.cos(angle)), float(np.sin(angle))
    T[:3, :3] = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = torch.tensor([shift, -0.5 * shift, 0.7 * shift])
    return T


def _loop(gs, src, tgt, nrm, T0, numiters, damp, grad_lm, grad_T, need_tgt=True, fill="zero"):
    """ops.icp_loop_autograd forward + backward under the flag -> ((g_src, g_tgt or None, g_nrm, g_T0) numpy, rows (Q, ns, 8))."""
    ns, nt = src.shape[0], tgt.shape[0]
    Q = 2 * numiters if grad_lm else numiters
    nv = gs._native
    nbytes = nv.ws_bytes("gs_icp_backward_det_ws_bytes", ns, nt, numiters, int(grad_lm))
    off = nv.ws_bytes("gs_icp_backward_ws_bytes", ns)
    assert off % 256 == 0 and nbytes >= off + align256(Q * ns * ROW * 4)
    ws = prepare_ws(gs, nbytes, "icp_bwd_det", fill)
    s, tg, n, T = (x.to(DEV).clone().requires_grad_(r) for x, r in ((src, True), (tgt, need_tgt), (nrm, True), (T0, True)))
    out, _ = gs.ops.icp_loop_autograd(s, tg, n, T, numiters, damp, None, GRAD_PARAMS if grad_lm else None)
    out.backward(grad_T.to(DEV))
    torch.cuda.synchronize()
    rows = read_rows(gs, ws, "icp_bwd_det", off, (Q, ns))
    return [None if x.grad is None else x.grad.cpu().numpy() for x in (s, tg, n, T)], rows


def _check_loop_fold(grads, rows, nt):
    Q, ns = rows.shape[:2]
    want = fold_of_rows(rows, nt, lg_of(Q * ns))
    if grads[1] is not None:
        assert same_bits(grads[1], want[:, :3])
    assert same_bits(grads[2], want[:, 3:])
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("grad_lm", [False, True], ids=["icp", "gradicp"])
def test_loop_outputs_are_the_fold_of_all_launches_rows(gs, det_flag, grad_lm):
    """2000 sources, 64 targets, 3 iterations: Q = 3 (LM) or 6 (gradLM) slabs of rows, lg = ceil(log2(Q ns)).  With both
    tgt and nrm wanted and with nrm alone (the rows are stored all the same); from a stale workspace and from a zeroed one."""
    src, tgt, nrm = _loop_scene()
    nt, numiters = tgt.shape[0], 3
    T0 = _pose(0.02, 0.004)
    W = torch.randn(4, 4, generator=torch.Generator().manual_seed(8))
    det_flag(True)
    grads, rows = _loop(gs, src, tgt, nrm, T0, numiters, 1e-8, grad_lm, W, fill="stale")
    assert rows.shape == ((6 if grad_lm else 3), 2000, ROW)
    assert_rows_are_fresh(rows, nt)
    assert all((rows[q, :, 6] >= 0).any() for q in range(rows.shape[0])) or not grad_lm
    want = _check_loop_fold(grads, rows, nt)
    per_target = np.bincount(rows[..., 6][rows[..., 6] >= 0], minlength=nt)
    assert per_target.max() > rows.shape[0] and np.isfinite(want).all() and np.abs(want[per_target > 0]).max() > 0
    assert not bits(want[per_target == 0]).any()
    z_grads, z_rows = _loop(gs, src, tgt, nrm, T0, numiters, 1e-8, grad_lm, W, fill="zero")
    for a, b in zip(grads, z_grads):
        assert same_bits(a, b)
    only, o_rows = _loop(gs, src, tgt, nrm, T0, numiters, 1e-8, grad_lm, W, need_tgt=False, fill="stale")
    assert only[1] is None and same_bits(only[2], grads[2]) and same_bits(only[0], grads[0]) and same_bits(only[3], grads[3])
    assert_rows_are_fresh(o_rows, nt)
    _check_loop_fold(only, o_rows, nt)


# candidates for a rejected LM iteration (new_err >= err): Gauss-Newton steps from poor poses with next to no damping overshoot
REJECT_CANDIDATES = [(3, a, sh, d) for d in (1e-8, 1e-4) for a, sh in ((0.6, 0.2), (1.2, 0.3), (0.3, 0.1), (2.0, 0.5), (0.0, 0.0))]
REJECT_CANDIDATES += [(5, a, sh, d) for _, a, sh, d in REJECT_CANDIDATES]


@pytest.mark.gpu
def test_a_rejected_iteration_leaves_a_slab_of_no_contribution_rows(gs, det_flag):
    """Plain ICP: a rejected LM iteration contributes nothing, and its slab must say so (j = -1 in every row) even when the
    workspace held stale contributions.  The configuration is the first of REJECT_CANDIDATES whose forward trace shows a
    rejected iteration together with an accepted one."""
    src, tgt, nrm = _loop_scene()
    nt, ns = tgt.shape[0], src.shape[0]
    found = None
    for numiters, angle, shift, damp in REJECT_CANDIDATES:
        T0 = _pose(angle, shift)
        _, _, trace = gs.ops.icp_device_loop(src.to(DEV), tgt.to(DEV), nrm.to(DEV), T0.to(DEV), numiters, damp, None, want_trace=True)
        accepted = trace[:, 45].cpu().numpy() != 0  # (1: the step was taken, 0: a rejected LM iteration)
        if (~accepted).any() and accepted.any():
            found = (numiters, T0, damp, accepted)
            break
    assert found is not None, "no candidate configuration rejects an iteration"
    numiters, T0, damp, accepted = found
    print("rejected iterations", np.nonzero(~accepted)[0], "of", numiters)
    W = torch.randn(4, 4, generator=torch.Generator().manual_seed(9))
    det_flag(True)
    grads, rows = _loop(gs, src, tgt, nrm, T0, numiters, damp, False, W, fill="stale")
    assert rows.shape == (numiters, ns, ROW)
    assert_rows_are_fresh(rows, nt)
    for k in range(numiters):  # reverse launch q = numiters - 1 - k walks iteration k
        slab = rows[numiters - 1 - k, :, 6]
        assert (slab >= 0).any() if accepted[k] else (slab == -1).all(), (k, accepted)
    _check_loop_fold(grads, rows, nt)
    z_grads, _ = _loop(gs, src, tgt, nrm, T0, numiters, damp, False, W, fill="zero")
    for a, b in zip(grads, z_grads):
        assert same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("grad_lm", [False, True], ids=["icp", "gradicp"])
def test_loop_fold_with_non_finite_rows(gs, det_flag, grad_lm):
    """One +inf and one NaN in the upstream grad_T: the rows carry non-finite words, and every output element is still the
    rule over its rows (the float sum's NaN / infinity; NaN compares as NaN)."""
    src, tgt, nrm = _loop_scene()
    nt = tgt.shape[0]
    W = torch.randn(4, 4, generator=torch.Generator().manual_seed(10))
    W[0, 3], W[1, 1] = float("inf"), float("nan")
    det_flag(True)
    grads, rows = _loop(gs, src, tgt, nrm, _pose(0.02, 0.004), 3, 1e-8, grad_lm, W, fill="zero")
    j = rows[..., 6]
    assert ((j == -1) | ((j >= 0) & (j < nt))).all() and (j >= 0).any()
    words = np.ascontiguousarray(rows[..., :6]).view(np.float32)[j >= 0]
    assert not np.isfinite(words).all()
    want = _check_loop_fold(grads, rows, nt)
    assert not np.isfinite(want).all()


# ------------------------------------------------------------------ the chamfer folds
def _chamfer_bwd(gs, a, b, ca, cb, kab, kba, g2, g1, fill=None, sentinel=7.0):
    """ops.chamfer_backward_raw into sentinel-filled outputs -> (g_a, g_b numpy, rows of direction 0 (B, Na, 8), of 1 (B, Nb, 8))."""
    B, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    det = torch.are_deterministic_algorithms_enabled()
    ws = None
    if det:
        nbytes = gs._native.ws_bytes("gs_chamfer_backward_det_ws_bytes", B, Na, Nb)
        assert nbytes >= align256(B * Na * ROW * 4) + align256(B * Nb * ROW * 4)
        ws = prepare_ws(gs, nbytes, "chamfer_bwd", fill or "zero")
    out = (torch.full_like(a, sentinel), torch.full_like(b, sentinel))
    g_a, g_b = gs.ops.chamfer_backward_raw(a, b, ca, cb, kab, kba, g2.to(DEV), g1.to(DEV), out=out)
    torch.cuda.synchronize()
    r0 = r1 = None
    if det:
        r0 = read_rows(gs, ws, "chamfer_bwd", 0, (B, Na))
        r1 = read_rows(gs, ws, "chamfer_bwd", align256(B * Na * ROW * 4), (B, Nb))
    return g_a.cpu().numpy(), g_b.cpu().numpy(), r0, r1


def _chamfer_scene():
    rng = np.random.RandomState(60)
    counts = ((327, 130), (1000, 49))  # rows of a per batch element, rows of b per batch element
    Na, Nb = 327, 1000
    a = np.full((2, Na, 3), np.nan, np.float32)
    b = np.full((2, Nb, 3), np.nan, np.float32)
    for k in range(2):
        a[k, :counts[0][k]] = rng.rand(counts[0][k], 3) * 2.0
        b[k, :counts[1][k]] = rng.rand(counts[1][k], 3) * 2.0
    a[0, 5] = b[0, 17]  # a source lying exactly on its target
    t = lambda x: torch.from_numpy(x).to(DEV)
    return t(a), t(b), torch.tensor(counts[0], dtype=torch.int32, device=DEV), torch.tensor(counts[1], dtype=torch.int32, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [0, 1], ids=["a_to_b", "b_to_a"])
def test_chamfer_scattered_part_is_the_fold_of_the_rows(gs, det_flag, d):
    """B = 2, ragged counts (327 / 130 against 1000 / 49), one direction at a time (the other direction's g2, g1 zero, so the
    target cloud's adjoint is the scattered part alone and the source cloud's the direct part alone): one fold per batch
    element, lg = ceil(log2 cap) of the source side; rows at or beyond the target's count keep their fill."""
    a, b, ca, cb = _chamfer_scene()
    _, kab, kba = gs.ops.chamfer_raw(a, b, ca, cb)
    rng = np.random.RandomState(64 + d)
    g2, g1 = torch.zeros(2, 2), torch.zeros(2, 2)
    g2[:, d] = torch.from_numpy(rng.rand(2).astype(np.float32) + 0.5)
    g1[:, d] = torch.from_numpy(rng.rand(2).astype(np.float32) + 0.5)
    det_flag(True)
    g_a, g_b, r0, r1 = _chamfer_bwd(gs, a, b, ca, cb, kab, kba, g2, g1, "stale")
    z_a, z_b, _, _ = _chamfer_bwd(gs, a, b, ca, cb, kab, kba, g2, g1, "zero")
    assert same_bits(g_a, z_a) and same_bits(g_b, z_b)
    rows, g_src, g_tgt = (r0, g_a, g_b) if d == 0 else (r1, g_b, g_a)
    cs, ct = ((ca, cb) if d == 0 else (cb, ca))
    cs, ct = cs.cpu().numpy(), ct.cpu().numpy()
    cap_s = rows.shape[1]
    for k in range(2):
        mine = rows[k, :cs[k]]
        assert_rows_are_fresh(mine, int(ct[k]))
        assert (mine[:, 6] >= 0).all() and not mine[:, 3:6].any()  # every source has a neighbour; no normal part
        want = fold_of_rows(mine, int(ct[k]), lg_of(cap_s))
        assert same_bits(g_tgt[k, :ct[k]], want[:, :3])
        assert (g_tgt[k, ct[k]:] == 7.0).all() and (g_src[k, cs[k]:] == 7.0).all()
        hit = np.bincount(mine[:, 6], minlength=int(ct[k])) > 0
        assert not bits(g_tgt[k, :ct[k]][~hit]).any() and g_tgt[k, :ct[k]][hit].any()
        # the direct part is the negated row (cham_contrib: the target receives -v): 0 + v
        v = np.float32(0.0) - np.ascontiguousarray(mine[:, :3]).view(np.float32)
        assert same_bits(g_src[k, :cs[k]], np.float32(0.0) + v)
    if d == 0:
        assert r0[0, 5, 6] == 17 and not (r0[0, 5, :3] & 0x7FFFFFFF).any()  # the source on its target contributes zeros


@pytest.mark.gpu
def test_chamfer_rows_are_the_contributions(gs, det_flag):
    """Direction a -> b on duplicated targets b' = b[j_i]: every target has one source, the fold of one term is that term,
    so g_b'[i] is row i of the original call and the negated direct part g_a[i], bit for bit; the original g_b is the rule
    over those; and the flag-off path (one float atomic onto zero) gives the same bits."""
    a, b, ca, cb = _chamfer_scene()
    B, Na = a.shape[0], a.shape[1]
    _, kab, kba = gs.ops.chamfer_raw(a, b, ca, cb)
    g2 = torch.tensor([[0.75, 0.0], [1.25, 0.0]])
    g1 = torch.tensor([[0.5, 0.0], [1.5, 0.0]])
    det_flag(True)
    g_a, g_b, r0, _ = _chamfer_bwd(gs, a, b, ca, cb, kab, kba, g2, g1, "stale")
    n_a, n_b = ca.cpu().numpy(), cb.cpu().numpy()
    j = (kab & 0xFFFFFFFF).cpu().numpy()
    b2 = torch.full((B, Na, 3), float("nan"), device=DEV)
    for k in range(B):
        b2[k, :n_a[k]] = b[k, torch.from_numpy(j[k, :n_a[k]]).to(DEV)]
    kab2 = (kab & ~0xFFFFFFFF) | torch.arange(Na, device=DEV)[None]
    kab2 = torch.where(kab == -1, kab, kab2)
    none = torch.full((B, Na), -1, dtype=torch.int64, device=DEV)
    d_a, d_b, d0, _ = _chamfer_bwd(gs, a, b2, ca, ca, kab2, none, g2, g1, "stale")
    det_flag(False)
    f_a, f_b, _, _ = _chamfer_bwd(gs, a, b2, ca, ca, kab2, none, g2, g1, sentinel=0.0)
    lg = lg_of(Na)
    for k in range(B):
        n = n_a[k]
        assert np.array_equal(d0[k, :n, :6], r0[k, :n, :6]) and np.array_equal(d0[k, :n, 6], np.arange(n))
        words = np.ascontiguousarray(r0[k, :n, :3]).view(np.float32)
        single = np.array([[fold_rule_f32(words[i, c:c + 1], lg, words) for c in range(3)] for i in range(n)], np.float32)
        assert same_bits(d_b[k, :n], single) and ((bits(single) == bits(words)) | (words == 0)).all()
        assert same_bits(d_b[k, :n], np.float32(0.0) - g_a[k, :n]) and same_bits(d_a[k, :n], g_a[k, :n])
        refold = np.array([[fold_rule_f32(d_b[k, :n][j[k, :n] == t, c], lg, d_b[k, :n]) for c in range(3)] for t in range(n_b[k])], np.float32)
        assert same_bits(g_b[k, :n_b[k]], refold)
        assert same_bits(f_b[k, :n], d_b[k, :n]) and same_bits(f_a[k, :n], d_a[k, :n])
