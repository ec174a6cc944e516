"""GPU tests: the entry points that tests/test_workspace_exact.py does not hold -- compaction, the per-op ICP stages, the
one-call map updates and their reverse passes, taped localisation, rendering, the metrics, voxels and neighbours, the TSDF
reverse passes and extraction, RGB-D and SDF odometry -- run in a workspace (and, where they take one, a tape) of EXACTLY the
queried size, on 0xA5 and on 0xFF bytes, between guard bands, and give the bits they give on the cached workspace after a
larger call of the same kind has used it (tests/workspace_check.py).  What the entries compute is their families' tests'.

Each shape is the smallest at which every piece of the entry's workspace holds more than one of its units and ends off a
boundary (the constants are named at the cases); each `dirty=` shape is about twice that in every extent.  Each case first
asserts that its input is not degenerate, so that "wrote nothing" is never why two runs agree.

And one CPU test: the cases of the two files, as registered with covers(), are exactly the header's declarations that take
(ws, ws_bytes) -- a new entry point without a case fails there, before any GPU run.

Not bitwise (float atomics into the compared outputs; their `_det` twins carry the bitwise claim): gs_slam_localize_backward and
gs_chamfer_backward.  gs_rgbd_odometry_taped / gs_rgbd_odometry_bwd take their tape without a size, so only the guards around a
tape of exactly gs_rgbd_odometry_tape_size bytes speak for it."""
import math
import types

import pytest
import torch

from tests import workspace_check
from tests.workspace_check import DEV, at, check_exact, deterministic, frames, make_clouds, make_table, valid_points

gpu = pytest.mark.gpu
covers = lambda *entries: workspace_check.covers(__name__, *entries)


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


def rand(*shape, seed=0, lo=0.0, hi=1.0):
    g = torch.Generator(DEV).manual_seed(seed)
    return lo + (hi - lo) * torch.rand(*shape, device=DEV, generator=g)


def i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def cached(key, fn, held={}):
    """fn() once per run under `key` (inputs that several cases share, and the `dirty=` ones)."""
    if key not in held:
        held[key] = fn()
    return held[key]


# ------------------------------------------------------------------ compaction: kCB = 1024 rows per block (gs_compact.hpp); 1025
# rows = two blocks, one row in the second; arrays of widths 3 and 1; a run of kept rows across the seam at row 1024
def _compact_inputs(n, seed=0):
    a, b = rand(n, 3, seed=seed), rand(n, 1, seed=seed + 1)
    mask = (rand(n, seed=seed + 2) < 0.4).to(torch.uint8)
    mask[1018:min(n, 1031)] = 1
    mask[5:9] = 0
    assert int(mask.sum()) > 0 and int(mask[1024:].sum()) > 0
    return a, b, mask


@gpu
@covers("gs_compact_rows")
def test_compact_rows(gs, monkeypatch):
    a, _, mask = _compact_inputs(1025)
    big, _, big_mask = _compact_inputs(2051, seed=7)
    check_exact(gs, monkeypatch, "gs_compact_rows", lambda: gs.ops.compact_rows(a, mask), outs=at("gs_compact_rows", "out", "out_count"),
                dirty=lambda: gs.ops.compact_rows(big, big_mask))


@gpu
@covers("gs_compact_multi")
def test_compact_multi(gs, monkeypatch):
    a, b, mask = _compact_inputs(1025)
    big_a, big_b, big_mask = _compact_inputs(2051, seed=7)
    held = []
    run = lambda: held.append(gs.ops.compact_multi_raw([a, b], mask))  # (the outputs travel in a host array: held here)
    check_exact(gs, monkeypatch, "gs_compact_multi", run, outs=lambda: held[0][0] + [held[0][1]],
                dirty=lambda: gs.ops.compact_multi_raw([big_a, big_b], big_mask))


@gpu
@covers("gs_expand_multi")
def test_expand_multi(gs, monkeypatch):
    """The adjoint of compact_multi: ops._MultiMaskSelectFn.backward, called as autograd calls it (its outputs travel in a
    host array, so the case holds what it returns)."""
    def inputs(n, seed):
        a, b, mask = _compact_inputs(n, seed)
        k = int(mask.sum())
        ctx = types.SimpleNamespace(saved_tensors=(mask,), shapes=[a.shape, b.shape])
        return ctx, rand(k, 3, seed=seed + 3), rand(k, 1, seed=seed + 4)

    small, big = inputs(1025, 0), inputs(2051, 7)
    held = []
    run = lambda: held.append(gs.ops._MultiMaskSelectFn.backward(*small))
    check_exact(gs, monkeypatch, "gs_expand_multi", run, outs=lambda: list(held[0][2:]),
                dirty=lambda: gs.ops._MultiMaskSelectFn.backward(*big))


# ------------------------------------------------------------------ the table fixture of test_workspace_exact.py: 12 x 16, B = 2,
# Nmax 70, counts 70 / 50; its `dirty=` twin: 24 x 32, Nmax 140, counts 140 / 100
def table(gs):
    return cached("table", lambda: make_table(gs, 12, 16, 70, (70, 50)))


def big_table(gs):
    return cached("big_table", lambda: make_table(gs, 24, 32, 140, (140, 100)))


def _rows(gs, t, ds=0):
    rows, cnt = gs.ops.project_active_raw(t["mp"], t["counts"], t["P"][:, 1].contiguous(), t["K"][:, 0].contiguous(), t["H"], t["W"], ds)
    assert 0 < int(cnt) <= t["B"] * t["Nmax"]
    return rows, cnt


@gpu
@covers("gs_gather_table_rows")
def test_gather_table_rows(gs, monkeypatch):
    def call(t):
        rows, cnt = _rows(gs, t)
        return lambda: gs.ops.gather_table_rows_raw(rows, cnt, t["B"] * t["Nmax"], t["mp"], t["Nmax"])

    check_exact(gs, monkeypatch, "gs_gather_table_rows", call(table(gs)), outs=at("gs_gather_table_rows", "out", "counts"),
                dirty=call(big_table(gs)))


# ------------------------------------------------------------------ per-op ICP: the clouds fixture (65 sources: two 64-point tiles,
# one lane in the second; 130 targets); `dirty=`: 131 / 261
def clouds(gs):
    return cached("clouds", lambda: make_clouds(gs, 65, 130))


def big_clouds(gs):
    return cached("big_clouds", lambda: make_clouds(gs, 131, 261))


@gpu
@covers("gs_knn1")
def test_knn1(gs, monkeypatch):
    src, tgt, _, _ = clouds(gs)
    big_src, big_tgt, _, _ = big_clouds(gs)
    idx = gs.ops.knn1_unpack(gs.ops.knn1_raw(src, tgt))[1]
    assert bool(((idx >= 0) & (idx < tgt.shape[0])).all()) and len(set(idx.tolist())) > 1  # every source found a neighbour
    check_exact(gs, monkeypatch, "gs_knn1", lambda: gs.ops.knn1_raw(src, tgt), outs=at("gs_knn1", "best"),
                dirty=lambda: gs.ops.knn1_raw(big_src, big_tgt))


@gpu
@covers("gs_icp_linearize")
def test_icp_linearize(gs, monkeypatch):
    def call(c):
        src, tgt, nrm, _ = c
        best = gs.ops.knn1_raw(src, tgt)
        assert float(gs.ops.icp_linearize_raw(src, tgt, nrm, best, 0.5)[43]) > 0  # pairs inside the threshold
        return lambda: gs.ops.icp_linearize_raw(src, tgt, nrm, best, 0.5)

    check_exact(gs, monkeypatch, "gs_icp_linearize", call(clouds(gs)), outs=at("gs_icp_linearize", "out44"), dirty=call(big_clouds(gs)))


@gpu
@covers("gs_icp_linearize_backward_det")
def test_icp_linearize_backward_det(gs, monkeypatch):
    def call(c):
        best = gs.ops.knn1_raw(c[0], c[1])

        def run():
            src, tgt, nrm = (x.clone().requires_grad_(True) for x in c[:3])
            with deterministic(True):
                H, g, e = gs.ops.icp_linearize(src, tgt, nrm, best, 0.5)
                ((H * torch.arange(36.0, device=DEV).view(6, 6)).sum() + g.sum() + 2.0 * e).backward()
            assert bool(src.grad.abs().sum() > 0)
        return run

    # (the wrapper hands the kernels zeroed adjoints)
    check_exact(gs, monkeypatch, "gs_icp_linearize_backward_det", call(clouds(gs)),
                outs=at("gs_icp_linearize_backward_det", "g_src", "g_tgt", "g_normals"), fill=0, dirty=call(big_clouds(gs)))


# ------------------------------------------------------------------ the one-call map updates: the table fixture's frame 1 into an
# arena of Nmax + H W rows that holds the map of frame 0
DIST_TH, DOT_TH, SIGMA = 0.0625, math.cos(math.radians(20.0)), 1.5


def _arena(t, seed=0):
    """(depth, rgb, K, poses, [points, normals, colors, ccounts], counts, stats) of the live frame and a fresh arena."""
    B, cap, n = t["B"], t["Nmax"] + t["H"] * t["W"], t["Nmax"]
    mk = lambda c: torch.zeros(B, cap, c, device=DEV)
    mp, mn, mc, cc = mk(3), mk(3), mk(3), mk(1)
    mp[:, :n], mn[:, :n] = t["mp"], t["mn"]
    for b, k in enumerate(t["counts"].tolist()):
        mc[b, :k], cc[b, :k] = rand(k, 3, seed=seed + b), 1.0
    depth, rgb = t["depth"][:, 1].contiguous(), t["rgb"][:, 1].contiguous()
    assert int((depth > 0).sum()) > 0
    return (depth, rgb, t["K"], t["P"][:, 1:2].contiguous(), [mp, mn, mc, cc], t["counts"].clone(),
            torch.zeros(4 + B, dtype=torch.int32, device=DEV))


def _update(gs, t, taped):
    depth, rgb, K, poses, arena, counts, stats = _arena(t)
    fn = gs.ops.pointfusion_update_taped_raw if taped else gs.ops.pointfusion_update_raw
    before = counts.clone()

    def run():
        fn(depth, rgb, K, poses, *arena, counts, DIST_TH, DOT_TH, SIGMA, stats)
        assert bool((counts > before).all()) and bool((stats != 0).any()), (counts.tolist(), stats.tolist())  # rows appended in both elements
    return arena + [counts, stats], run


@gpu
@covers("gs_pointfusion_update", "gs_pointfusion_update_taped")
@pytest.mark.parametrize("taped", [False, True], ids=["plain", "taped"])
def test_pointfusion_update(gs, monkeypatch, taped):
    """Everything is updated in place: the arena, its counts and the step's counters are put back in front of every run."""
    entry = "gs_pointfusion_update" + ("_taped" if taped else "")
    state, run = _update(gs, table(gs), taped)
    dirty = _update(gs, big_table(gs), taped)[1]
    check_exact(gs, monkeypatch, entry, run, outs=[], inout=state, dirty=dirty, **(dict(tape=at(entry, "tape")[0], tape_out=True) if taped else {}))


@gpu
@covers("gs_pointfusion_update_backward")
def test_pointfusion_update_backward(gs, monkeypatch):
    """One frame back over the tape of the taped update: the arena (restored to the previous frame's), its counts and the running
    adjoint of the whole map are updated in place, the frame's four adjoints are written."""
    def call(t, seed):
        depth, rgb, K, poses, arena, counts, stats = _arena(t, seed)
        nmax = arena[0].shape[1]
        tape = gs.ops.pointfusion_update_taped_raw(depth, rgb, K, poses, *arena, counts, DIST_TH, DOT_TH, SIGMA, stats)
        G = [rand(*a.shape, seed=seed + 10 + k, lo=-1.0) for k, a in enumerate(arena)]
        g = [torch.empty(t["B"], t["H"], t["W"], 3, device=DEV) for _ in range(4)]
        state = arena + [counts] + G
        held = [x.clone() for x in state]

        def run():  # (from the state after the forward, whatever an earlier run made of it)
            for x, h in zip(state, held):
                x.copy_(h)
            gs.ops.pointfusion_update_backward_raw(depth, rgb, K, poses, *arena, counts, nmax, SIGMA, tape, *G, *g)
            assert all(bool(torch.isfinite(x).all()) and bool(x.abs().sum() > 0) for x in g) and bool((counts < held[4]).all())
        return state, g, run

    state, g, run = call(table(gs), 0)
    e = "gs_pointfusion_update_backward"
    check_exact(gs, monkeypatch, e, run, outs=at(e, "g_vertex", "g_gvertex", "g_gnormal", "g_rgb"), inout=state, tape=at(e, "tape")[0],
                dirty=call(big_table(gs), 50)[2])


@gpu
@covers("gs_aggregate_update")
def test_aggregate_update(gs, monkeypatch):
    def call(t):
        depth, rgb, K, poses, arena, counts, stats = _arena(t)
        before = counts.clone()

        def run():
            gs.ops.aggregate_update_raw(depth, rgb, K, poses, *arena[:3], counts, stats)
            assert bool((counts > before).all())  # valid pixels appended in both elements
        return arena[:3] + [counts, stats], run

    state, run = call(table(gs))
    check_exact(gs, monkeypatch, "gs_aggregate_update", run, outs=[], inout=state, dirty=call(big_table(gs))[1])


def _merge_inputs(gs, t, seed=0):
    """The unique correspondences of the table's frame 1 and what the merge reads besides."""
    rows, cnt = _rows(gs, t)
    gV, gN, rgb = (t[k][:, 1:2].contiguous() for k in ("gV", "gN", "rgb"))
    urows, ucnt = gs.ops.fusion_unique_raw(rows, None, cnt, t["B"] * t["Nmax"], gV, t["mp"], t["cc"])
    n = int(ucnt)
    assert n > 0 and len(set(urows[:n, 0].tolist())) == t["B"]  # matched rows in every batch element
    alpha = rand(t["B"], 1, t["H"], t["W"], 1, seed=seed, lo=0.1)
    mc = rand(t["B"], t["Nmax"], 3, seed=seed + 1)
    return urows[:n].contiguous(), n, gV, gN, rgb, alpha, t["counts"], t["mp"], t["mn"], mc, t["cc"]


@gpu
@covers("gs_fusion_merge")
def test_fusion_merge(gs, monkeypatch):
    def call(t):
        rows, n, *rest = _merge_inputs(gs, t)
        return lambda: gs.ops.fusion_merge_raw(rows, gs.ops.dev_int(n, DEV), n, *rest)

    e = "gs_fusion_merge"
    check_exact(gs, monkeypatch, e, call(table(gs)), outs=at(e, "out_points", "out_normals", "out_colors", "out_ccounts"),
                dirty=call(big_table(gs)))


@gpu
@covers("gs_fusion_merge_backward")
def test_fusion_merge_backward(gs, monkeypatch):
    def call(t):
        rows, n, gV, gN, rgb, alpha, counts, mp, mn, mc, cc = _merge_inputs(gs, t)

        def run():
            leaves = [x.clone().requires_grad_(True) for x in (gV, gN, rgb, alpha, mp, mn, mc, cc)]
            outs = gs.ops.fusion_merge(rows, counts, *leaves)
            sum((o * rand(*o.shape, seed=20 + k, lo=-1.0)).sum() for k, o in enumerate(outs)).backward()
            assert all(bool(x.grad.abs().sum() > 0) for x in leaves)
        return run

    e = "gs_fusion_merge_backward"  # (the wrapper hands the kernels zeroed frame adjoints)
    outs = at(e, "g_in_points", "g_in_normals", "g_in_colors", "g_in_ccounts", "g_gvertex", "g_gnormal", "g_rgb", "g_alpha")
    check_exact(gs, monkeypatch, e, call(table(gs)), outs=outs, fill=0, dirty=call(big_table(gs)))


@gpu
@covers("gs_fusion_merge_inplace")
def test_fusion_merge_inplace(gs, monkeypatch):
    """(no wrapper: the call in ops' words, on gs_fusion_merge's workspace)"""
    ops = gs.ops

    def call(t):
        rows, n, gV, gN, rgb, alpha, counts, mp, mn, mc, cc = _merge_inputs(gs, t)
        state = [x.clone() for x in (mp, mn, mc, cc)]
        before = [x.clone() for x in state]
        n_dev = ops.dev_int(n, DEV)

        def run():
            ws = ops.workspace(ops.ws_bytes("gs_fusion_merge_ws_bytes", t["B"], t["Nmax"]), DEV, "merge")
            ops.call("gs_fusion_merge_inplace", ops.ptr(rows), ops.ptr(n_dev), n, ops.ptr(gV), ops.ptr(gN), ops.ptr(rgb), ops.ptr(alpha), t["B"],
                     t["H"], t["W"], t["Nmax"], ops.ptr(counts), *(ops.ptr(x) for x in state), ops.ptr(ws), ws.numel(), ops.stream())
            assert all(not torch.equal(a, b) for a, b in zip(state, before))  # every array merged into
        return state, run

    state, run = call(table(gs))
    check_exact(gs, monkeypatch, "gs_fusion_merge_inplace", run, outs=[], inout=state, dirty=call(big_table(gs))[1])


# ------------------------------------------------------------------ taped localisation: 24 x 32, ds 2, 2 iterations, B = 2 with
# maps of every second valid point of frame 0 (274 / 268 rows: the even ones, the odd ones -- subsets at which the loop accepts
# a step in both elements); `dirty=`: 48 x 64, every third point (851 / 847 rows)
def _localize_inputs(gs, H, W, picks):
    f = frames(gs, 2, 2, H, W)
    clouds = [[x[pick].contiguous() for x in valid_points(f, b, 0)] for b, pick in enumerate(picks)]
    counts = [c[0].shape[0] for c in clouds]
    assert counts[0] != counts[1]
    mp, mn = torch.zeros(2, max(counts), 3, device=DEV), torch.zeros(2, max(counts), 3, device=DEV)
    for b, (p, n) in enumerate(clouds):
        mp[b, :counts[b]], mn[b, :counts[b]] = p, n
    depth, prev = f["depth"][:, 1:2].contiguous(), f["P"][:, :1].contiguous()
    gV = gs.ops.vertex_normal_maps_raw(depth, f["K"], prev, want_local=False)[2]
    return gV, depth, f["K"], prev, mp, mn, i32(counts)


def _localize_autograd(gs, inputs, det):
    gV, depth, K, prev, mp, mn, counts = inputs
    gV, prev, mp, mn = (x.clone().requires_grad_(True) for x in (gV, prev, mp, mn))
    with deterministic(det):
        out = gs.ops.slam_localize_autograd(gV, depth, K, prev, mp, mn, counts, 2, 2, 1e-8, 0.1)
        assert bool(((out.detach() - prev.detach()).abs().amax(dim=(1, 2, 3)) > 0).all())  # a step was taken in both elements
        (out * rand(*out.shape, seed=3, lo=-1.0)).sum().backward()
    assert all(bool(x.grad.abs().sum() > 0) for x in (gV, prev, mp, mn))


FUSED = pytest.mark.parametrize("fused", [1, 0], ids=["fused_front", "separate_front"])


def _localize_case(gs, monkeypatch, fused, entry, det, **kw):
    small = cached("localize", lambda: _localize_inputs(gs, 24, 32, (slice(0, None, 2), slice(1, None, 2))))
    big = cached("big_localize", lambda: _localize_inputs(gs, 48, 64, (slice(0, None, 3), slice(1, None, 3))))
    lib = gs._native.lib()
    lib.gs_set_fused_setup(fused)
    try:
        check_exact(gs, monkeypatch, entry, lambda: _localize_autograd(gs, small, det), dirty=lambda: _localize_autograd(gs, big, det),
                    tape=at(entry, "tape")[0], **kw)
    finally:
        lib.gs_set_fused_setup(1)


@gpu
@covers("gs_slam_localize_taped")
@FUSED
def test_slam_localize_taped(gs, monkeypatch, fused):
    _localize_case(gs, monkeypatch, fused, "gs_slam_localize_taped", False, outs=at("gs_slam_localize_taped", "out_poses"), tape_out=True)


@gpu
@covers("gs_slam_localize_backward", "gs_slam_localize_backward_det")
@FUSED
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
def test_slam_localize_backward(gs, monkeypatch, fused, det):
    entry = "gs_slam_localize_backward" + ("_det" if det else "")
    outs = at(entry, "grad_gvertex", "grad_map_points", "grad_map_normals", "grad_prev_poses")
    _localize_case(gs, monkeypatch, fused, entry, det, outs=outs, bitwise=det)


# ------------------------------------------------------------------ rendering: B = 2, 9 x 29 = 261 pixels (two 256-pixel blocks,
# five pixels in the second), maps of 130 / 70 rows; `dirty=`: 18 x 58, 260 / 140 rows
def _render_inputs(gs, H, W, Nmax, counts):
    t = make_table(gs, 2 * H, 2 * W, Nmax, counts, every=5)  # (the map: every fifth valid point of the scene at twice the size)
    cam = frames(gs, 2, 2, H, W)
    mc = rand(t["B"], Nmax, 3, seed=5)
    poses, K = cam["P"][:, 1].contiguous(), cam["K"][:, 0].contiguous()
    index = gs.ops.render_map_raw(t["mp"], t["mn"], mc, t["counts"], poses, K, H, W)[0]
    assert bool(((index >= 0).sum(dim=(1, 2)) > 1).all())  # pixels that show a row in both elements
    g = [rand(t["B"], H, W, seed=6, lo=-1.0)] + [rand(t["B"], H, W, 3, seed=7 + k, lo=-1.0) for k in range(3)]
    return t["mp"], t["mn"], mc, t["counts"], poses, K, H, W, index, g


def _render(gs):
    return (cached("render", lambda: _render_inputs(gs, 9, 29, 130, (130, 70))), cached("big_render", lambda: _render_inputs(gs, 18, 58, 260, (260, 140))))


@gpu
@covers("gs_render_map")
def test_render_map(gs, monkeypatch):
    small, big = _render(gs)
    e = "gs_render_map"
    check_exact(gs, monkeypatch, e, lambda: gs.ops.render_map_raw(*small[:8]),
                outs=at(e, "out_index", "out_depth", "out_points", "out_normals", "out_colors"), dirty=lambda: gs.ops.render_map_raw(*big[:8]))


@gpu
@covers("gs_render_map_backward")
def test_render_map_backward(gs, monkeypatch):
    small, big = _render(gs)
    call = lambda s: (lambda: gs.ops.render_map_backward_raw(s[0], s[3], s[4], s[8], *s[9]))
    e = "gs_render_map_backward"
    check_exact(gs, monkeypatch, e, call(small), outs=at(e, "g_points", "g_normals", "g_colors", "g_poses"), dirty=call(big))


# ------------------------------------------------------------------ metrics: (Na, Nb) = (65, 15) in element 0, (15, 65) in element 1;
# `dirty=`: 131 / 31
def _chamfer_inputs(gs, n, m, seed):
    a, b = rand(2, n, 3, seed=seed), rand(2, n, 3, seed=seed + 1)
    ca, cb = i32((n, m)), i32((m, n))
    stats, kab, kba = gs.ops.chamfer_raw(a, b, ca, cb)
    assert bool((stats[:, :, 0] > 0).all())
    return a, b, ca, cb, kab, kba, rand(2, 2, seed=seed + 2, lo=0.5), rand(2, 2, seed=seed + 3, lo=0.5)


def _chamfer(gs):
    return cached("chamfer", lambda: _chamfer_inputs(gs, 65, 15, 0)), cached("big_chamfer", lambda: _chamfer_inputs(gs, 131, 31, 9))


@gpu
@covers("gs_chamfer")
def test_chamfer(gs, monkeypatch):
    small, big = _chamfer(gs)
    check_exact(gs, monkeypatch, "gs_chamfer", lambda: gs.ops.chamfer_raw(*small[:4]), outs=at("gs_chamfer", "stats", "keys_ab", "keys_ba"),
                dirty=lambda: gs.ops.chamfer_raw(*big[:4]))


@gpu
@covers("gs_chamfer_backward", "gs_chamfer_backward_det")
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
def test_chamfer_backward(gs, monkeypatch, det):
    """(the atomics entry's queried size is 0: the pointer at the guard boundary, ws_bytes = 0, the guards checked.  Both add
    into the adjoints, which start from zero.)"""
    small, big = _chamfer(gs)

    def call(s):
        def run():
            with deterministic(det):
                g_a, g_b = gs.ops.chamfer_backward_raw(*s)
            assert bool(g_a.abs().sum() > 0) and bool(g_b.abs().sum() > 0)
        return run

    entry = "gs_chamfer_backward" + ("_det" if det else "")
    check_exact(gs, monkeypatch, entry, call(small), outs=at(entry, "g_a", "g_b"), bitwise=det, fill=0, dirty=call(big))


# ------------------------------------------------------------------ voxels: N = 257 and 130 rows (voxel.hip's 256-thread blocks: two,
# one row in the second), 4 x 4 x 4 cells of 0.3 over the unit cube and its margin, C = 11; `dirty=`: 515 / 260 rows
def _voxel_inputs(gs, N, n1, seed):
    pts, counts = rand(2, N, 3, seed=seed, lo=-0.1, hi=1.1), i32((N, n1))
    voxel_of, n_voxels, _, voxel_count, _ = gs.ops.voxel_assign(pts, counts, 0.3)
    M = int(n_voxels.max())
    assert 10 <= int(n_voxels.min()) and M <= 125
    return pts, counts, rand(2, N, 11, seed=seed + 1, lo=-1.0), voxel_of, n_voxels, voxel_count, M


def _voxels(gs):
    return cached("voxels", lambda: _voxel_inputs(gs, 257, 130, 0)), cached("big_voxels", lambda: _voxel_inputs(gs, 515, 260, 4))


@gpu
@covers("gs_voxel_assign")
def test_voxel_assign(gs, monkeypatch):
    small, big = _voxels(gs)
    e = "gs_voxel_assign"
    check_exact(gs, monkeypatch, e, lambda: gs.ops.voxel_assign(small[0], small[1], 0.3),
                outs=at(e, "voxel_of", "n_voxels", "n_dropped", "voxel_count", "voxel_first"), dirty=lambda: gs.ops.voxel_assign(big[0], big[1], 0.3))


@gpu
@covers("gs_voxel_reduce")
@pytest.mark.parametrize("mode", [0, 1], ids=["sum", "mean"])
def test_voxel_reduce(gs, monkeypatch, mode):
    small, big = _voxels(gs)
    call = lambda s: (lambda: gs.ops.voxel_reduce_raw(s[2], s[1], s[3], s[4], s[5], s[6], mode))
    check_exact(gs, monkeypatch, "gs_voxel_reduce", call(small), outs=at("gs_voxel_reduce", "out"), dirty=call(big))


# ------------------------------------------------------------------ neighbours: Ns 65 (40 in element 1), Nt 130 (77), K = 8;
# `dirty=`: 131 (80) / 261 (150)
def _knn_inputs(gs, ns, ns1, nt, nt1, seed):
    src, tgt, cs, ct = rand(2, ns, 3, seed=seed), rand(2, nt, 3, seed=seed + 1), i32((ns, ns1)), i32((nt, nt1))
    keys = gs.ops.knn_raw(src, tgt, cs, ct, 8)
    assert bool((keys[0, :ns] != -1).all()) and bool((keys[1, :ns1] != -1).all())
    return src, tgt, cs, ct, keys, rand(2, ns, 8, seed=seed + 2, lo=-1.0)


def _knn(gs):
    return cached("knn", lambda: _knn_inputs(gs, 65, 40, 130, 77, 0)), cached("big_knn", lambda: _knn_inputs(gs, 131, 80, 261, 150, 5))


@gpu
@covers("gs_knn")
def test_knn(gs, monkeypatch):
    small, big = _knn(gs)
    check_exact(gs, monkeypatch, "gs_knn", lambda: gs.ops.knn_raw(*small[:4], 8), outs=at("gs_knn", "keys"), dirty=lambda: gs.ops.knn_raw(*big[:4], 8))


@gpu
@covers("gs_knn_backward")
def test_knn_backward(gs, monkeypatch):
    small, big = _knn(gs)
    check_exact(gs, monkeypatch, "gs_knn_backward", lambda: gs.ops.knn_backward_raw(*small), outs=at("gs_knn_backward", "g_src", "g_tgt"),
                dirty=lambda: gs.ops.knn_backward_raw(*big))


# ------------------------------------------------------------------ TSDF volumes, stated analytically (x fastest, B = 2)
V, TRUNC, MAXW = 0.05, 0.15, 2.0


def _centres(dims, origin):
    nx, ny, nz = dims
    z, y, x = torch.meshgrid(torch.arange(nz, device=DEV), torch.arange(ny, device=DEV), torch.arange(nx, device=DEV), indexing="ij")
    return torch.stack([x, y, z], -1).float().add(0.5).mul(V) + torch.tensor(origin, device=DEV)


def _cam(fx, cx, cy, B):
    K = torch.eye(4, device=DEV)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fx, cx, cy
    return K.repeat(B, 1, 1, 1).contiguous()  # (B,1,4,4)


def _poses(B, L):
    """Cameras at the world's origin looking down +z, each moved by a few millimetres of its own."""
    P = torch.eye(4, device=DEV).repeat(B, L, 1, 1)
    P[:, :, :3, 3] = rand(B, L, 3, seed=11, lo=-0.004, hi=0.004)
    return P.contiguous()


ORIGINS = [(-0.125, -0.075, 1.0), (-0.12, -0.08, 1.01)]  # a (5, 3, 2) volume in front of the cameras, per batch element


def _slab(dims, seed):
    """tsdf, weight, color, origin of a tilted plane through the middle of the volume's z extent."""
    cent = torch.stack([_centres(dims, o) for o in ORIGINS])
    mid = torch.tensor([o[2] + 0.5 * V * dims[2] for o in ORIGINS], device=DEV).view(2, 1, 1, 1)
    tsdf = ((mid + 0.1 * cent[..., 0] - 0.05 * cent[..., 1] - cent[..., 2]) / TRUNC).clamp(-1.0, 1.0).contiguous()
    weight = rand(*tsdf.shape, seed=seed, lo=1.0, hi=1.5)
    return tsdf, weight, rand(*tsdf.shape, 3, seed=seed + 1), torch.tensor(ORIGINS, device=DEV)


# integration's reverse: 33 frames (one past the chunk of 32) of 8 x 8 into (5, 3, 2); `dirty=`: 66 frames of 16 x 16 into (10, 6, 4)
def _integrate_inputs(L, H, dims, seed):
    B = 2
    depth = rand(B, L, H, H, seed=seed, lo=1.02, hi=1.0 + V * dims[2] - 0.02)
    depth[:, :, 0, 0] = 0.0
    shape = (B, dims[2], dims[1], dims[0])
    return dict(depth=depth, K=_cam(2.5 * H, (H - 1) / 2.0, (H - 1) / 2.0, B), poses=_poses(B, L), weight=rand(*shape, seed=seed + 1, hi=1.5),
                origin=torch.tensor(ORIGINS, device=DEV), g_tsdf=rand(*shape, seed=seed + 2, lo=-1.0), g_color=rand(*shape, 3, seed=seed + 3, lo=-1.0))


@gpu
@covers("gs_tsdf_integrate_backward", "gs_tsdf_integrate_backward_poses")
@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("how", ["state", "poses", "poses_only_frames"])
def test_tsdf_integrate_backward(gs, monkeypatch, how, color):
    """(poses_only_frames: without g_tsdf_in / g_color_in the adjoints carried from chunk to chunk live in the workspace)"""
    small = cached("integrate", lambda: _integrate_inputs(33, 8, (5, 3, 2), 0))
    big = cached("big_integrate", lambda: _integrate_inputs(66, 16, (10, 6, 4), 20))

    def call(s, check):
        def run():
            args = (s["depth"], s["K"], s["poses"], s["weight"], s["origin"], V, TRUNC, MAXW, s["g_tsdf"], s["g_color"] if color else None)
            if how == "state":
                got = gs.ops.tsdf_integrate_backward_raw(*args)
            else:
                got = gs.ops.tsdf_integrate_backward_poses_raw(*args, want_state=how == "poses")
            if check:
                assert bool((got[2].abs().sum(dim=(1, 2, 3)) > 0).all()) and (how == "state" or bool(got[4].abs().sum() > 0))
        return run

    e = "gs_tsdf_integrate_backward" + ("" if how == "state" else "_poses")
    outs = at(e, "g_tsdf_in", "g_color_in", "g_depth", "g_rgb") + (at(e, "g_poses") if how != "state" else [])
    check_exact(gs, monkeypatch, e, call(small, True), outs=outs, dirty=call(big, False))


# the cast's reverse: (5, 3, 2), 20 x 28 pixels (2 x 2 tiles of 16 x 16 outputs at stride 1), L = 2; `dirty=`: (10, 6, 4), 40 x 56
def _cast_inputs(gs, dims, height, width, stride, seed):
    tsdf, weight, color, origin = _slab(dims, seed)
    K, poses = _cam(3.6 * width, (width - 1) / 2.0, 0.75 * height, 2), _poses(2, 2)  # (the volume lies across the seams of the tiles)
    step = 0.02
    depth, _, _, k_end = gs.ops.tsdf_raycast_raw(tsdf, weight, color, origin, V, K, poses, height, width, stride, step)
    return dict(vol=(tsdf, weight, color, origin), cam=(K, poses, height, width, stride, step, 1.0), k_end=k_end, hits=(k_end > 0).sum(dim=(2, 3)),
                g_depth=rand(*depth.shape, seed=seed + 2, lo=-1.0), g_rgb=rand(*depth.shape, 3, seed=seed + 3, lo=-1.0))


@gpu
@covers("gs_tsdf_raycast_backward", "gs_tsdf_raycast_backward_poses")
@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("how", ["volume", "poses", "poses_only"])
def test_tsdf_raycast_backward(gs, monkeypatch, how, stride, color):
    small = cached(("cast", stride), lambda: _cast_inputs(gs, (5, 3, 2), 20, 28, stride, 0))
    big = cached(("big_cast", stride), lambda: _cast_inputs(gs, (10, 6, 4), 40, 56, stride, 30))
    assert bool((small["hits"] > 1).all()), small["hits"].tolist()  # rays that hit, in every camera

    def call(s):
        tsdf, weight, col, origin = s["vol"]
        args = (tsdf, weight, col if color else None, origin, V, *s["cam"], s["k_end"], s["g_depth"], s["g_rgb"] if color else None)
        if how == "volume":
            return lambda: gs.ops.tsdf_raycast_backward_raw(*args)
        return lambda: gs.ops.tsdf_raycast_backward_poses_raw(*args, want_volume=how == "poses")

    e = "gs_tsdf_raycast_backward" + ("" if how == "volume" else "_poses")
    outs = at(e, "g_tsdf", "g_color") + (at(e, "g_poses") if how != "volume" else [])
    check_exact(gs, monkeypatch, e, call(small), outs=outs, dirty=call(big))


# extraction and faces: (9, 6, 7) = 378 voxels, 1134 edge slots (two blocks of 1024), a sphere per batch element and an unobserved
# slab; `dirty=`: (18, 12, 14)
def _sphere(dims, seed):
    o = torch.tensor([(-0.2, -0.15, 0.9), (-0.22, -0.14, 0.91)], device=DEV)
    size = torch.tensor(dims, device=DEV).float() * V
    cent = torch.stack([_centres(dims, tuple(x.tolist())) for x in o])
    c = (o + size * torch.tensor([(0.5, 0.5, 0.5), (0.45, 0.55, 0.5)], device=DEV)).view(2, 1, 1, 1, 3)
    r = torch.tensor([0.37, 0.31], device=DEV).view(2, 1, 1, 1) * size.min()
    tsdf = (((cent - c).norm(dim=-1) - r) / TRUNC).clamp(-1.0, 1.0).contiguous()
    weight = torch.ones_like(tsdf)
    weight[:, :, :, 0] = 0.0
    return tsdf, weight, rand(*tsdf.shape, 3, seed=seed), o


def _extract_inputs(gs, dims, seed):
    tsdf, weight, color, origin = _sphere(dims, seed)
    n = gs.ops.tsdf_extract_raw(tsdf, weight, color, origin, V, 1.0, cap=0)[4]
    cap = int(n.max())
    assert int(n.min()) > 0 and n[0] != n[1]
    edge = gs.ops.tsdf_extract_raw(tsdf, weight, color, origin, V, 1.0, cap=cap)[3]
    nf = gs.ops.tsdf_faces_raw(tsdf, weight, 1.0, None, None, fcap=0)[1]
    assert int(nf.min()) > 0
    return tsdf, weight, color, origin, cap, edge, n, int(nf.max())


def _extract(gs):
    return cached("extract", lambda: _extract_inputs(gs, (9, 6, 7), 0)), cached("big_extract", lambda: _extract_inputs(gs, (18, 12, 14), 8))


@gpu
@covers("gs_tsdf_extract")
@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_tsdf_extract(gs, monkeypatch, color):
    small, big = _extract(gs)
    call = lambda s: (lambda: gs.ops.tsdf_extract_raw(s[0], s[1], s[2] if color else None, s[3], V, 1.0, cap=s[4]))
    e = "gs_tsdf_extract"
    check_exact(gs, monkeypatch, e, call(small), outs=at(e, "points", "normals", "colors", "edge", "n_points"), dirty=call(big))


@gpu
@covers("gs_tsdf_faces")
def test_tsdf_faces(gs, monkeypatch):
    small, big = _extract(gs)
    call = lambda s: (lambda: gs.ops.tsdf_faces_raw(s[0], s[1], 1.0, s[5], s[6], fcap=s[7], points_fit=True))
    check_exact(gs, monkeypatch, "gs_tsdf_faces", call(small), outs=at("gs_tsdf_faces", "faces", "n_faces"), dirty=call(big))


# ------------------------------------------------------------------ RGB-D odometry: 30 x 45 (1350 pixels: six 256-pixel rows, the
# last partial), 2 levels, iterations (2, 1), B = 2 -- tests/test_rgbd_odometry.py's scene; `dirty=`: 96 x 130
def _rgbd_pair():
    from tests import test_rgbd_odometry as fw

    def make(name):
        t = fw.dev_scene(name)
        t["T"] = fw.dev_T(fw.transforms(name)["true"])
        t["g_sums"] = rand(2, 29, seed=2, lo=-1.0)
        return t
    return cached("rgbd", lambda: (make("30x45"), make("96x130")))


def _rgbd_whole(gs, t, differentiable):
    leaves = [t[k].clone().requires_grad_(differentiable) for k in ("td", "tc", "sd", "sc")]
    init = torch.eye(4, device=DEV).repeat(2, 1, 1).requires_grad_(differentiable)
    T, info = gs.ops.rgbd_odometry(*leaves, t["K"], init=init, numiters=(2, 1), levels=2, differentiable=differentiable)
    assert bool((info[:, :, 0] > 50).all()) and bool((info[:, :, 3] >= 1).all())  # valid pixels and an iteration at every level
    if differentiable:
        (T[:, :3] * rand(2, 3, 4, seed=4, lo=-1.0)).sum().backward()
        assert all(bool(x.grad.abs().sum() > 0) for x in leaves + [init])


@gpu
@covers("gs_rgbd_odometry")
def test_rgbd_odometry(gs, monkeypatch):
    small, big = _rgbd_pair()
    check_exact(gs, monkeypatch, "gs_rgbd_odometry", lambda: _rgbd_whole(gs, small, False), outs=at("gs_rgbd_odometry", "out_T", "info"),
                dirty=lambda: _rgbd_whole(gs, big, False))


@gpu
@covers("gs_rgbd_odometry_taped")
def test_rgbd_odometry_taped(gs, monkeypatch):
    small, big = _rgbd_pair()
    e = "gs_rgbd_odometry_taped"
    check_exact(gs, monkeypatch, e, lambda: _rgbd_whole(gs, small, True), outs=at(e, "out_T", "info"), ws_at=at(e, "ws")[0],
                tape=at(e, "tape")[0], tape_out=True, tape_sized=False, dirty=lambda: _rgbd_whole(gs, big, True))


@gpu
@covers("gs_rgbd_odometry_bwd")
def test_rgbd_odometry_bwd(gs, monkeypatch):
    small, big = _rgbd_pair()
    e = "gs_rgbd_odometry_bwd"
    check_exact(gs, monkeypatch, e, lambda: _rgbd_whole(gs, small, True), outs=at(e, "g_tgt_depth", "g_tgt_rgb", "g_src_depth", "g_src_rgb", "g_init"),
                tape=at(e, "tape")[0], tape_sized=False, dirty=lambda: _rgbd_whole(gs, big, True))


@gpu
@covers("gs_rgbd_rows")
def test_rgbd_rows(gs, monkeypatch):
    small, big = _rgbd_pair()

    def call(t, check):
        def run():
            valid, _, sums = gs.ops.rgbd_rows_raw(t["td"], t["tc"], t["sd"], t["sc"], t["K"], t["T"])
            assert not check or (bool((valid.sum(dim=(1, 2)) > 50).all()) and bool((sums[:, 28] > 50).all()))
        return run

    check_exact(gs, monkeypatch, "gs_rgbd_rows", call(small, True), outs=at("gs_rgbd_rows", "valid", "rows", "sums"), dirty=call(big, False))


@gpu
@covers("gs_rgbd_rows_bwd")
def test_rgbd_rows_bwd(gs, monkeypatch):
    small, big = _rgbd_pair()

    def call(t, check):
        def run():
            grads = gs.ops.rgbd_rows_bwd_raw(t["td"], t["tc"], t["sd"], t["sc"], t["K"], t["T"], t["g_sums"])
            assert not check or all(bool(g.abs().sum() > 0) for g in grads)
        return run

    e = "gs_rgbd_rows_bwd"
    check_exact(gs, monkeypatch, e, call(small, True), outs=at(e, "g_tgt_depth", "g_tgt_rgb", "g_src_depth", "g_src_rgb", "g_T"), dirty=call(big, False))


# ------------------------------------------------------------------ SDF odometry: 30 x 45 at stride 2 (15 x 23 = 345 pixels: two
# 256-pixel rows, the second partial), 2 levels, iterations (2, 1), B = 2 -- tests/test_sdf_odometry.py's scene and volume;
# `dirty=`: 96 x 130 at stride 2
def _sdf_pair():
    from tests import test_sdf_odometry as fw

    def make(name):
        t = fw.dev_scene(name)
        t["D"] = fw.dev_T(fw.deltas("true"))
        return t
    return cached("sdf", lambda: (make("30x45s2"), make("96x130"), fw.V, fw.TRUNC))


@gpu
@covers("gs_sdf_rows")
def test_sdf_rows(gs, monkeypatch):
    small, big, v, trunc = _sdf_pair()

    def call(t, check):
        def run():
            valid, _, sums = gs.ops.sdf_rows_raw(t["depth"], t["K"], t["P"], t["D"], t["tsdf"], t["weight"], t["origin"], v, trunc, stride=2)
            assert not check or (bool((valid.sum(dim=(1, 2)) > 50).all()) and bool((sums[:, 28] > 50).all()))
        return run

    check_exact(gs, monkeypatch, "gs_sdf_rows", call(small, True), outs=at("gs_sdf_rows", "valid", "rows", "sums"), dirty=call(big, False))


@gpu
@covers("gs_sdf_odometry")
def test_sdf_odometry(gs, monkeypatch):
    small, big, v, trunc = _sdf_pair()

    def call(t, check):
        def run():
            T, info = gs.ops.sdf_odometry(t["depth"], t["K"], t["P"], t["tsdf"], t["weight"], t["origin"], v, trunc, numiters=(2, 1), levels=2,
                                          stride=2)
            assert not check or (bool((info[:, :, 0] > 20).all()) and bool((info[:, :, 3] >= 1).all()))
        return run

    check_exact(gs, monkeypatch, "gs_sdf_odometry", call(small, True), outs=at("gs_sdf_odometry", "out_T", "info"), dirty=call(big, False))


# ------------------------------------------------------------------ CPU: the list is whole
def test_every_workspace_entry_has_a_case():
    """Every gs_* declaration of include/gradslam_hip.h that takes (ws, ws_bytes) -- or a sized tape -- is registered by a case of
    this file or of tests/test_workspace_exact.py, and nothing is registered that the header does not declare."""
    from tests import test_workspace_exact

    with open(workspace_check.HEADER) as f:
        declared = workspace_check.header_entries(f.read())
    held = workspace_check.REGISTRY[test_workspace_exact.__name__] | workspace_check.REGISTRY[__name__]
    assert len(declared) >= 53
    assert declared == held, dict(without_a_case=sorted(declared - held), not_declared=sorted(held - declared))
    assert not workspace_check.REGISTRY[test_workspace_exact.__name__] & workspace_check.REGISTRY[__name__]
