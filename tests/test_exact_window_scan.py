"""The grid search's window scan examines each lane's EXACT slot ranges (pix_start[g - 1] .. pix_start[g + 2) per window row), not
whole 16-slot chunks, and tells the fallback searches to skip only the chunks that lie wholly inside those ranges
(csrc/gs_icp_assoc.hpp LaneWin, csrc/gs_lanewin.hpp).  Whatever the ranges look like, every association launch of a loop must
return the brute-force scan's packed (distance, index) keys bit for bit, and the pose must be the chunk-box search's.

Each scene is run as a taped six-iteration loop under eight and sixteen waves per block, LM and gradLM, with the grid search
(proofs on whatever the density: gs_set_grid_search(2)) and with the chunk-box search (0).  Scenes are ds-grid scenes like
tests/test_gpu_parity._grid_scene, but with per-pixel target counts set by hand, so that the ranges' ends fall where the
arithmetic can go wrong.  Lanes that must take an exact search are made so by geometry (tests/test_loop_waves.py): a source
point half a metre in front of the wall has no target inside the proof's bound; one to six such lanes per tile take the
point-serial search, more than six the tile-level search -- the two paths that consult the covered chunks."""
import math

import pytest
import torch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import gradslam_amd

    return gradslam_amd


def scene(n_per, Hd, Wd, seed, ds=4, motion=0.004, src_rows=None):
    """A wavy wall seen through a Wd x Hd ds-grid: n_per[pixel] targets bucketed on every pixel (reference order shuffled), one
    source point on every pixel (all of them: borders included; src_rows: only these pixel rows), moved by a small rigid motion."""
    g = torch.Generator().manual_seed(seed)
    n_per = torch.as_tensor(n_per, dtype=torch.int64)
    assert n_per.shape == (Hd * Wd,)
    fx = fy = 525.0 * (Wd * ds) / 640.0
    cx, cy = (Wd * ds - 1) / 2.0, (Hd * ds - 1) / 2.0
    wall = lambda x, y: 2.0 + 0.3 * torch.sin(2.0 * x) * torch.cos(2.0 * y)

    def backproject(u, v, jitter):
        z = wall((u - cx) / fx * 2.0, (v - cy) / fy * 2.0) + jitter
        return torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)

    cell = torch.arange(Hd * Wd)
    tcell = cell.repeat_interleave(n_per)
    nt = tcell.shape[0]
    u = (tcell % Wd).float() * ds + (torch.rand(nt, generator=g) - 0.5)
    v = (tcell // Wd).float() * ds + (torch.rand(nt, generator=g) - 0.5)
    tgt = backproject(u, v, 0.002 * torch.randn(nt, generator=g))
    perm = torch.randperm(nt, generator=g)
    tgt, tcell = tgt[perm].contiguous(), tcell[perm]
    nrm = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.1 * torch.randn(nt, 3, generator=g), dim=-1)
    order = torch.argsort(tcell, stable=True)
    pix_start = torch.zeros(Hd * Wd + 1, dtype=torch.int64)
    pix_start[1:] = torch.cumsum(n_per, 0)
    sc = cell if src_rows is None else cell[torch.isin(cell // Wd, torch.tensor(src_rows))]
    src = backproject((sc % Wd).float() * ds, (sc // Wd).float() * ds, 0.001 * torch.randn(sc.shape[0], generator=g))
    a = 0.5 * motion
    R = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float32)
    src = (src @ R.t() + torch.tensor([motion, -0.5 * motion, 0.3 * motion])).contiguous()
    K = torch.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return dict(src=src, src_pix=sc.to(torch.int32), tgt=tgt, nrm=nrm.contiguous(), order=order, pix_start=pix_start.to(torch.int32),
                tgt_pix=tcell.to(torch.int32), Wd=Wd, Hd=Hd, cam_pose=torch.eye(4), cam_K=K, ds=ds)


def on_device(sc):
    out = dict(sc)
    out["scan_points"] = sc["tgt"][sc["order"]]
    out["scan_orig"] = sc["order"].to(torch.int32)
    del out["order"]
    return {k: (v.contiguous().to(DEV) if torch.is_tensor(v) else v) for k, v in out.items()}


def off_the_wall(sc, per_tile, tile_points=64):
    """`per_tile` lanes of every tile moved half a metre towards the camera: no target within the proof's bound."""
    n = sc["src"].shape[0]
    for t0 in range(0, n, tile_points):
        sc["src"][t0 + 5: min(t0 + 5 + per_tile, n), 2] -= 0.5
    return sc


def window_rows(sc):
    """(first, one-past-last) slot of the three window rows of every source pixel, as the kernel clamps them (the window centred
    on the point's own pixel: the first launch's, up to the motion)."""
    Wd, Hd, ps = sc["Wd"], sc["Hd"], sc["pix_start"].long()
    nc, rows = Wd * Hd, []
    for p in sc["src_pix"].tolist():
        for r in (-1, 0, 1):
            g = p + r * Wd
            if g + 1 >= 0 and g - 1 <= nc - 1:
                rows.append((int(ps[min(max(g - 1, 0), nc - 1)]), int(ps[min(max(g + 1, 0), nc - 1) + 1])))
    return rows


def check(gs, sc, tile_points=0):
    """Every association of the taped loop == the brute-force scan, grid search and chunk-box search, 8 / 16 waves, LM / gradLM;
    the grid search's pose == the chunk-box search's."""
    from tests import test_gpu_parity as P

    lib = gs._native.lib()
    d = on_device(sc)
    want = {}  # the brute-force keys of a launch's cloud, computed once per distinct cloud

    def reference(cloud):
        k = cloud.cpu().numpy().tobytes()
        if k not in want:
            want[k] = gs.ops.knn1_raw(cloud.contiguous(), d["tgt"], brute_force=True)
        return want[k]

    import ctypes

    counts = (ctypes.c_uint * 4)()
    assert lib.gs_loop_counts(counts, 1) == 0  # (reset)
    try:
        lib.gs_set_tile_points(tile_points)
        for nw in (8, 16):
            assert lib.gs_set_loop_waves(nw) == nw
            for grad_lm in (0, 1):
                T = {}
                for mode in (2, 0):
                    lib.gs_set_grid_search(mode)
                    T[mode], assoc = P._taped_loop_with_hints(gs, d, 6, grad_lm)
                    assert len(assoc) == (12 if grad_lm else 7)
                    for a, (cloud, keys) in enumerate(assoc):
                        bad = (keys != reference(cloud)).sum().item()
                        assert bad == 0, (nw, grad_lm, mode, a, bad)
                assert torch.equal(T[2], T[0]), (nw, grad_lm)
                assert torch.isfinite(T[2]).all()
    finally:
        lib.gs_set_grid_search(1)
        lib.gs_set_tile_points(0)
        assert lib.gs_set_loop_waves(0) == 0
    assert lib.gs_loop_counts(counts, 0) == 0
    assert counts[0] == 8 and counts[1] == 4, list(counts)  # eight loops, four of them as a grid search
    return want


def test_every_offset_inside_a_chunk(gs):
    """A counts pattern of period 11 and sum 19: pix_start mod 16 moves by three per period, so a window row's first slot and its
    one-past-last slot each take all sixteen offsets inside a chunk; nt is no multiple of 16; slot 0 and slot nt are reached."""
    Hd, Wd = 12, 24
    pattern = [0, 1, 2, 3, 5, 1, 0, 4, 1, 2, 0]
    n_per = [pattern[i % len(pattern)] for i in range(Hd * Wd)]
    sc = scene(n_per, Hd, Wd, seed=1)
    nt = sc["tgt"].shape[0]
    rows = window_rows(sc)
    assert nt % 16 != 0
    assert {lo % 16 for lo, hi in rows if hi > lo} == set(range(16)) and {hi % 16 for lo, hi in rows if hi > lo} == set(range(16))
    assert any(lo == 0 and hi > 0 for lo, hi in rows) and any(hi == nt and hi > lo for lo, hi in rows)
    check(gs, sc)


@pytest.mark.parametrize("per_tile", [3, 20])
def test_rows_longer_than_a_chunk(gs, per_tile):
    """20 and 40 targets per pixel: a row of three pixels is 80 - 100 slots whose ends fall inside chunks -- interior chunks are
    covered, edge chunks are not.  Three lanes per tile off the wall: the point-serial search; twenty: the tile-level search."""
    Hd, Wd = 10, 16
    n_per = [20 if (i + i // Wd) % 2 == 0 else 40 for i in range(Hd * Wd)]
    sc = scene(n_per, Hd, Wd, seed=2)
    rows = window_rows(sc)
    assert all(hi - lo > 16 for lo, hi in rows) and any(lo % 16 for lo, hi in rows) and any(hi % 16 for lo, hi in rows)
    check(gs, off_the_wall(sc, per_tile))


def test_empty_rows_and_empty_windows(gs):
    """At most one target per pixel, three whole pixel rows empty: windows with one or two empty rows, and (the middle one of the
    three) source pixels whose nine pixels hold nothing at all."""
    Hd, Wd = 12, 24
    g = torch.Generator().manual_seed(3)
    n_per = torch.randint(0, 2, (Hd * Wd,), generator=g)
    n_per[4 * Wd: 7 * Wd] = 0
    sc = scene(n_per, Hd, Wd, seed=3)
    rows = window_rows(sc)
    assert sum(1 for lo, hi in rows if hi == lo) >= 3 * Wd
    check(gs, sc)


def test_borders_and_narrow_grid(gs):
    """Wd = 24: a tile spans three pixel rows; every pixel carries a source point, so the first and last column (where g +- 1 wraps
    into the neighbouring row) and the first and last row are window centres; 33 points per tile; a motion of a third of a pixel."""
    Hd, Wd = 12, 24
    g = torch.Generator().manual_seed(4)
    sc = scene(torch.randint(0, 7, (Hd * Wd,), generator=g), Hd, Wd, seed=4, motion=0.03)
    cols, rws = sc["src_pix"].long() % Wd, sc["src_pix"].long() // Wd
    assert {0, Wd - 1} <= set(cols.tolist()) and {0, Hd - 1} <= set(rws.tolist())
    check(gs, off_the_wall(sc, 2, 33), tile_points=33)


def test_band_the_pool_cannot_hold(gs):
    """70 targets per pixel on a 4 x 64 grid: one row band of a tile (66 pixels) is 4620 points, more than the 4096 the LDS pool
    holds, so the scan reads its candidates from memory."""
    Hd, Wd = 4, 64
    sc = scene([70] * (Hd * Wd), Hd, Wd, seed=5)
    assert 66 * 70 > 4096
    check(gs, off_the_wall(sc, 3))


def test_duplicates_across_a_chunk_boundary(gs):
    """Two exact copies of one target in the same pixel, in the scan slots 16 k - 1 and 16 k -- either side of a chunk boundary --
    put where the pixel's source point lies, so that they are its nearest neighbours: the lower reference index must win,
    whichever of the two slots holds it."""
    Hd, Wd = 12, 24
    g = torch.Generator().manual_seed(6)
    sc = scene(torch.randint(2, 6, (Hd * Wd,), generator=g), Hd, Wd, seed=6, motion=0.0005)
    order, ps, tgt = sc["order"], sc["pix_start"].long(), sc["tgt"]
    pix_of_src = {int(p): i for i, p in enumerate(sc["src_pix"].tolist())}
    dup, lower_first = [], 0
    for b in range(16, tgt.shape[0], 16):
        pix = int(torch.searchsorted(ps, torch.tensor(b), right=True)) - 1
        if ps[pix] <= b - 1 and b < ps[pix + 1]:  # slots b - 1 and b lie in the same pixel
            if len(dup) % 2:  # (scan order inside a pixel is ascending reference index: every other pair the other way round)
                order[[b - 1, b]] = order[[b, b - 1]]
            i, j = int(order[b - 1]), int(order[b])
            tgt[i] = tgt[j] = sc["src"][pix_of_src[pix]] + torch.tensor([0.0, 0.0, 0.0005])
            dup.append(min(i, j))
            lower_first += i < j
    assert len(dup) >= 20 and 0 < lower_first < len(dup)  # both orders occur
    want = check(gs, sc)
    first = next(iter(want.values()))  # (any launch: the duplicates stay the nearest of their source points)
    found = set((first & 0xffffffff).tolist())
    assert len(found & set(dup)) >= len(dup) // 2, (len(found & set(dup)), len(dup))
