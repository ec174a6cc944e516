"""The grid search's SECOND window (csrc/gs_icp_loop.hpp knn_second_window): a lane whose first window -- centred on the pixel its
point projected to in the previous launch -- carried no proof examines the 3 x 3 to 7 x 7 pixels around the pixel it projects to
NOW, and only then takes the exact chunk-box search.  Whatever path a lane takes, every association launch of a loop must return
the brute-force scan's packed (distance, index) keys bit for bit, and the pose must be the chunk-box search's: scene(...) and
check(...) of tests/test_exact_window_scan.py, unmodified (taped six-iteration loops, eight and sixteen waves, LM and gradLM, grid
search against chunk-box search).

The scenes are built so that the path is taken by GEOMETRY, on any build: target and source are put on the plane z = 2 (every
point scaled along its own ray: it keeps its pixel) and the source is rotated about a camera axis by 1.5 ds-cells.  Point-to-plane
on a plane recovers a rotation about an in-plane axis in one Gauss-Newton step (damping 1e-8), so the step folded into the second
launch moves every point that far back, to the next cell -- where the first window's bound (0.87 cells, 9 cm) is too small for a target
on every other pixel row only (sparse).  The second window is taken by tiles with more than six lanes in need, in the eight-wave form of the kernel (the sixteen-wave
form, which dense targets run, goes straight to the exact search: its results are checked all the same).  Each test restates cam_cell in torch and asserts from the taped clouds that the intended
share of lanes changes cell.  gs_window_counts then shows what the device did."""
import ctypes
import math

import pytest
import torch

from tests.test_exact_window_scan import check, on_device, scene

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import gradslam_amd

    return gradslam_amd


def flatten(sc, seed, rough=0.001):
    """Target and source onto the plane z = 2, each point moved along its ray: same pixel.  2 mm of depth noise on the target,
    `rough` on the source."""
    g = torch.Generator().manual_seed(seed)
    for k, jit in (("tgt", 0.002), ("src", rough)):
        p = sc[k]
        z = 2.0 + jit * torch.randn(p.shape[0], generator=g)
        sc[k] = (p * (z / p[:, 2]).unsqueeze(1)).contiguous()
    return sc


def rotate(sc, axis, cells):
    """The source rotated about the camera's y (axis 0: the image moves sideways) or x axis (1: it moves down) by `cells` ds-cells
    at the image centre."""
    f = float(sc["cam_K"][axis, axis])
    a = cells * sc["ds"] / f
    c, s = math.cos(a), math.sin(a)
    R = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]] if axis == 0 else [[1, 0, 0], [0, c, s], [0, -s, c]], dtype=torch.float32)
    sc["src"] = (sc["src"] @ R.t()).contiguous()
    return sc


def cam_cell(sc, cloud):
    """csrc/gs_icp_loop.hpp cam_cell for the scenes' camera (identity pose): the ds-grid pixel nearest to a point's projection."""
    K, ds, Wd, Hd = sc["cam_K"], sc["ds"], sc["Wd"], sc["Hd"]
    p = cloud.cpu()
    u = ((K[0, 0] * p[:, 0] + K[0, 2] * p[:, 2]) / p[:, 2]) / ds
    v = ((K[1, 1] * p[:, 1] + K[1, 2] * p[:, 2]) / p[:, 2]) / ds
    return torch.round(v).clamp(0, Hd - 1).long() * Wd + torch.round(u).clamp(0, Wd - 1).long()


def taped_clouds(gs, sc):
    """The clouds of the six-iteration LM loop's seven association launches (grid search, default wave count)."""
    from tests import test_gpu_parity as P

    lib = gs._native.lib()
    lib.gs_set_grid_search(2)
    try:
        _, assoc = P._taped_loop_with_hints(gs, on_device(sc), 6, 0)
    finally:
        lib.gs_set_grid_search(1)
    return [cloud.clone() for cloud, _ in assoc]


def run(gs, sc, tile_points=0):
    """check(...) with the second window's counters around it: {blocks that took it, lanes proven, lanes handed on, refusals}."""
    lib = gs._native.lib()
    counts = (ctypes.c_uint * 4)()
    assert lib.gs_window_counts(counts, 1) == 0
    want = check(gs, sc, tile_points)
    assert lib.gs_window_counts(counts, 1) == 0
    print("second window: blocks %d, lanes proven %d, handed on %d, blocks refused %d" % tuple(counts))
    return list(counts), want


def moved_share(sc, clouds, a=0, b=1):
    ca, cb = cam_cell(sc, clouds[a]), cam_cell(sc, clouds[b])
    return (ca != cb).float().mean().item(), ca, cb


def first_window_len(sc, p):
    """Slots of the 3 x 3 window around pixel p, as the kernel clamps its rows (tests/test_exact_window_scan.window_rows)."""
    Wd, nc, ps = sc["Wd"], sc["Wd"] * sc["Hd"], sc["pix_start"].long()
    n = 0
    for r in (-1, 0, 1):
        g = p + r * Wd
        if g + 1 >= 0 and g - 1 <= nc - 1:
            n += int(ps[min(max(g + 1, 0), nc - 1) + 1]) - int(ps[min(max(g - 1, 0), nc - 1)])
    return n


def sparse(Hd, Wd):
    """One target per pixel on every other pixel row: a source point on a row without targets has its neighbour one cell (10 cm)
    away.  A window centred on the point's own cell proves that (its bound is 1.87 cells: the nearest target outside it projects
    at least 2 ds - 0.5 image pixels from the centre); a window centred one cell off leaves 0.87 cells, 9 cm, and does not."""
    return [1 if (i // Wd) % 2 == 0 else 0 for i in range(Hd * Wd)]


def test_sideways_move(gs):
    """The whole cloud starts 1.5 cells sideways of a target that covers every third pixel column: the first step moves 92 % of
    the lanes to the next cell of their row, and the two lanes in three without a target on their own column have their
    neighbour 1 to 1.5 cells away -- beyond the 0.87 cells the first window proves one cell from its centre.  Wd = 24: a tile
    spans three rows, row ranges run on across row ends.  Tiles of the second launch take the second window in place of the
    tile-level search, and it proves most of their lanes.  (That NO tile goes on to the tile-level search cannot be read from
    the counters' four slots; what is asserted is that at most six lanes per block on the path are handed on, on average --
    the point-serial search's share.  One target per pixel, every other column, a checkerboard and a rough source were
    measured too: at most three lanes of a tile lose their first proof there, and no tile takes the path.)"""
    Hd, Wd = 16, 24
    n_per = [1 if (i % Wd) % 3 == 0 else 0 for i in range(Hd * Wd)]
    sc = rotate(flatten(scene(n_per, Hd, Wd, seed=11, motion=0.0), 11), 0, 1.5)
    share, ca, cb = moved_share(sc, taped_clouds(gs, sc))
    same_row = ((ca // Wd) == (cb // Wd)).float().mean().item()
    print("lanes that change cell between launch 1 and 2: %.3f, that stay in their row: %.3f" % (share, same_row))
    assert share >= 0.9 and same_row >= 0.99
    counts, _ = run(gs, sc)
    assert counts[0] >= 2 * (Hd * Wd // 64) and counts[3] == 0, counts  # two eight-wave grid-search loops, every tile of launch 2
    assert counts[1] >= 5 * counts[2], counts                           # proven: by far the most
    assert counts[2] <= 6 * counts[0], counts


def test_move_down_a_row(gs):
    """The cloud starts 1.5 cells up: the centre changes ROW.  Wd = 40: a 64-lane tile spans a row end (two-row tiles)."""
    Hd, Wd = 30, 40
    sc = rotate(flatten(scene(sparse(Hd, Wd), Hd, Wd, seed=12, motion=0.0), 12), 1, 1.5)
    share, ca, cb = moved_share(sc, taped_clouds(gs, sc))
    rows = ((ca // Wd) != (cb // Wd)).float().mean().item()
    print("lanes that change cell between launch 1 and 2: %.3f, that change row: %.3f" % (share, rows))
    assert share >= 0.9 and rows >= 0.9
    counts, _ = run(gs, sc)
    assert counts[0] > 0 and counts[3] == 0, counts
    assert counts[1] >= 2 * 0.2 * Hd * Wd, counts
    assert counts[2] * 10 <= counts[1], counts


def test_uncovered_strip(gs):
    """The target ends six pixel rows above the grid's last row; the source covers every row.  A lane k rows below the target's
    last row has its neighbour k cells away: an empty first window from k = 2 on (the key is the seed's), a second window of
    radius 2 and 3 for k = 2 and 3, and no window within radius 3 beyond -- those lanes are handed on.
    This is also the scene for "no candidate at all in the first window".  A live lane whose KEY is none cannot occur in the grid
    search: before the scan wave 0 folds a seed -- a real target: the previous launch's neighbour, or in the first launch the next
    target in pixel order -- into every live lane's key whenever the target is not empty (knn1_loop_k), so knn_second_window's
    `bd0 < INFINITY` only guards lanes that are not live.  What does occur is the empty first WINDOW asserted below: its lanes
    carry the seed's key alone, and whether they get a second window depends on how far that seed is."""
    Hd, Wd = 20, 24
    n_per = torch.ones(Hd * Wd, dtype=torch.int64)
    n_per[(Hd - 6) * Wd:] = 0
    sc = flatten(scene(n_per, Hd, Wd, seed=13, motion=0.002), 13)
    clouds = taped_clouds(gs, sc)
    counts, want = run(gs, sc)
    rows_away = {}
    for cloud in clouds:
        keys = want[cloud.cpu().numpy().tobytes()]
        nn_row = sc["tgt_pix"].long()[(keys.cpu() & 0xffffffff)] // Wd
        for k in (cam_cell(sc, cloud) // Wd - nn_row).tolist():
            rows_away[k] = rows_away.get(k, 0) + 1
    print("lanes by rows between their cell and their neighbour's:", dict(sorted(rows_away.items())))
    assert rows_away.get(2, 0) >= Wd // 2 and rows_away.get(3, 0) >= Wd // 2 and sum(v for k, v in rows_away.items() if k >= 4) >= Wd
    ps = sc["pix_start"].long()
    empty = [p for p in range((Hd - 4) * Wd, Hd * Wd) if first_window_len(sc, p) == 0]  # (two rows and more below the target)
    assert len(empty) == 4 * Wd and int(ps[-1]) > 0
    assert counts[0] > 0 and counts[3] == 0
    assert counts[1] >= rows_away.get(2, 0) + rows_away.get(3, 0), counts  # radius 2 and 3 proved their lanes (two eight-wave loops)
    assert counts[2] >= 2 * Wd, counts                                      # beyond radius 3: handed on


def test_borders_corners_and_narrow_grid(gs):
    """Wd = 6 (< 8), every pixel a source point 20 cm (one sigma) off the plane and no motion: in every launch about half the
    lanes of every tile -- border pixels included, a 64-lane tile spans eleven rows -- have their neighbour beyond the first
    window's 19 cm and take a second window of radius 2 or 3 that hangs over the grid's borders.  The four corner pixels' points
    are put 30 cm off the plane: each corner is such a lane."""
    Hd, Wd = 16, 6
    sc = flatten(scene([1] * (Hd * Wd), Hd, Wd, seed=14, motion=0.0), 14, rough=0.2)
    corners = [0, Wd - 1, (Hd - 1) * Wd, Hd * Wd - 1]
    for i in corners:
        sc["src"][i] = sc["src"][i] * (2.3 / sc["src"][i, 2])
    clouds = taped_clouds(gs, sc)
    cells = cam_cell(sc, clouds[0])  # (the first launch: the source as given, every window centred on its point's own cell)
    assert torch.equal(cells, sc["src_pix"].long())
    off = (clouds[0][:, 2].cpu() - 2.0).abs()
    far = cells[off > 0.2]  # (certainly in need: 1.87 cells, 19 cm, is the first window's bound at its best)
    assert min(int((off[t:t + 64] > 0.2).sum()) for t in range(0, off.shape[0], 64)) > 6
    assert {0, Wd - 1} <= set((far % Wd).tolist()) and {0, Hd - 1} <= set((far // Wd).tolist())
    assert set(corners) <= set(far.tolist())
    counts, _ = run(gs, sc)
    assert counts[0] > 0 and counts[1] > 0 and counts[3] == 0, counts


def test_33_point_tiles(gs):
    """tile_points = 33 on a 24 x 16 grid moved sideways and down, source 25 cm (one sigma) off the plane: tiles start anywhere in
    a row, and tiles with more than six points beyond the first window's 19 cm exist in the second launch."""
    Hd, Wd = 16, 24
    sc = rotate(rotate(flatten(scene([1] * (Hd * Wd), Hd, Wd, seed=15, motion=0.0), 15, rough=0.25), 0, -1.5), 1, 1.5)
    clouds = taped_clouds(gs, sc)
    far = (clouds[1][:, 2].cpu() - 2.0).abs() > 0.2
    assert max(int(far[t:t + 33].sum()) for t in range(0, far.shape[0], 33)) > 6
    counts, _ = run(gs, sc, tile_points=33)
    assert counts[0] > 0 and counts[1] > 0 and counts[3] == 0, counts


def test_dense_target_is_refused(gs):
    """Ten targets per pixel, source 20 cm off the plane: every tile has more than six lanes in need in every launch, a first
    window holds ~90 slots and a re-centred one as many -- above the cap of 64.  Every such block is refused before it asks for
    anything and takes the exact search as before; same results."""
    Hd, Wd = 16, 24
    sc = flatten(scene([10] * (Hd * Wd), Hd, Wd, seed=16, motion=0.002), 16, rough=0.2)
    for t in range(0, Hd * Wd, 64):  # the longest first window of every tile is above the cap
        assert max(first_window_len(sc, int(p)) for p in sc["src_pix"][t:t + 64]) > 64
    clouds = taped_clouds(gs, sc)
    far = (clouds[1][:, 2].cpu() - 2.0).abs() > 0.2
    assert min(int(far[t:t + 64].sum()) for t in range(0, far.shape[0], 64)) > 6
    counts, _ = run(gs, sc)
    assert counts[3] >= 2 * 7 * (Hd * Wd // 64) and counts[0] == 0 and counts[1] == 0, counts  # eight-wave loops, every tile and launch


def test_equal_distances_across_a_window_edge(gs):
    """Two targets at EXACTLY the same fp32 distance from a source point, 2.5 cells to either side of it (pairs along a row, pairs
    along a column), the point itself 0.45 cells off its cell's centre -- so one target sits on pixel c' - 2, inside the radius-2
    window around the point's cell c', and the other on c' + 3, outside it -- and no other target within 3.4 cells.  The lower
    reference index must win, whichever side holds it (both orders are built).  An equal-distance candidate outside the window
    that PROVES cannot exist (its bound exceeds the best), so the edge the pair straddles is radius 2's: that window's bound
    (2.42 cells on the near side) does not exceed the best, radius 3's (3.42) does, and the radius-3 window must find both.
    Distances are exact because nothing is rounded: the first launch sees the source as given (identity), and point, offset and
    depth are multiples of 2^-10.  The first window is empty there and the key is the seed's (the next target in pixel order:
    the pair's far member, or a target three cells along the row), so every lane of the cleared blocks is in need."""
    Hd, Wd, ds = 30, 40, 4
    centres = [(r, c) for r in (5, 14, 23) for c in (6, 17, 28)]
    n_per = torch.ones(Hd * Wd, dtype=torch.int64)
    for r, c in centres:
        for rr in range(r - 3, r + 4):
            n_per[rr * Wd + c - 4: rr * Wd + c + 5] = 0
    pairs = []
    for k, (r, c) in enumerate(centres):
        a, b = ((r, c - 2), (r, c + 3)) if k % 2 == 0 else ((r - 2, c), (r + 3, c))
        n_per[a[0] * Wd + a[1]] = n_per[b[0] * Wd + b[1]] = 1
        if k % 2:
            n_per[r * Wd + c + 3] = 1  # the seed of a column pair's point: three cells along its row
        pairs.append((r * Wd + c, a[0] * Wd + a[1], b[0] * Wd + b[1], k % 2))
    sc = flatten(scene(n_per, Hd, Wd, seed=17, motion=0.0), 17)
    fx, cx, cy = float(sc["cam_K"][0, 0]), float(sc["cam_K"][0, 2]), float(sc["cam_K"][1, 2])
    q = lambda x: round(x * 1024.0) / 1024.0
    A = q(2.5 * ds * 2.0 / fx)
    ps, order, tgt, tgt_pix = sc["pix_start"].long(), sc["order"], sc["tgt"], sc["tgt_pix"]
    lower_inside = 0
    want_nn = {}
    for k, (i, pa, pb, vertical) in enumerate(pairs):
        r, c = i // Wd, i % Wd
        u, v = c * ds + (0.0 if vertical else 0.45 * ds), r * ds + (0.45 * ds if vertical else 0.0)
        s = torch.tensor([q((u - cx) * 2.0 / fx), q((v - cy) * 2.0 / fx), 2.0])
        sc["src"][i] = s
        sa, sb = int(ps[pa]), int(ps[pb])
        ia, ib = int(order[sa]), int(order[sb])
        if (ia < ib) != (k % 4 < 2):  # both orders: the inside target holds the lower reference index in every other pair of pairs
            order[sa], order[sb] = ib, ia
            tgt_pix[ia], tgt_pix[ib] = pb, pa
            ia, ib = ib, ia
        d = torch.tensor([0.0, A, 0.0]) if vertical else torch.tensor([A, 0.0, 0.0])
        tgt[ia], tgt[ib] = s - d, s + d
        lower_inside += ia < ib
        want_nn[i] = min(ia, ib)
        da, db = [((s[0] - t[0]) ** 2 + (s[1] - t[1]) ** 2) + (s[2] - t[2]) ** 2 for t in (tgt[ia], tgt[ib])]
        assert da == db and float(da) == A * A  # exactly equal in fp32, as the kernel computes them
        others = torch.ones(tgt.shape[0], dtype=torch.bool)
        others[[ia, ib]] = False
        assert float(((tgt[others] - s) ** 2).sum(1).min()) > (2.7 * ds * 2.0 / fx) ** 2  # nothing else as near
    assert 0 < lower_inside < len(pairs)
    # the pair's pixels, from the projection: c' - 2 / c' + 3 (rows: r' - 2 / r' + 3)
    cells = cam_cell(sc, tgt)
    assert torch.equal(cells, tgt_pix.long())
    clouds = taped_clouds(gs, sc)
    assert torch.equal(clouds[0].cpu(), sc["src"])  # the first launch sees the source as given
    counts, want = run(gs, sc)
    first = want[clouds[0].cpu().numpy().tobytes()].cpu()
    for i, j in want_nn.items():
        assert int(first[i] & 0xffffffff) == j, (i, int(first[i] & 0xffffffff), j)
    assert counts[0] > 0 and counts[1] >= 2 * len(pairs) and counts[3] == 0, counts
