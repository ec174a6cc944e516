"""The one-call map updates (ops.pointfusion_update_raw, ops.aggregate_update_raw) and the stream compaction under them,
called directly on inputs engineered so that every decision is unambiguous.

The frame is a 6 x 8 plane at depth 2 with f = 4, cx = 3, cy = 2 and two holes; map points are dyadic rationals on (or a
power of two beside) pixel rays.  Projections are then exact (u = w z / z), and every threshold (distance, normal dot
product, image border, half pixel) is exercised along an axis where the frame's own value is exact: z = 2 for the
distance, (0, 0, 1) for the normal.  The frame's x and y are NOT the dyadic (w - 3) / 2, (h - 2) / 2: the reference
inverts the intrinsics with 1 / (f + 1e-6), which puts them some 2e-7 off.  That offset is far below every margin used
here (the next candidate differs by 2^-22 at the least along z, by 1 / 64^2 in squared distance elsewhere), and at the
centre pixel (h = 2, w = 3) it is exactly zero, which is where the two distance-threshold rows sit.  test_engineered_
inputs_are_unambiguous (CPU only) is the proof: the float32 oracle and the same oracle in float64 produce identical
active, similar and unique tables and identical appended pixel lists, and every hand-placed row meets the fate its name
states.  The GPU tests then allow no flips at all.

Edges reached (by row name in _HAND): image border at +-2^-10 / 2^-9 in u and v, half pixels (round half to even), z = 0,
z < 0 with an in-frame projection, dist == th and one ulp below, dot == th and one ulp above, a dot product > 1, three
bit-equal keys held by two items of one thread and another workgroup (twice: smallest index in the first block, and in
the block next to the partial last one), confidence before distance, c == 0 rows, a map point over a hole, a rotation
that is not symmetric with a non-zero inverse translation (b = 1), very different counts per batch element with a
partial last block, no correspondence anywhere, a correspondence in one batch element only, the capacity clamp.
"""
import ctypes
import functools
import math
import warnings

import pytest
import torch

from tests.helpers import rel_err

DEV = "cuda:0"

H, W, B = 6, 8, 2
COUNTS = (2077, 5)            # three 1024-row blocks for b = 0 (the last one partial), one nearly empty for b = 1
NMAX = 2200
DIST_TH = 0.0625
DOT_TH = float(torch.tensor(math.cos(math.radians(20.0)), dtype=torch.float32))
SIGMA = 1.5
HOLES = ((1, 5), (4, 1))
ULP2 = 2.0 ** -22             # one float32 ulp of a coordinate in [2, 4)
VARIANTS = ("main", "none", "b1_only")

# b = 1: 90 degrees about the camera's y axis and a dyadic translation: R is not symmetric, -R^T t is not zero
R1 = ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0))
T1 = (0.5, -0.25, 0.5)


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ---------------------------------------------------------------------------------------------- the engineered inputs
def _ray(h, w, z):
    """The point of pixel (h, w)'s ray at depth z (exact for the dyadic z used here)."""
    return ((w - 3) * z / 4.0, (h - 2) * z / 4.0, z)


def _uv(u, v, z=2.0):
    """The camera-frame point that projects to (u, v) at depth z."""
    return ((u - 3.0) * z / 4.0, (v - 2.0) * z / 4.0, z)


E10, E9 = 2.0 ** -10, 2.0 ** -9
NUP = (0.0, 0.0, 1.0)
DOT_ABOVE = float(torch.nextafter(torch.tensor(DOT_TH, dtype=torch.float32), torch.tensor(2.0)))

# name -> (row index, camera-frame point, normal, confidence count).  The fates are asserted by name in
# test_engineered_inputs_are_unambiguous.
_HAND = {
    # image border (reference: u > -1e-3, u < W - 0.999, likewise v) and rounding to the pixel
    "u_lo_in": (100, _uv(-E10, 2), NUP, 1.0), "u_lo_out": (101, _uv(-E9, 2), NUP, 3.0),
    "u_hi_in": (102, _uv(7 + E10, 2), NUP, 1.0), "u_hi_out": (103, _uv(7 + E9, 2), NUP, 3.0),
    "v_lo_in": (1100, _uv(3, -E10), NUP, 1.0), "v_lo_out": (1101, _uv(3, -E9), NUP, 3.0),
    "v_hi_in": (2060, _uv(3, 5 + E10), NUP, 1.0), "v_hi_out": (2061, _uv(3, 5 + E9), NUP, 3.0),
    "half_2p5": (300, _uv(2.5, 3), NUP, 3.0), "half_3p5": (301, _uv(3.5, 3), NUP, 3.0),
    "z_zero": (302, (0.5, 0.5, 0.0), NUP, 3.0), "z_neg": (303, (0.5, 0.5, -2.0), NUP, 3.0),
    # thresholds, at the centre pixel for the distance (the frame's vertex there is (0, 0, 2) exactly)
    "dist_eq": (500, (0.0, 0.0, 2.0625), NUP, 3.0), "dist_below": (501, (0.0, 0.0, 2.0625 - ULP2), NUP, 1.0),
    "dot_eq": (502, _ray(1, 1, 2.0), (0.0, 0.0, DOT_TH), 3.0), "dot_above": (503, _ray(1, 2, 2.0), (0.0, 0.0, DOT_ABOVE), 1.0),
    "dot_big": (504, _ray(1, 3, 2.0), (0.0, 0.0, 1.25), 1.0),
    # three bit-equal keys on one pixel: items 0 and 1 of one thread of block 0, and block 1
    "tieA_0": (10, _ray(3, 5, 2 + 2.0 ** -5), NUP, 1.0), "tieA_1": (266, _ray(3, 5, 2 - 2.0 ** -5), NUP, 1.0),
    "tieA_2": (1037, _ray(3, 5, 2 + 2.0 ** -5), NUP, 1.0),
    # the same with the smallest index in block 1, the neighbour of the partial last block, which holds the third
    "tieB_0": (1030, _ray(3, 6, 2 - 2.0 ** -5), NUP, 1.0), "tieB_1": (1286, _ray(3, 6, 2 + 2.0 ** -5), NUP, 1.0),
    "tieB_2": (2050, _ray(3, 6, 2 - 2.0 ** -5), NUP, 1.0),
    # key order: confidence first, then ray distance; the loser always has the smaller index
    "c1_near": (700, _ray(4, 3, 2.0), NUP, 1.0), "c3_far": (701, _ray(4, 3, 2 + 2.0 ** -5), NUP, 3.0),
    "c0_near": (710, _ray(4, 4, 2.0), NUP, 0.0), "chalf_far": (711, _ray(4, 4, 2 + 2.0 ** -5), NUP, 0.5),
    "c0_far": (720, _ray(4, 5, 2 + 2.0 ** -5), NUP, 0.0), "c0_nearer": (721, _ray(4, 5, 2 + 2.0 ** -6), NUP, 0.0),
    # a map point over a hole of the frame
    "over_hole": (800, _ray(1, 5, 2.0), NUP, 1.0),
}
# (the tie rows' x and y are their rays' at THEIR depth: the three rows of a group must share x and y for bit-equal
# keys, so they are re-placed on the pixel's z = 2 ray point below)
_TIE_PIX = {"tieA": (3, 5), "tieB": (3, 6)}
# pixels that belong to the hand-placed rows, and a few that get no map point at all (they are appended, and give
# the capacity clamp enough unmatched pixels); the lattice fill stays off both
_RESERVED = {(2, 0), (2, 7), (0, 3), (5, 3), (3, 2), (3, 4), (2, 3), (1, 1), (1, 2), (1, 3), (3, 5), (3, 6), (4, 3), (4, 4),
             (4, 5)}
_EMPTY = {(0, 0), (0, 7), (5, 0), (5, 7), (0, 1), (5, 6)}
# b = 1 (five rows, camera-frame constructions pushed through the pose): name -> (row, point, normal, count)
_HAND1 = {
    "dist_below": (0, (0.0, 0.0, 2.0625 - ULP2), NUP, 1.0), "dist_eq": (1, (0.0, 0.0, 2.0625), NUP, 3.0),
    "u_lo_in": (2, _uv(-E10, 2), NUP, 2.0), "u_lo_out": (3, _uv(-E9, 2), NUP, 3.0),
    "plain": (4, _ray(3, 5, 2 + 2.0 ** -5), NUP, 2.0),
}
_EXPECT_PIXEL = {"u_lo_in": (2, 0), "u_hi_in": (2, 7), "v_lo_in": (0, 3), "v_hi_in": (5, 3), "half_2p5": (3, 2), "half_3p5": (3, 4),
                 "dist_eq": (2, 3), "dist_below": (2, 3), "dot_eq": (1, 1), "dot_above": (1, 2), "dot_big": (1, 3),
                 "over_hole": (1, 5), "c1_near": (4, 3), "c3_far": (4, 3), "c0_near": (4, 4), "chalf_far": (4, 4),
                 "c0_far": (4, 5), "c0_nearer": (4, 5), "tieA_0": (3, 5), "tieA_1": (3, 5), "tieA_2": (3, 5),
                 "tieB_0": (3, 6), "tieB_1": (3, 6), "tieB_2": (3, 6)}
_INACTIVE = ("u_lo_out", "u_hi_out", "v_lo_out", "v_hi_out", "z_zero", "z_neg")
_NOT_SIMILAR = ("half_2p5", "half_3p5", "dist_eq", "dot_eq", "over_hole")
_WINNERS = ("u_lo_in", "u_hi_in", "v_lo_in", "v_hi_in", "dist_below", "dot_above", "dot_big", "tieA_0", "tieB_0", "c3_far",
            "chalf_far", "c0_nearer")
_LOSERS = ("tieA_1", "tieA_2", "tieB_1", "tieB_2", "c1_near", "c0_near", "c0_far")


def _to_world(p, b):
    if b == 0:
        return p
    return tuple(sum(R1[i][j] * p[j] for j in range(3)) + T1[i] for i in range(3))


def _rot(n, b):
    return n if b == 0 else tuple(sum(R1[i][j] * n[j] for j in range(3)) for i in range(3))


@functools.lru_cache(maxsize=None)
def _case(variant):
    """Everything as float32 CPU tensors: depth (B,1,H,W,1), rgb (B,1,H,W,3), K, pose (B,1,4,4) and the map as four
    per-element lists.  variant: "main"; "none" = the whole map moved 1.0 away along the camera's z (no point is similar
    to anything); "b1_only" = only b = 0's map moved."""
    g = torch.Generator().manual_seed(20260)
    depth = torch.full((B, 1, H, W, 1), 2.0)
    for h, w in HOLES:
        depth[:, :, h, w] = 0.0
    # colours take part in no decision: full-mantissa values, so that (c * x + 0) * (1 / c) is visibly not the identity
    rgb = torch.rand((B, 1, H, W, 3), generator=g)
    K = torch.eye(4).view(1, 1, 4, 4).repeat(B, 1, 1, 1)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2] = 4.0, 4.0, 3.0, 2.0
    pose = torch.eye(4).view(1, 1, 4, 4).repeat(B, 1, 1, 1)
    pose[1, 0, :3, :3] = torch.tensor(R1)
    pose[1, 0, :3, 3] = torch.tensor(T1)

    free = [(h, w) for h in range(H) for w in range(W) if (h, w) not in _RESERVED | _EMPTY | set(HOLES)]
    normals = ((0.0, 0.0, 1.0), (0.0, 0.25, 0.96875), (0.0, 0.5, 0.75))
    cvals = (0.0, 0.5, 1.0, 2.0, 3.0)
    rows = []  # b = 0, camera frame: (point, normal, count)
    ri = lambda n: int(torch.randint(0, n, (1,), generator=g))
    for _ in range(COUNTS[0]):
        h, w = free[ri(len(free))]
        rows.append((_ray(h, w, 2.0 + (ri(11) - 5) / 64.0), normals[ri(3)], cvals[ri(5)]))
    for name, (n, p, nrm, c) in _HAND.items():
        if name[:4] in _TIE_PIX:  # x, y of the pixel's z = 2 ray point, z as stated
            x, y, _ = _ray(*_TIE_PIX[name[:4]], 2.0)
            p = (x, y, p[2])
        rows[n] = (p, nrm, c)
    # a few c = 3 rows behind the camera with full-mantissa coordinates: live, never active, re-rounded by the merge
    behind = torch.rand((8, 6), generator=g)
    for i in range(8):
        x = behind[i].tolist()
        rows[900 + i] = ((x[0], x[1], -1.0 - x[2]), (x[3], x[4], x[5]), 3.0)
    rows1 = [None] * COUNTS[1]
    for name, (n, p, nrm, c) in _HAND1.items():
        rows1[n] = (p, nrm, c)

    shift = {"main": (0.0, 0.0), "none": (1.0, 1.0), "b1_only": (1.0, 0.0)}[variant]
    pts, nrms, cols, ccs = [], [], [], []
    for b, rs in enumerate((rows, rows1)):
        P = torch.tensor([_to_world((p[0], p[1], p[2] + shift[b]), b) for p, _, _ in rs], dtype=torch.float32)
        Nn = torch.tensor([_rot(n, b) for _, n, _ in rs], dtype=torch.float32)
        C = torch.tensor([[c] for _, _, c in rs], dtype=torch.float32)
        pts.append(P); nrms.append(Nn); ccs.append(C)
        cols.append(torch.rand((len(rs), 3), generator=g))
    # every coordinate that takes part in a decision was stated exactly: the float32 tensors hold what was written
    assert all(tuple(pts[0][n].double().tolist()) == (rows[n][0][0], rows[n][0][1], rows[n][0][2] + shift[0]) for n in (100, 101, 500, 501, 10, 2050))
    assert float(pts[1][0, 0].double()) == 2.0625 - ULP2 + 0.5 + shift[1]
    return dict(depth=depth, rgb=rgb, K=K, pose=pose, points=pts, normals=nrms, colors=cols, feats=ccs)


@functools.lru_cache(maxsize=None)
def _oracle(variant, dtype):
    """The reference restatement on the engineered inputs, in float32 or float64: frame, the three tables, the updated
    map, the appended pixel lists and the map after update_map_aggregate.  Computed once per (variant, dtype)."""
    from oracle import fusion
    from oracle.cloud import Cloud

    c = _case(variant)
    cv = lambda xs: [x.to(dtype) for x in xs]
    fr = fusion.make_frame(c["rgb"].to(dtype), c["depth"].to(dtype), c["K"].to(dtype), c["pose"].to(dtype))
    cloud = Cloud(cv(c["points"]), cv(c["normals"]), cv(c["colors"]), cv(c["feats"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "dot product > 1" (dot_big asks for it), "no similar points" (variant none)
        active = fusion.find_active_map_points(cloud, fr)
        similar, _ = fusion.find_similar_map_points(cloud, fr, active, DIST_TH, DOT_TH)
        unique = fusion.find_best_unique_correspondences(cloud, fr, similar)
        out = fusion.fuse_with_map(cloud, fr, unique, SIGMA)
        agg = fusion.update_map_aggregate(Cloud(cv(c["points"]), cv(c["normals"]), cv(c["colors"])), fr)
        dots = (torch.zeros_like(cloud.padded("normals")))
        if active.shape[0]:
            b, n, h, w = active.unbind(1)
            dots[b, n] = fr["gN"][b, 0, h, w]
        max_dot = float((dots * cloud.padded("normals")).sum(-1).max())
    valid = (c["depth"] > 0)[:, 0, :, :, 0]
    appended = []
    for b in range(B):
        taken = {(int(r[2]), int(r[3])) for r in unique if int(r[0]) == b}
        appended.append([(h, w) for h in range(H) for w in range(W) if bool(valid[b, h, w]) and (h, w) not in taken])
    return dict(fr=fr, active=active, similar=similar, unique=unique, out=out, agg=agg, appended=appended, max_dot=max_dot)


def _fates(o, b=0):
    """row -> pixel for the active rows of batch element b, and the sets of similar and winning rows."""
    pick = lambda t: {int(r[1]): (int(r[2]), int(r[3])) for r in t if int(r[0]) == b}
    return pick(o["active"]), set(pick(o["similar"])), set(pick(o["unique"]))


# ---------------------------------------------------------------------------------------------- 1. CPU self-check
@pytest.mark.parametrize("variant", VARIANTS)
def test_engineered_inputs_are_unambiguous(variant):
    """float32 and float64 oracle agree on every decision: the condition for comparing the GPU with zero flips allowed."""
    o32, o64 = _oracle(variant, torch.float32), _oracle(variant, torch.float64)
    for name in ("active", "similar", "unique"):
        assert torch.equal(o32[name], o64[name]), name
    assert o32["appended"] == o64["appended"]
    assert o32["out"].counts == o64["out"].counts == [COUNTS[b] + len(o32["appended"][b]) for b in range(B)]
    assert o32["max_dot"] == o64["max_dot"] == 1.25
    fr = o32["fr"]
    for b in range(B):  # the appended rows are the frame's pixels in row-major order
        hw = torch.tensor(o32["appended"][b], dtype=torch.int64).view(-1, 2)
        assert torch.equal(o32["out"].points[b][COUNTS[b]:], fr["gV"][b, 0, hw[:, 0], hw[:, 1]])
        assert hw.shape[0] >= 8 and all(p not in o32["appended"][b] for p in HOLES)
    # the frame itself: z and the normal are exact, x and y carry the reference's 1 / (f + 1e-6)
    V, N = fr["V"][:, 0], fr["N"][:, 0]
    ok = (fr["depth"] > 0)[:, 0, :, :, 0]
    assert bool((V[..., 2][ok] == 2.0).all()) and torch.equal(V[:, 2, 3], torch.tensor([[0.0, 0.0, 2.0]] * B))
    ws, hs = torch.arange(W).float().view(1, 1, W), torch.arange(H).float().view(1, H, 1)
    assert float(((V[..., 0] - (ws - 3) / 2).abs() * ok).max()) < 1e-6 and float(((V[..., 1] - (hs - 2) / 2).abs() * ok).max()) < 1e-6
    plain = ok.clone()
    for h, w in HOLES:  # the forward differences of a hole's left and upper neighbour reach into the hole
        plain[:, h, w - 1] = False
        plain[:, h - 1, w] = False
        if h == H - 2:  # the last row repeats the difference of the row above it
            plain[:, H - 1, w] = False
    assert bool((N[plain] == torch.tensor([0.0, 0.0, 1.0])).all())
    for h, w in HOLES:
        assert not V[:, h, w].any() and not N[:, h, w].any() and not fr["gV"][:, 0, h, w].any()
    if variant != "main":
        moved = [0] if variant == "b1_only" else [0, 1]
        for b in moved:
            assert not any(int(r[0]) == b for r in o32["unique"])
        if variant == "b1_only":
            assert any(int(r[0]) == 1 for r in o32["unique"])
        return
    # ---- every hand-placed row's fate, by name
    idx = {k: v[0] for k, v in _HAND.items()}
    act, sim, win = _fates(o32, 0)
    for name, px in _EXPECT_PIXEL.items():
        assert act.get(idx[name]) == px, (name, act.get(idx[name]))
    for name in _INACTIVE:
        assert idx[name] not in act, name
    for name in _NOT_SIMILAR:
        assert idx[name] in act and idx[name] not in sim, name
    for name in _WINNERS:
        assert idx[name] in sim and idx[name] in win, name
    for name in _LOSERS:
        assert idx[name] in sim and idx[name] not in win, name
    assert all(900 + i not in act for i in range(8))
    # the three rows of a tie group do hold bit-equal keys, in float32 and in float64
    for o in (o32, o64):
        for grp in ("tieA", "tieB"):
            n = torch.tensor([idx[grp + "_%d" % i] for i in range(3)])
            h, w = _TIE_PIX[grp]
            pts = torch.stack([_case("main")["points"][0][i] for i in n]).to(o["fr"]["gV"].dtype)
            ray = ((pts - o["fr"]["gV"][0, 0, h, w]) ** 2).sum(-1)
            assert ray[0] == ray[1] == ray[2] and ray[0] > 0
    # pixels: the hole under a map point and the pixel whose only candidates fail a threshold are / are not appended
    assert (1, 5) not in o32["appended"][0] and (1, 1) in o32["appended"][0] and (2, 3) not in o32["appended"][0]
    for px in _EMPTY | {(3, 2), (3, 4)}:
        assert px in o32["appended"][0]
    # the lattice: dozens of similar candidates on every pixel it reaches whose frame normal is (0, 0, 1), and on some
    # of them the winning key is held by more than one row (same c, same depth), so the index decides there too
    per_pixel = {}
    for n in sim:
        per_pixel.setdefault(act[n], []).append(n)
    lattice = {k: v for k, v in per_pixel.items() if k not in _RESERVED}
    assert len(lattice) >= 20 and min(len(v) for v in lattice.values()) >= 15
    c0 = _case("main")
    shared = 0
    for px, ns in lattice.items():
        key = lambda n: (float(c0["feats"][0][n]), float(c0["points"][0][n, 2]))  # same pixel, c and depth: bit-equal keys
        (winner,) = [n for n in ns if n in win]
        holders = [n for n in ns if key(n) == key(winner)]
        assert winner == min(holders), px
        assert key(winner)[0] == max(key(n)[0] for n in ns), px
        shared += len(holders) > 1
    assert shared >= 4
    # b = 1 under the rotated pose
    idx1 = {k: v[0] for k, v in _HAND1.items()}
    act1, sim1, win1 = _fates(o32, 1)
    assert act1 == {idx1["dist_below"]: (2, 3), idx1["dist_eq"]: (2, 3), idx1["u_lo_in"]: (2, 0), idx1["plain"]: (3, 5)}
    assert sim1 == win1 == {idx1["dist_below"], idx1["u_lo_in"], idx1["plain"]}


# ---------------------------------------------------------------------------------------------- GPU side
def _arena(variant, nmax, feats=True):
    c = _case(variant)
    out = []
    for name, width in (("points", 3), ("normals", 3), ("colors", 3), ("feats", 1))[: 4 if feats else 3]:
        a = torch.zeros((B, nmax, width), dtype=torch.float32)
        for b in range(B):
            a[b, : COUNTS[b]] = c[name][b]
        out.append(a.to(DEV))
    return out


def _frame_args(variant):
    c = _case(variant)
    return c["depth"][:, 0].contiguous().to(DEV), c["rgb"][:, 0].contiguous().to(DEV), c["K"].to(DEV), c["pose"].to(DEV)


def _run_fusion(gs, variant, nmax, taped=False):
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    depth, rgb, K, pose = _frame_args(variant)
    arena = _arena(variant, nmax)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    stats = torch.zeros(4 + B, dtype=torch.int32, device=DEV)
    if not taped:
        ops.pointfusion_update_raw(depth, rgb, K, pose, *arena, counts, DIST_TH, DOT_TH, SIGMA, stats)
    else:
        tape = torch.empty(nv.ws_bytes("gs_pointfusion_update_tape_bytes", B, H, W), dtype=torch.uint8, device=DEV)
        ws = nv.workspace(nv.ws_bytes("gs_pointfusion_update_ws_bytes", B, H, W, nmax), depth.device, "fusion_step")
        nv.call("gs_pointfusion_update_taped", nv.ptr(depth), nv.ptr(rgb), nv.ptr(K), nv.ptr(pose), B, H, W, *[nv.ptr(a) for a in arena],
                nv.ptr(counts), nmax, DIST_TH, DOT_TH, SIGMA, nv.ptr(stats), nv.ptr(tape), tape.numel(), nv.ptr(ws), ws.numel(),
                nv.stream())
    torch.cuda.synchronize()
    return [a.cpu() for a in arena], counts.cpu().tolist(), stats.cpu().tolist()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    same = a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    if not same and a.shape == b.shape:  # say what kind of difference it is before the assertion fires
        bad = _bits(a) != _bits(b)
        print("bits differ at %d of %d values, largest |a - b| = %.3e, first at %s: %r vs %r" % (
            int(bad.sum()), bad.numel(), float((a - b).abs().max()), bad.nonzero()[0].tolist(), float(a[bad][0]), float(b[bad][0])))
    return same


NAMES = ("points", "normals", "colors", "feats")


def _check_fusion(variant, got, counts, stats, nmax, clamped=()):
    """The updated arena against the oracle: the stats words here, the map's values in _check_fusion_values."""
    c, o32, o64 = _case(variant), _oracle(variant, torch.float32), _oracle(variant, torch.float64)
    want_counts = [min(n, nmax) for n in o32["out"].counts]
    assert counts == want_counts
    assert all((want_counts[b] < o32["out"].counts[b]) == (b in clamped) for b in range(B))
    assert stats[0] == o32["active"].shape[0] and stats[1] == o32["unique"].shape[0]
    assert stats[2] == (1 if clamped else 0)
    assert stats[3] == int(_bits(torch.tensor([o32["max_dot"]], dtype=torch.float32))) and o32["max_dot"] > 1.0
    assert stats[4:] == [want_counts[b] - COUNTS[b] for b in range(B)]
    _check_fusion_values(variant, c["feats"], o32["unique"], o32["out"], o64["out"], got, counts, nmax)


def _check_fusion_values(label, feats_in, unique, out32, out64, got, counts, nmax):
    """An updated map (four padded arrays `got`, per-element `counts`) against the oracle's (out32, out64: the float32 and
    float64 Clouds after fuse_with_map with the table `unique` on a map whose confidence counts were feats_in).  Decisions and
    every value that does not pass through alpha: exact.  Values that carry alpha: rel_err against the float64 oracle,
    bounded by 4 x the float32 oracle's own (floor 2^-22).  Shared with tests/test_fusion_stages_edges.py."""
    want_counts = [min(n, nmax) for n in out32.counts]
    assert counts == want_counts
    alpha_gpu, alpha_32, alpha_64 = ({n: [] for n in NAMES} for _ in range(3))
    for b in range(len(feats_in)):
        n_in, n_out = feats_in[b].shape[0], want_counts[b]
        matched = torch.zeros(n_in, dtype=torch.bool)
        matched[[int(r[1]) for r in unique if int(r[0]) == b]] = True
        # the matched rows are the rows whose confidence count moved (alpha >= exp(-8.5 / 4.5) here, counts <= 3)
        assert torch.equal(got[3][b, :n_in, 0] != feats_in[b][:, 0], matched), "set of matched rows, b = %d" % b
        for i, name in enumerate(NAMES):
            g, w32, w64 = got[i][b], getattr(out32, name)[b], getattr(out64, name)[b]
            assert _same_bits(g[:n_in][~matched], w32[:n_in][~matched]), (name, b, "unmatched live rows")
            if name != "feats":  # row-major order over the unmatched valid pixels, bit for bit
                assert _same_bits(g[n_in:n_out], w32[n_in:n_out]), (name, b, "appended rows")
            assert not g[n_out:].any(), (name, b, "rows beyond the new count")
            sel = matched if name != "feats" else torch.cat([matched, torch.ones(n_out - n_in, dtype=torch.bool)])
            alpha_gpu[name].append(g[:n_out][: sel.shape[0]][sel]); alpha_32[name].append(w32[: sel.shape[0]][sel])
            alpha_64[name].append(w64[: sel.shape[0]][sel])
    for name in NAMES:
        if sum(x.numel() for x in alpha_gpu[name]) == 0:
            continue
        ref = torch.cat(alpha_64[name])
        own = rel_err(torch.cat(alpha_32[name]), ref)
        err = rel_err(torch.cat(alpha_gpu[name]), ref)
        bound = max(4.0 * own, 2.0 ** -22)
        print("%s/%s: alpha-path rel_err GPU %.3e, float32 oracle %.3e, bound %.3e" % (label, name, err, own, bound))
        # Measured on an MI355X, GPU / float32 oracle / bound -- variant main: points 5.760e-8 / 5.760e-8 / 2.384e-7 (floor),
        # normals 5.619e-8 / 5.619e-8 / 2.384e-7 (floor), colours 1.132e-7 / 1.132e-7 / 4.529e-7, counts 4.354e-8 / 4.354e-8 /
        # 2.384e-7 (floor); variant none (appended counts only): 1.415e-7 / 1.415e-7 / 5.659e-7; variant b1_only: points
        # 4.923e-8, normals 5.960e-8, colours 1.041e-7, counts 2.516e-8, each equal to the float32 oracle's own figure.
        # The bound is not fixed in advance: two expf implementations may each be an ulp or two off in opposite directions
        # and the merge multiplies by alpha once, hence 4 x the float32 oracle's own error, with a floor of 2^-22.
        assert err <= bound, (name, err, bound)


@pytest.mark.gpu
def test_pointfusion_update_decisions_and_values(gs):
    """Reaches: borders, half pixels, z <= 0, both thresholds on and one ulp off, dot > 1 (stats[3]), bit-equal keys across
    items / workgroups in two arrangements, key order, c == 0, a point over a hole, the rotated pose of b = 1, counts
    (2077, 5), the re-rounding of unmatched live rows, the append order, rows beyond the count."""
    got, counts, stats = _run_fusion(gs, "main", NMAX)
    _check_fusion("main", got, counts, stats, NMAX)
    # by name as well: the winners' counts moved, the losers' and the rejected rows' did not
    moved = got[3][0, :, 0] != _arena("main", NMAX)[3][0, :, 0].cpu()
    for name in _WINNERS:
        assert moved[_HAND[name][0]], name
    for name in _LOSERS + _NOT_SIMILAR + _INACTIVE:
        assert not moved[_HAND[name][0]], name
    # re-rounding is not the identity: c = 3 rows that no pixel takes differ from their input where the formula says
    c = _case("main")
    changed = 0
    for name in ("u_lo_out", "dist_eq", "dot_eq", "half_2p5", "z_neg"):
        n = _HAND[name][0]
        x = c["colors"][0][n]
        assert _same_bits(got[2][0, n], (3.0 * x + 0.0) * (1.0 / torch.tensor(3.0))), name
        changed += int((_bits(got[2][0, n]) != _bits(x)).sum())
    assert changed > 0


@pytest.mark.gpu
def test_pointfusion_update_taped_leaves_the_same_arena(gs):
    plain, taped = _run_fusion(gs, "main", NMAX), _run_fusion(gs, "main", NMAX, taped=True)
    assert plain[1] == taped[1] and plain[2] == taped[2]
    assert all(_same_bits(a, b) for a, b in zip(plain[0], taped[0]))


@pytest.mark.gpu
def test_pointfusion_update_without_any_correspondence(gs):
    """FLAG_ANY stays 0: live rows keep their bits (c = 3 rows included), every valid pixel is appended."""
    got, counts, stats = _run_fusion(gs, "none", NMAX)
    _check_fusion("none", got, counts, stats, NMAX)
    c = _case("none")
    assert stats[1] == 0 and stats[4:] == [H * W - len(HOLES)] * B
    for i, name in enumerate(NAMES):
        for b in range(B):
            assert _same_bits(got[i][b, : COUNTS[b]], c[name][b]), (name, b)


@pytest.mark.gpu
def test_pointfusion_update_correspondence_in_one_batch_element_only(gs):
    """The reference merges the whole padded batch as soon as ANY element has a correspondence: b = 0 has none here and
    its rows are re-rounded all the same."""
    got, counts, stats = _run_fusion(gs, "b1_only", NMAX)
    _check_fusion("b1_only", got, counts, stats, NMAX)
    c, o32 = _case("b1_only"), _oracle("b1_only", torch.float32)
    assert stats[1] == sum(int(r[0]) == 1 for r in o32["unique"]) > 0 and stats[4] == H * W - len(HOLES)
    c3 = c["feats"][0][:, 0] == 3.0
    for i, name in enumerate(NAMES[:3]):
        x = c[name][0][c3]
        want = (3.0 * x + 0.0 * 0.0) * (1.0 / torch.tensor(3.0))
        differs = _bits(want) != _bits(x)
        assert torch.equal(_bits(got[i][0, : COUNTS[0]][c3]) != _bits(x), differs), name
        assert _same_bits(got[i][0, : COUNTS[0]][c3], want), name
        if name == "colors":
            assert differs.any()


@pytest.mark.gpu
def test_pointfusion_update_capacity_clamp(gs):
    """count + unmatched = Nmax + 7 for b = 0: the count stops at Nmax, the flag is raised, the rows that fit are the first of
    the oracle's list; b = 1 is not affected."""
    o32 = _oracle("main", torch.float32)
    nmax = o32["out"].counts[0] - 7
    assert nmax > COUNTS[0] and nmax >= o32["out"].counts[1]
    got, counts, stats = _run_fusion(gs, "main", nmax)
    _check_fusion("main", got, counts, stats, nmax, clamped=(0,))
    assert counts == [nmax, o32["out"].counts[1]] and stats[2] == 1
    assert stats[4:] == [len(o32["appended"][0]) - 7, len(o32["appended"][1])]


# ---------------------------------------------------------------------------------------------- 3. aggregate update
def _run_aggregate(gs, nmax):
    from gradslam_amd import ops

    depth, rgb, K, pose = _frame_args("main")
    arena = _arena("main", nmax, feats=False)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    stats = torch.full((4 + B,), -1, dtype=torch.int32, device=DEV)
    ops.aggregate_update_raw(depth, rgb, K, pose, *arena, counts, stats)
    torch.cuda.synchronize()
    return [a.cpu() for a in arena], counts.cpu().tolist(), stats.cpu().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("clamp", [False, True], ids=["fits", "clamped"])
def test_aggregate_update_against_oracle(gs, clamp):
    """Holes, the rotated pose of b = 1, starting counts (2077, 5); with and without the capacity clamp."""
    c, o32 = _case("main"), _oracle("main", torch.float32)
    full = o32["agg"].counts
    assert full == [COUNTS[b] + H * W - len(HOLES) for b in range(B)]
    nmax = full[0] - 7 if clamp else NMAX
    got, counts, stats = _run_aggregate(gs, nmax)
    want = [min(n, nmax) for n in full]
    assert counts == want and stats[2] == (1 if clamp else 0) and stats[4:] == [want[b] - COUNTS[b] for b in range(B)]
    for i, name in enumerate(NAMES[:3]):
        for b in range(B):
            assert _same_bits(got[i][b, : COUNTS[b]], c[name][b]), (name, b, "rows the map held")
            assert _same_bits(got[i][b, COUNTS[b]:want[b]], getattr(o32["agg"], name)[b][COUNTS[b]:want[b]]), (name, b, "appended")
            assert not got[i][b, want[b]:].any(), (name, b, "rows beyond the new count")


# ---------------------------------------------------------------------------------------------- 4. compaction seams
# 1024 * 1024 rows are 1024 blocks, the last size that scans its block counts inside the write pass (kSelfScanBlocks);
# one row more takes the scan launch, whose 1024-wide chunks then carry for the first time
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 1024 * 1024, 1024 * 1024 + 1]


def _masks(n):
    i = torch.arange(n, device=DEV)
    out = {"none": torch.zeros(n, dtype=torch.bool, device=DEV), "all": torch.ones(n, dtype=torch.bool, device=DEV),
           "first": i == 0, "last": i == n - 1, "3mod4": (i % 4) == 3}
    if n >= 1023:
        g = torch.Generator(device="cpu").manual_seed(n)
        out["random30"] = (torch.rand(n, generator=g) < 0.3).to(DEV)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_compact_rows_seams(gs, n):
    from gradslam_amd import ops

    g = torch.Generator(device="cpu").manual_seed(7 + n)
    f = torch.rand((n, 3), generator=g).to(DEV)
    q = torch.randint(-2 ** 62, 2 ** 62, (n, 4), generator=g, dtype=torch.int64).to(DEV)
    for name, m in _masks(n).items():
        for src in (f, q):
            out = ops.compact_rows(src, m)
            assert out.dtype == src.dtype and torch.equal(out, src[m]), (name, src.dtype)
        assert torch.equal(ops.compact_rows(f, m.to(torch.uint8)), f[m]), (name, "uint8 mask")


def _append(nv, srcs, dsts, mask, count, cap):
    k = len(srcs)
    appended, overflow = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    n = mask.shape[0]
    ws = nv.workspace(nv.ws_bytes("gs_append_rows_ws_bytes", n), mask.device, "append_test")
    a_src = (ctypes.c_void_p * k)(*[s.data_ptr() for s in srcs])
    a_dst = (ctypes.c_void_p * k)(*[d.data_ptr() for d in dsts])
    widths = (ctypes.c_int * k)(*[s.shape[1] for s in srcs])
    nv.call("gs_append_rows", k, a_src, widths, a_dst, nv.ptr(mask), n, nv.ptr(count), cap, nv.ptr(appended), nv.ptr(overflow),
            nv.ptr(ws), ws.numel(), nv.stream())
    return int(count), int(appended), int(overflow)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_append_rows_seams(gs, n):
    """gs_append_rows with arrays of width 3 and 1: rows behind a device-side count, sentinels before and after intact,
    and the capacity clamp one row short of what the mask selects."""
    from gradslam_amd import _native as nv

    g = torch.Generator(device="cpu").manual_seed(11 + n)
    a, b = torch.rand((n, 3), generator=g).to(DEV), torch.rand((n, 1), generator=g).to(DEV)
    base, rows = 5, 5 + n + 4
    for name, m in _masks(n).items():
        sel_a, sel_b = a[m], b[m]
        k = sel_a.shape[0]
        for cap in ([rows - 1] if k < 2 else [rows - 1, base + k - 1]):
            da, db = torch.full((rows, 3), -5.0, device=DEV), torch.full((rows, 1), -5.0, device=DEV)
            da[:base], db[:base] = 7.0, 7.0
            count = torch.tensor([base], dtype=torch.int32, device=DEV)
            fit = min(k, cap - base)
            got = _append(nv, (a, b), (da, db), m.to(torch.uint8), count, cap)
            assert got == (base + fit, fit, 1 if fit < k else 0), (name, cap, got)
            assert torch.equal(da[base:base + fit], sel_a[:fit]) and torch.equal(db[base:base + fit], sel_b[:fit]), (name, cap)
            assert bool((da[:base] == 7.0).all()) and bool((db[:base] == 7.0).all()), (name, cap)
            assert bool((da[base + fit:] == -5.0).all()) and bool((db[base + fit:] == -5.0).all()), (name, cap)


@pytest.mark.gpu
def test_compaction_of_no_rows(gs):
    """n = 0 never reaches a launch with an empty grid (compact_blocks(0) is 1).  Through the wrapper an empty tensor either
    has a NULL data pointer, which gs_compact_rows refuses by name, or a real one, and then the result is empty; a caller
    that passes real buffers and n = 0 gets a zero count from one fully masked-off block, and nothing is written."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    empty = torch.empty((0, 3), device=DEV)
    mask = torch.empty((0,), dtype=torch.bool, device=DEV)
    try:
        out = ops.compact_rows(empty, mask)
    except RuntimeError as e:
        assert "gs_compact_rows" in str(e)
    else:
        assert out.shape == (0, 3)
    # real buffers, zero rows: accepted, nothing selected, nothing written
    src, dst = torch.rand((4, 3), device=DEV), torch.full((4, 3), -5.0, device=DEV)
    m8 = torch.ones(4, dtype=torch.uint8, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = nv.workspace(nv.ws_bytes("gs_compact_ws_bytes", 0), src.device, "compact")
    nv.call("gs_compact_rows", nv.ptr(src), nv.ptr(m8), 0, 3, nv.ptr(dst), nv.ptr(cnt), nv.ptr(ws), ws.numel(), nv.stream())
    assert int(cnt) == 0 and bool((dst == -5.0).all())
