"""The per-op PointFusion stages (slam/fusionutils.py: find_active_map_points, find_similar_map_points, find_best_unique_
correspondences, find_correspondences, fuse_with_map, update_map_fusion) and the entry points under them (gs_fusion_similar,
gs_fusion_unique, gs_fusion_new_mask; kernels similar_k, unique_pass1_k, unique_pass2_k, valid_mask_k, clear_matched_k,
scatter_match_k), on the engineered inputs of tests/test_map_update_edges.py.

That file proves on the CPU (test_engineered_inputs_are_unambiguous) that the float32 and the float64 oracle take identical
decisions on these inputs; test_device_frame_is_the_frame_the_proof_assumed shows that the frame the kernels see is the frame
that proof assumed (z = 2 and the normal (0, 0, 1) exact, the centre pixel's vertex (0, 0, 2), holes zero, b = 1 pushed exactly
through its 0/+-1 rotation).  On that ground every table below is compared with torch.equal: no flip is allowed.

Which test reaches which edge (row names are _HAND's in tests/test_map_update_edges.py):
  dist == th / one ulp below, dot == th / one ulp above (similar_pair's < and >)
                                        test_wrappers_stage_by_stage, test_raw_similar, test_table_longer_than_one_grid_pass
  dot product > 1: warning names 1.25; max_dot holds its bits; max_dot is +0.0 when the largest dot is exactly 1.0
                                        test_wrappers_stage_by_stage, test_raw_similar
  no similar point at all: warning, (0, 4) int64 table, all-false mask     test_wrappers_stage_by_stage[none]
  bit-equal keys in one thread / two workgroups, smallest n wins, whatever the order of the table
                                        test_wrappers_stage_by_stage, test_raw_unique (reversed, shuffled)
  key order: confidence before ray distance, c == 0 rows; candidates that fail a threshold compete (the ACTIVE table)
                                        test_wrappers_stage_by_stage (unique of the active table)
  keep flags == compacted table (keep != NULL against keep == NULL); *d_n < max_rows; *d_n == 0; max_rows == 0;
  words behind the count untouched      test_raw_similar, test_raw_unique, test_wrappers_stage_by_stage (find_correspondences)
  a point over a hole; depth -1 / NaN / +inf; rows == NULL
                                        test_raw_new_mask
  merge: matched set, re-rounding of unmatched live rows, append order, padding, alpha path; inplace or not; what the
  object that was passed in holds afterwards; no match at all; a match in one batch element only; grad mode
                                        test_fuse_with_map_against_oracle, test_update_map_fusion_against_oracle
  rows beyond the first 2048 x 256 of a table (the stride loops' second trip)
                                        test_table_longer_than_one_grid_pass
  NULL / non-positive / short-workspace arguments, the workspace layout
                                        test_fusion_stage_entry_points_refuse_bad_arguments (no device work: runs anywhere)

The input object after fuse_with_map.  oracle.fusion.fuse_with_map is functional (it leaves its input Cloud alone, which
test_oracle_fuse_is_functional states); the reference proper assigns the merged padded arrays to the object it was given
before it clones (slam/fusionutils.py:696-699, :718-720), and gradslam_amd does the same.  So what is pinned is: after a call
with a non-empty table the object passed in keeps its counts and holds, bit for bit, the first counts[b] rows of the result;
with an empty table it holds its input bits; with inplace=True it IS the result.

Alpha-path figures of the per-op path (rel_err against the float64 oracle; GPU / float32 oracle / bound = max(4 x the
float32 oracle's own, 2^-22), the rule of _check_fusion_values), measured on an MI355X:
  main (fuse_with_map, update_map_fusion, and the 255-fold map of test_table_longer_than_one_grid_pass alike):
      points 5.760e-8 / 5.760e-8 / 2.384e-7 (floor), normals 5.619e-8 / 5.619e-8 / 2.384e-7 (floor),
      colours 1.132e-7 / 1.132e-7 / 4.529e-7, counts 4.354e-8 / 4.354e-8 / 2.384e-7 (floor)
  none (appended counts only): 1.415e-7 / 1.415e-7 / 5.659e-7
  b1_only: points 4.923e-8 / 4.923e-8 / 2.384e-7 (floor), normals 5.960e-8 / 5.960e-8 / 2.384e-7 (floor),
      colours 1.041e-7 / 1.041e-7 / 4.162e-7, counts 2.516e-8 / 2.516e-8 / 2.384e-7 (floor)
They are the one-call path's figures (tests/test_map_update_edges.py): both paths round like the float32 oracle.

The long table.  With b = 0's map tiled 255 times the active table has 526 069 rows, but the similar table only 159 888,
and every pixel's winner and a clearing row for every pixel lie in the first copy.  The similarity stage is checked on the
active table's rows beyond the first pass by name; b = 1's rows stand at the table's end, so find_correspondences loses them
if a unique pass loses its second trip; and gs_fusion_unique and gs_fusion_new_mask are also given the "late" table
(_late_table), in which one pixel is held only by a row beyond the first pass.

Not detectable by value: a stride of blockDim.x in place of gridDim.x * blockDim.x in similar_k makes every block rescan the
rows behind it and store the same verdicts again; the long table catches a stride that SKIPS rows (twice the grid, say).
"""
import functools
import warnings

import pytest
import torch

from tests.test_map_update_edges import (B, COUNTS, DEV, DIST_TH, DOT_TH, H, HOLES, NAMES, R1, SIGMA, T1, VARIANTS, W, _HAND,
                                         _HAND1, _LOSERS, _WINNERS, _bits, _case, _check_fusion_values, _oracle, _same_bits)

F32, F64 = torch.float32, torch.float64
GRID_PASS = 2048 * 256  # grid1d in csrc/fusion.hip: at most 2048 blocks of 256 threads; rows beyond are the stride loop's
SENT = 0xAB


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ---------------------------------------------------------------------------------------------- expected tables (CPU)
def _key(t, nmax):
    """One integer per table row: (b, n) is unique within a table."""
    return t[:, 0] * nmax + t[:, 1]


def _member(active, similar, nmax):
    return torch.isin(_key(active, nmax), _key(similar, nmax))


def _cloud_of(c, dtype):
    from oracle.cloud import Cloud

    cv = lambda xs: [x.to(dtype) for x in xs]
    return Cloud(cv(c["points"]), cv(c["normals"]), cv(c["colors"]), cv(c["feats"]))


@functools.lru_cache(maxsize=None)
def _unique_of_active(variant, dtype):
    """The oracle's best unique correspondences among ALL active rows (no similarity filter in front)."""
    from oracle import fusion

    o = _oracle(variant, dtype)
    return fusion.find_best_unique_correspondences(_cloud_of(_case(variant), dtype), o["fr"], o["active"])


@functools.lru_cache(maxsize=None)
def _oracle_warning_kinds(variant):
    """Which of the two warnings the oracle's similarity stage raises on this variant, in order."""
    from oracle import fusion

    o = _oracle(variant, F32)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        fusion.find_similar_map_points(_cloud_of(_case(variant), F32), o["fr"], o["active"], DIST_TH, DOT_TH)
    return _kinds(rec)


def _kinds(rec):
    """The warnings of the fusion stages (the oracle's or the package's) among the recorded ones, by kind and in order."""
    out = []
    for w in rec:
        if not w.filename.endswith(("fusionutils.py", "fusion.py")):
            continue
        msg = str(w.message)
        if "Max of dot product" in msg:
            assert issubclass(w.category, RuntimeWarning)
            out.append("dot")
        elif "No similar map points" in msg:
            assert issubclass(w.category, RuntimeWarning)
            out.append("none")
        else:
            out.append(msg)
    return out


@functools.lru_cache(maxsize=None)
def _unit_dot_case():
    """main with dot_big's normal set to (0, 0, 1): the largest dot product over the active rows is then exactly 1.0."""
    c = dict(_case("main"))
    c["normals"] = [x.clone() for x in c["normals"]]
    c["normals"][0][_HAND["dot_big"][0]] = torch.tensor([0.0, 0.0, 1.0])
    return c


def _max_dot(c, dtype):
    o = _oracle("main", dtype)  # same frame, same active table: normals take part in neither
    cloud = _cloud_of(c, dtype)
    b, n, h, w = o["active"].unbind(1)
    return float((o["fr"]["gN"][b, 0, h, w] * cloud.padded("normals")[b, n]).sum(-1).max())


# ---- a table longer than one grid pass: b = 0's map is k consecutive copies of main's 2077 rows
def _tiled_case(k):
    c = dict(_case("main"))
    for name in ("points", "normals", "colors", "feats"):
        c[name] = [c[name][0].repeat(k, 1), c[name][1]]
    return c


def _tile_table(t, k):
    """The table of the k-fold map from the table of the plain one: copy j of row (0, n, h, w) is (0, j * 2077 + n, h, w);
    b = 1 is as it was; (b, n) order."""
    t0, t1 = t[t[:, 0] == 0], t[t[:, 0] == 1]
    parts = []
    for j in range(k):
        tj = t0.clone()
        tj[:, 1] += j * COUNTS[0]
        parts.append(tj)
    return torch.cat(parts + [t1], 0)


def _derived_tables(k):
    """What the k-fold map's tables must be: active and similar are the tiled tables; unique is unchanged, because the first
    copy holds the smallest index of every bit-equal key."""
    o = _oracle("main", F32)
    return _tile_table(o["active"], k), _tile_table(o["similar"], k), o["unique"]


@functools.lru_cache(maxsize=None)
def _tiled_oracle(k, dtype):
    """The oracle proper on the k-fold map (under a second per precision at k = 255; computed once)."""
    from oracle import fusion

    cloud, fr = _cloud_of(_tiled_case(k), dtype), _oracle("main", dtype)["fr"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        active = fusion.find_active_map_points(cloud, fr)
        similar, mask = fusion.find_similar_map_points(cloud, fr, active, DIST_TH, DOT_TH)
        unique = fusion.find_best_unique_correspondences(cloud, fr, similar)
    return active, similar, unique, mask


def _tiled_tables(k):
    return _tiled_oracle(k, F32)[:3]


@functools.lru_cache(maxsize=None)
def _long_k():
    a = _oracle("main", F32)["active"]
    n0, n1 = int((a[:, 0] == 0).sum()), int((a[:, 0] == 1).sum())
    return -(-(GRID_PASS + 256 - n1) // n0)


@functools.lru_cache(maxsize=None)
def _tiled_fused(k, dtype):
    """The oracle's fuse_with_map on the k-fold map (elementwise over the padded map: cheap at any k)."""
    from oracle import fusion

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fusion.fuse_with_map(_cloud_of(_tiled_case(k), dtype), _oracle("main", dtype)["fr"], _oracle("main", F32)["unique"], SIGMA)


# ---------------------------------------------------------------------------------------------- CPU conditions
@pytest.mark.parametrize("variant", VARIANTS)
def test_unique_of_the_active_table_is_unambiguous(variant):
    """Rows that fail a threshold compete for their pixel too when the unique stage is given the active table.  Keys are
    confidence, then ray distance, and distinct ones differ by >= 2^-22 along z: float32 and float64 pick the same rows."""
    u32, u64 = _unique_of_active(variant, F32), _unique_of_active(variant, F64)
    diff = [(r32.tolist(), r64.tolist()) for r32, r64 in zip(u32, u64) if not torch.equal(r32, r64)] if u32.shape == u64.shape else "shapes"
    assert torch.equal(u32, u64), diff
    # it is another table than the similar one's winners: rows that are not similar win pixels here
    o = _oracle(variant, F32)
    assert u32.shape[0] >= o["unique"].shape[0] and u32.shape[0] > 0
    if variant == "main":
        assert not torch.equal(u32, o["unique"])
        won = {int(r[1]) for r in u32 if int(r[0]) == 0}
        assert _HAND["dist_eq"][0] in won and _HAND["dist_below"][0] not in won  # c = 3 beats c = 1 once dist_eq is let in


def test_unit_dot_case_has_a_largest_dot_of_exactly_one():
    assert _max_dot(_case("main"), F32) == _max_dot(_case("main"), F64) == 1.25
    assert _max_dot(_unit_dot_case(), F32) == _max_dot(_unit_dot_case(), F64) == 1.0


def test_oracle_warnings():
    assert _oracle_warning_kinds("main") == ["dot"]
    assert _oracle_warning_kinds("none") == ["dot", "none"]
    assert _oracle_warning_kinds("b1_only") == ["dot"]


def test_oracle_fuse_is_functional():
    from oracle import fusion

    c, o = _case("main"), _oracle("main", F32)
    cloud = _cloud_of(c, F32)
    out = fusion.fuse_with_map(cloud, o["fr"], o["unique"], SIGMA)
    assert out is not cloud and cloud.counts == list(COUNTS)
    for name in NAMES:
        assert all(torch.equal(x, y) for x, y in zip(getattr(cloud, name), c[name]))


def test_tiled_tables_are_the_oracles():
    """On the k-fold map (k = 3, and the k of the long table) the float32 and the float64 oracle agree, and give what the
    derivation says: tiled active and similar tables, the plain map's winners."""
    for k in (3, _long_k()):
        want = _derived_tables(k)
        for dtype in (F32, F64):
            active, similar, unique, mask = _tiled_oracle(k, dtype)
            assert torch.equal(active, want[0]) and torch.equal(similar, want[1]) and torch.equal(unique, want[2]), (k, dtype)
            assert torch.equal(mask, _member(want[0], want[1], k * COUNTS[0]))
    # the long table is long enough, and the rows the GPU test names lie beyond the first grid pass
    active = _tiled_tables(k)[0]
    assert active.shape[0] >= GRID_PASS + 256 and _tile_table(_oracle("main", F32)["active"], k - 1).shape[0] < GRID_PASS + 256
    for name in ("dist_below", "dot_above", "dist_eq", "dot_eq"):
        assert _row_of(active, (k - 1) * COUNTS[0] + _HAND[name][0]) > GRID_PASS, name


def _row_of(table, n, b=0):
    (i,) = ((table[:, 0] == b) & (table[:, 1] == n)).nonzero().view(-1).tolist()
    return i


# In the k-fold map every pixel's winner, and a row that clears every pixel, lies in the FIRST copy: a unique or a clear pass that
# lost its second trip would go unnoticed.  The "late" table is the tiled active table without the rows of pixel (5, 3) of
# b = 0 (v_hi_in's, the only candidate there) in every copy but the last: that pixel's only row then lies beyond one grid pass.
LATE_PIX = (5, 3)


def _late_table(k):
    t = _tile_table(_oracle("main", F32)["active"], k)
    at = (t[:, 0] == 0) & (t[:, 2] == LATE_PIX[0]) & (t[:, 3] == LATE_PIX[1])
    return t[~at | (t[:, 1] >= (k - 1) * COUNTS[0])]


def _late_unique(k):
    """The winners of the late table: those of the plain active table, with pixel (5, 3)'s in the last copy."""
    u = _unique_of_active("main", F32).clone()
    at = (u[:, 0] == 0) & (u[:, 2] == LATE_PIX[0]) & (u[:, 3] == LATE_PIX[1])
    assert int(at.sum()) == 1 and int(u[at][0, 1]) == _HAND["v_hi_in"][0]
    u[at, 1] += (k - 1) * COUNTS[0]
    return u


def test_late_table_winners_are_the_oracles():
    from oracle import fusion

    for k in (3, _long_k()):
        for dtype in (F32, F64) if k == 3 else (F32,):  # (the sort of half a million rows takes a second and a half)
            got = fusion.find_best_unique_correspondences(_cloud_of(_tiled_case(k), dtype), _oracle("main", dtype)["fr"], _late_table(k))
            assert torch.equal(got, _late_unique(k)), (k, dtype)
    t = _late_table(k)
    assert t.shape[0] >= GRID_PASS + 256 and _row_of(t, (k - 1) * COUNTS[0] + _HAND["v_hi_in"][0]) > GRID_PASS
    assert int(((t[:, 0] == 0) & (t[:, 2] == LATE_PIX[0]) & (t[:, 3] == LATE_PIX[1])).sum()) == 1


def _align256(n):
    return -(-n // 256) * 256


def test_fusion_stage_entry_points_refuse_bad_arguments():
    """NULL pointers, non-positive sizes and max_rows < 0 return -1, a missing or short workspace -2 (the device pointers below
    are never read: every check happens on the host before the first launch or memset)."""
    from gradslam_amd import _native as nv

    lib = nv.lib()
    P = 4096  # a non-NULL stand-in

    def refused(fn, ok, pos, bad, code=-1):
        args = list(ok)
        args[pos] = bad
        assert fn(*args) == code, (pos, bad)

    # rows, d_n, max_rows, gv, gn, H, W, mp, mn, Nmax, dist_th, dot_th, keep, max_dot, stream
    ok = [P, P, 10, P, P, 6, 8, P, P, 100, 0.1, 0.9, P, None, None]
    for pos in (0, 1, 3, 4, 7, 8, 12):
        refused(lib.gs_fusion_similar, ok, pos, None)
    for pos, bad in ((5, 0), (5, -1), (6, 0), (6, -3), (9, 0), (9, -1), (2, -1)):
        refused(lib.gs_fusion_similar, ok, pos, bad)
    assert b"gs_fusion_similar" in lib.gs_last_error()

    # rows, keep, d_n, max_rows, gv, B, H, W, mp, cc, Nmax, out_rows, out_count, ws, ws_bytes, stream
    ok = [P, None, P, 10, P, 2, 6, 8, P, P, 100, P, P, P, 1 << 20, None]
    for pos in (0, 2, 4, 8, 9, 11, 12):
        refused(lib.gs_fusion_unique, ok, pos, None)
    for pos, bad in ((5, 0), (5, -1), (6, 0), (6, -1), (7, 0), (7, -1), (10, 0), (10, -1), (3, -1)):
        refused(lib.gs_fusion_unique, ok, pos, bad)
    refused(lib.gs_fusion_unique, ok, 13, None, -2)
    refused(lib.gs_fusion_unique, ok, 14, lib.gs_fusion_unique_ws_bytes(2, 6, 8) - 1, -2)
    refused(lib.gs_fusion_unique, ok, 14, 0, -2)
    assert b"gs_fusion_unique" in lib.gs_last_error()
    # the stated layout: a 64-bit key and a 32-bit index per pixel, then the compaction's two ints per 1024-pixel block
    for Bq, Hq, Wq in ((2, 6, 8), (1, 480, 640), (3, 33, 31)):
        npix = Bq * Hq * Wq
        want = _align256(8 * npix) + _align256(4 * npix) + _align256(2 * 4 * -(-npix // 1024))
        assert lib.gs_fusion_unique_ws_bytes(Bq, Hq, Wq) == want, (Bq, Hq, Wq)

    # depth, rows, d_n, max_rows, B, H, W, mask, stream
    ok = [P, P, P, 10, 2, 6, 8, P, None]
    for pos in (0, 7, 1, 2):  # rows / d_n may be NULL only with max_rows == 0
        refused(lib.gs_fusion_new_mask, ok, pos, None)
    for pos, bad in ((4, 0), (4, -1), (5, 0), (5, -1), (6, 0), (6, -1), (3, -1)):
        refused(lib.gs_fusion_new_mask, ok, pos, bad)
    assert b"gs_fusion_new_mask" in lib.gs_last_error()


# ---------------------------------------------------------------------------------------------- GPU side
def _frame(gs, c, channels_first=False, depth_grad=False):
    rgb, depth = c["rgb"].to(DEV), c["depth"].to(DEV)
    if channels_first:
        rgb, depth = rgb.permute(0, 1, 4, 2, 3).contiguous(), depth.permute(0, 1, 4, 2, 3).contiguous()
    if depth_grad:
        depth.requires_grad_(True)
    return gs.RGBDImages(rgb, depth, c["K"].to(DEV), c["pose"].to(DEV), channels_first=channels_first)


def _cloud(gs, c):
    mv = lambda xs: [x.clone().to(DEV) for x in xs]
    return gs.Pointclouds(points=mv(c["points"]), normals=mv(c["normals"]), colors=mv(c["colors"]), features=mv(c["feats"]))


def _arena_of(pcs):
    got = [x.detach().cpu() for x in (pcs.points_padded, pcs.normals_padded, pcs.colors_padded, pcs.features_padded)]
    return got, pcs.num_points_per_pointcloud.tolist()


def _recorded(fn, *args):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*args)
    return out, rec


# ---- 0. the frame
@pytest.mark.gpu
@pytest.mark.parametrize("channels_first", [False, True], ids=["channels_last", "channels_first"])
def test_device_frame_is_the_frame_the_proof_assumed(gs, channels_first):
    """What test_engineered_inputs_are_unambiguous asserts on the oracle's frame, on the frame the kernels read."""
    c = _case("main")
    assert all(torch.equal(c[k], _case(v)[k]) for k in ("depth", "rgb", "K", "pose") for v in VARIANTS)  # one frame for all variants
    fr = _frame(gs, c, channels_first)
    if channels_first:
        fr = fr.to_channels_last()
    V, N, gV, gN = (x[:, 0].cpu() for x in (fr.vertex_map, fr.normal_map, fr.global_vertex_map, fr.global_normal_map))
    assert V.shape == N.shape == gV.shape == gN.shape == (B, H, W, 3) and V.dtype == torch.float32
    ok = (c["depth"] > 0)[:, 0, :, :, 0]
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
        assert not V[:, h, w].any() and not N[:, h, w].any() and not gV[:, h, w].any() and not gN[:, h, w].any()
    # b = 0: the identity pose.  b = 1: products with 0 and +-1 are exact and so are sums with zeros, so each component is
    # ONE rounding of (a coordinate of V) + (a dyadic offset): the float64 result rounded once
    assert torch.equal(gV[0], V[0]) and torch.equal(gN[0], N[0])
    R, t = torch.tensor(R1, dtype=F64), torch.tensor(T1, dtype=F64)
    want_gV = ((V[1].double() @ R.T + t) * ok[1].unsqueeze(-1)).float()
    assert torch.equal(gV[1], want_gV) and torch.equal(gN[1], (N[1].double() @ R.T).float())
    assert torch.equal(gV[1, 2, 3], torch.tensor([2.5, -0.25, 0.5]))


# ---- 1. the wrappers, stage by stage
@pytest.mark.gpu
@pytest.mark.parametrize("channels_first", [False, True], ids=["channels_last", "channels_first"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_wrappers_stage_by_stage(gs, variant, channels_first):
    from gradslam_amd.slam import fusionutils as fu

    c, o32 = _case(variant), _oracle(variant, F32)
    cloud, frame = _cloud(gs, c), _frame(gs, c, channels_first)
    nmax = max(COUNTS)
    kinds = _oracle_warning_kinds(variant)

    active = fu.find_active_map_points(cloud, frame)
    assert active.dtype == torch.int64 and torch.equal(active.cpu(), o32["active"])

    (similar, mask), rec = _recorded(fu.find_similar_map_points, cloud, frame, active, DIST_TH, DOT_TH)
    assert similar.dtype == torch.int64 and mask.dtype == torch.bool
    assert torch.equal(similar.cpu(), o32["similar"])
    assert torch.equal(mask.cpu(), _member(o32["active"], o32["similar"], nmax))
    assert _kinds(rec) == kinds
    assert "dot" in kinds and all("1.25 > 1" in str(w.message) for w in rec if "Max of dot product" in str(w.message))
    if variant == "main":
        assert kinds == ["dot"]
        idx = {k: _row_of(o32["active"], v[0]) for k, v in _HAND.items() if k in ("dist_eq", "dist_below", "dot_eq", "dot_above", "dot_big")}
        m = mask.cpu()
        assert m[idx["dist_below"]] and m[idx["dot_above"]] and m[idx["dot_big"]] and not m[idx["dist_eq"]] and not m[idx["dot_eq"]]
        i1 = {k: _row_of(o32["active"], v[0], b=1) for k, v in _HAND1.items() if k in ("dist_eq", "dist_below")}
        assert m[i1["dist_below"]] and not m[i1["dist_eq"]]
    if variant == "none":
        assert kinds == ["dot", "none"] and similar.shape == (0, 4) and mask.shape == (o32["active"].shape[0],) and not mask.any()
        assert any("total %d active points" % o32["active"].shape[0] in str(w.message) for w in rec)

    unique = fu.find_best_unique_correspondences(cloud, frame, similar)
    assert unique.dtype == torch.int64 and torch.equal(unique.cpu(), o32["unique"])  # row order included: sorted by (b, h, w)
    if variant == "main":
        won = {int(r[1]) for r in unique.cpu() if int(r[0]) == 0}
        assert all(_HAND[n][0] in won for n in _WINNERS) and not any(_HAND[n][0] in won for n in _LOSERS)
    # the active table in place of the similar one: rows that fail a threshold compete as well
    assert torch.equal(_unique_of_active(variant, F32), _unique_of_active(variant, F64))
    of_active = fu.find_best_unique_correspondences(cloud, frame, active)
    assert torch.equal(of_active.cpu(), _unique_of_active(variant, F32))

    # the chained form: device counts, keep flags, no compaction, *d_n < max_rows
    chained, rec = _recorded(fu.find_correspondences, cloud, frame, DIST_TH, DOT_TH)
    assert chained.dtype == torch.int64 and torch.equal(chained.cpu(), o32["unique"])
    assert _kinds(rec) == kinds
    assert all("1.25 > 1" in str(w.message) for w in rec if "Max of dot product" in str(w.message))


def _input_afterwards(c, cloud, out, had_match, inplace):
    """What the object that was passed in holds after fuse_with_map (this file's docstring says why)."""
    if inplace:
        assert out is cloud
        return
    assert out is not cloud and cloud.num_points_per_pointcloud.tolist() == list(COUNTS)
    lists_in = (cloud.points_list, cloud.normals_list, cloud.colors_list, cloud.features_list)
    lists_out = (out.points_list, out.normals_list, out.colors_list, out.features_list)
    for name, li, lo in zip(NAMES, lists_in, lists_out):
        for b in range(B):
            want = lo[b][: COUNTS[b]] if had_match else c[name][b]
            assert li[b].shape[0] == COUNTS[b] and _same_bits(li[b].detach().cpu(), want.detach().cpu()), (name, b)
            assert li[b].data_ptr() != lo[b].data_ptr()  # its own storage


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True], ids=["nograd", "grad"])
@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_fuse_with_map_against_oracle(gs, variant, inplace, grad):
    """fuse_with_map on the oracle's own unique table, so that this stage stands alone.  grad: depth requires grad, which
    takes the merge through its autograd node and the append through mask_select_multi; same bits as without."""
    from gradslam_amd.slam import fusionutils as fu

    c, o32, o64 = _case(variant), _oracle(variant, F32), _oracle(variant, F64)
    table = o32["unique"].to(DEV)

    def run(depth_grad):
        cloud, frame = _cloud(gs, c), _frame(gs, c, depth_grad=depth_grad)
        with torch.enable_grad():
            out = fu.fuse_with_map(cloud, frame, table, SIGMA, inplace=inplace)
        return cloud, out

    cloud, out = run(grad)
    got, counts = _arena_of(out)
    assert out.points_padded.requires_grad == grad
    _check_fusion_values("per-op %s" % variant, c["feats"], o32["unique"], o32["out"], o64["out"], got, counts, got[0].shape[1])
    _input_afterwards(c, cloud, out, table.shape[0] != 0, inplace)
    if grad:
        plain, _ = _arena_of(run(False)[1])
        assert all(_same_bits(a, b) for a, b in zip(got, plain))
    if variant == "none":  # no merge at all: live rows keep their bits, every valid pixel is appended
        assert table.shape[0] == 0 and counts == [COUNTS[b] + H * W - len(HOLES) for b in range(B)]
        for i, name in enumerate(NAMES):
            assert all(_same_bits(got[i][b, : COUNTS[b]], c[name][b]) for b in range(B)), name
    if variant == "b1_only":  # a match in b = 1 only; b = 0 is re-rounded all the same, and takes every valid pixel
        assert {int(r[0]) for r in o32["unique"]} == {1} and counts[0] == COUNTS[0] + H * W - len(HOLES)
        assert counts[1] < COUNTS[1] + H * W - len(HOLES)


@pytest.mark.gpu
@pytest.mark.parametrize("channels_first", [False, True], ids=["channels_last", "channels_first"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_update_map_fusion_against_oracle(gs, variant, channels_first):
    from gradslam_amd.slam import fusionutils as fu

    c, o32, o64 = _case(variant), _oracle(variant, F32), _oracle(variant, F64)
    cloud, frame = _cloud(gs, c), _frame(gs, c, channels_first)
    out, rec = _recorded(fu.update_map_fusion, cloud, frame, DIST_TH, DOT_TH, SIGMA)
    assert _kinds(rec) == _oracle_warning_kinds(variant)
    got, counts = _arena_of(out)
    _check_fusion_values("per-op update %s" % variant, c["feats"], o32["unique"], o32["out"], o64["out"], got, counts, got[0].shape[1])
    _input_afterwards(c, cloud, out, o32["unique"].shape[0] != 0, False)


# ---- 2. the entry points themselves
SENT64 = int.from_bytes(bytes([SENT]) * 8, "little", signed=True)


def _raw(gs, c):
    frame, cloud = _frame(gs, c), _cloud(gs, c)
    r = dict(gV=frame.global_vertex_map, gN=frame.global_normal_map, mp=cloud.points_padded, mn=cloud.normals_padded,
             cc=cloud.features_padded, depth=frame.depth_image)
    assert all(x.is_contiguous() and x.dtype == torch.float32 for x in r.values())
    r["nmax"] = r["mp"].shape[1]
    return r


def _dev_i32(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def _similar(r, rows, n, max_rows, want_max_dot=True):
    from gradslam_amd import _native as nv

    keep = torch.full((rows.shape[0],), SENT, dtype=torch.uint8, device=DEV)
    md = torch.full((1,), float("nan"), device=DEV) if want_max_dot else None
    d_n = _dev_i32(n)
    nv.call("gs_fusion_similar", nv.ptr(rows), nv.ptr(d_n), max_rows, nv.ptr(r["gV"]), nv.ptr(r["gN"]), H, W, nv.ptr(r["mp"]),
            nv.ptr(r["mn"]), r["nmax"], DIST_TH, DOT_TH, nv.ptr(keep), nv.ptr(md), nv.stream())
    torch.cuda.synchronize()
    return keep.cpu(), (None if md is None else int(_bits(md.cpu())))


def _unique(r, rows, keep, n, max_rows):
    from gradslam_amd import _native as nv

    npix = B * H * W
    out = torch.full((npix, 4), SENT64, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(nv.ws_bytes("gs_fusion_unique_ws_bytes", B, H, W), dtype=torch.uint8, device=DEV)
    d_n = _dev_i32(n)
    nv.call("gs_fusion_unique", nv.ptr(rows), nv.ptr(keep), nv.ptr(d_n), max_rows, nv.ptr(r["gV"]), B, H, W, nv.ptr(r["mp"]),
            nv.ptr(r["cc"]), r["nmax"], nv.ptr(out), nv.ptr(cnt), nv.ptr(ws), ws.numel(), nv.stream())
    torch.cuda.synchronize()
    out, cnt = out.cpu(), int(cnt)
    assert 0 <= cnt <= npix and bool((out[cnt:] == SENT64).all()), "rows behind the count"
    return out[:cnt]


def _new_mask(depth, rows, n, max_rows):
    from gradslam_amd import _native as nv

    mask = torch.full((B, H, W), SENT, dtype=torch.uint8, device=DEV)
    d_n = None if rows is None else _dev_i32(n)
    nv.call("gs_fusion_new_mask", nv.ptr(depth), nv.ptr(rows), nv.ptr(d_n), max_rows, B, H, W, nv.ptr(mask), nv.stream())
    torch.cuda.synchronize()
    return mask.cpu()


def _padded(table, n_extra, row):
    """table + n_extra copies of one of its rows behind it: slack that a kernel which minds *d_n never reads, and valid
    indices for one that does not."""
    return torch.cat([table, row.view(1, 4).expand(n_extra, 4)], 0).contiguous().to(DEV)


@pytest.mark.gpu
def test_raw_similar(gs):
    c, o32 = _case("main"), _oracle("main", F32)
    r = _raw(gs, c)
    act = o32["active"]
    P, nmax = act.shape[0], r["nmax"]
    want = _member(act, o32["similar"], nmax).to(torch.uint8)
    # *d_n < max_rows: the slack rows are dist_below's (similar: a kernel that read them would write 1 over the sentinel)
    rows = _padded(act, 37, act[_row_of(act, _HAND["dist_below"][0])])
    keep, md = _similar(r, rows, P, P + 37)
    assert torch.equal(keep[:P], want) and bool((keep[P:] == SENT).all())
    assert md == int(_bits(torch.tensor([1.25])))
    keep2, _ = _similar(r, rows, P, P + 37, want_max_dot=False)  # max_dot = NULL
    assert torch.equal(keep2, keep)
    # the largest dot product is exactly 1.0: nothing is published (the kernel publishes above 1 only), +0.0 stays
    keep3, md = _similar(_raw(gs, _unit_dot_case()), rows, P, P + 37)
    assert torch.equal(keep3, keep) and md == 0
    # nothing to do: nothing written but max_dot = 0
    for n, max_rows in ((0, P + 37), (P, 0), (0, 0)):
        keep4, md = _similar(r, rows, n, max_rows)
        assert bool((keep4 == SENT).all()) and md == 0, (n, max_rows)


@pytest.mark.gpu
def test_raw_unique(gs):
    c, o32 = _case("main"), _oracle("main", F32)
    r = _raw(gs, c)
    act, sim, want = o32["active"], o32["similar"], o32["unique"]
    P, S = act.shape[0], sim.shape[0]
    # the slack rows are dist_eq's (c = 3, not similar): let in, they would take pixel (2, 3) from dist_below (c = 1)
    slack = act[_row_of(act, _HAND["dist_eq"][0])]
    flags = torch.cat([_member(act, sim, r["nmax"]).to(torch.uint8), torch.ones(37, dtype=torch.uint8)]).to(DEV)
    by_flags = _unique(r, _padded(act, 37, slack), flags, P, P + 37)
    compacted = _unique(r, _padded(sim, 37, slack), None, S, S + 37)
    assert torch.equal(by_flags, want) and torch.equal(compacted, want)
    assert _unique(r, _padded(sim, 37, slack), None, 0, S + 37).shape[0] == 0
    assert _unique(r, _padded(sim, 37, slack), None, S, 0).shape[0] == 0
    # the order of the table does not matter; among bit-equal keys the smallest n wins wherever it stands
    g = torch.Generator().manual_seed(5)
    for order in (torch.arange(S - 1, -1, -1), torch.randperm(S, generator=g), torch.randperm(S, generator=g)):
        assert torch.equal(_unique(r, sim[order].contiguous().to(DEV), None, S, S), want)
    order = torch.randperm(P, generator=g)
    assert torch.equal(_unique(r, act[order].contiguous().to(DEV), flags[:P].cpu()[order].to(DEV), P, P), want)


@pytest.mark.gpu
def test_raw_new_mask(gs):
    c, o32 = _case("main"), _oracle("main", F32)
    depth = c["depth"].to(DEV)
    uniq = o32["unique"]
    U = uniq.shape[0]
    # the slack rows name pixel (0, 0) of b = 0, which no map point reaches: a kernel that read them would clear it
    rows = _padded(uniq, 5, torch.tensor([0, 0, 0, 0]))
    mask = _new_mask(depth, rows, U, U + 5)
    for b in range(B):
        assert [tuple(p) for p in mask[b].nonzero().tolist()] == o32["appended"][b], b
    assert bool((mask <= 1).all()) and mask[0, 0, 0] == 1
    for h, w in HOLES:  # (1, 5) is the hole that over_hole projects to
        assert not mask[:, h, w].any()
    valid = (c["depth"] > 0)[:, 0, :, :, 0].to(torch.uint8)
    assert torch.equal(_new_mask(depth, None, 0, 0), valid)
    assert torch.equal(_new_mask(depth, rows, U, 0), valid) and torch.equal(_new_mask(depth, rows, 0, U + 5), valid)
    # the oracle's rule is depth > 0 (oracle/fusion.py, reference valid_depth_mask): false for -1 and for NaN, true for +inf
    odd = c["depth"].clone()
    spots = {(0, 0): -1.0, (0, 7): float("nan"), (5, 0): float("inf")}
    for (h, w), v in spots.items():
        assert (h, w) in o32["appended"][0]
        odd[0, 0, h, w, 0] = v
    rule = (odd > 0)[:, 0, :, :, 0]
    assert [bool(rule[0, h, w]) for h, w in spots] == [False, False, True]
    got = _new_mask(odd.to(DEV), rows, U, U + 5)
    want = mask.clone()
    want[0, 0, 0] = want[0, 0, 7] = 0
    assert torch.equal(got, want) and got[0, 5, 0] == 1
    assert torch.equal(_new_mask(odd.to(DEV), None, 0, 0), rule.to(torch.uint8))


# ---- 3. a table longer than one grid pass
@pytest.mark.gpu
def test_table_longer_than_one_grid_pass(gs):
    """b = 0's map is k copies of main's rows, so that the active table exceeds 2048 x 256 rows by more than a block: the rows
    beyond are reached by the kernels' stride loops only.  Zero flips, and the assertions name rows beyond the first pass."""
    from gradslam_amd.slam import fusionutils as fu

    k = _long_k()
    c, o32 = _tiled_case(k), _oracle("main", F32)
    active, similar, unique = _tiled_tables(k)
    P, nmax = active.shape[0], k * COUNTS[0]
    assert P >= GRID_PASS + 256
    cloud, frame = _cloud(gs, c), _frame(gs, c)
    last = {name: _row_of(active, (k - 1) * COUNTS[0] + _HAND[name][0]) for name in ("dist_below", "dot_above", "dist_eq", "dot_eq")}
    assert all(i > GRID_PASS for i in last.values())

    got_active = fu.find_active_map_points(cloud, frame)
    assert torch.equal(got_active.cpu(), active)
    (got_similar, mask), rec = _recorded(fu.find_similar_map_points, cloud, frame, got_active, DIST_TH, DOT_TH)
    mask = mask.cpu()
    assert mask.shape == (P,)
    assert mask[last["dist_below"]] and mask[last["dot_above"]] and not mask[last["dist_eq"]] and not mask[last["dot_eq"]]
    skeys = set(_key(got_similar.cpu(), nmax)[-700:].tolist())  # the last copy's rows and b = 1's
    key_of = lambda name: (k - 1) * COUNTS[0] + _HAND[name][0]
    assert key_of("dist_below") in skeys and key_of("dot_above") in skeys and key_of("dist_eq") not in skeys and key_of("dot_eq") not in skeys
    assert torch.equal(mask[GRID_PASS:], _member(active, similar, nmax)[GRID_PASS:]), "rows beyond the first grid pass"
    assert torch.equal(got_similar.cpu(), similar) and torch.equal(mask, _member(active, similar, nmax))
    assert _kinds(rec) == ["dot"]

    chained, _ = _recorded(fu.find_correspondences, cloud, frame, DIST_TH, DOT_TH)
    assert torch.equal(chained.cpu(), unique)

    # the unique passes and the clearing pass where ONLY a row beyond the first pass holds a pixel (the late table)
    late, r = _late_table(k), _raw(gs, c)
    assert r["nmax"] == nmax
    late_dev = late.contiguous().to(DEV)
    assert torch.equal(_unique(r, late_dev, None, late.shape[0], late.shape[0]), _late_unique(k))
    valid = (c["depth"] > 0)[:, 0, :, :, 0]
    for table in (similar, late):
        want = valid.clone()
        want[table[:, 0], table[:, 2], table[:, 3]] = False
        got = _new_mask(r["depth"], table.contiguous().to(DEV), table.shape[0], table.shape[0])
        assert torch.equal(got, want.to(torch.uint8))
    assert valid[0, LATE_PIX[0], LATE_PIX[1]] and got[0, LATE_PIX[0], LATE_PIX[1]] == 0

    # the merge: scatter_match_k runs over the unique table only, the map rows beyond one pass are merge_k's
    out = fu.fuse_with_map(cloud, frame, unique.to(DEV), SIGMA)
    got, counts = _arena_of(out)
    _check_fusion_values("per-op long", c["feats"], unique, _tiled_fused(k, F32), _tiled_fused(k, F64), got, counts, got[0].shape[1])
