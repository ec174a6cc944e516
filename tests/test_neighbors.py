"""Neighbours (kernel family N): exact K nearest neighbours of padded clouds, the adjoint of their distances, normals from the
neighbourhoods' covariances, and the two outlier filters of Pointclouds.

Every oracle is restated here in numpy / Python integers.  Keys are compared bit for bit (int64, KEY_NONE padding and the rows
beyond the counts included), under every setting of the grid knob: the search's result is a property of the key set alone.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops
from tests.helpers import exact_sum_f32, f32_to_int, int_to_f32

DEV = "cuda:0"
U = 2.0 ** -24  # unit roundoff of fp32
KEY_NONE = -1
SENTINEL = 0x5A5A5A5A5A5A5A5A
KS = (1, 3, 16, 32)
GRIDS = (1, 2, 5, 0)
NEW_SYMBOLS = {"gs_set_knn_grid": 1, "gs_knn_ws_bytes": 4, "gs_knn": 12, "gs_knn_backward_ws_bytes": 4, "gs_knn_backward": 15,
               "gs_knn_normals": 14}


def _align256(n):
    return -(-n // 256) * 256


def _cells(n, K):
    per = 8 if K <= 8 else (16 if K <= 16 else 32)
    g = 1
    while g < 128 and per * g * g < n:
        g += 1
    return g ** 3


# ------------------------------------------------------------------ CPU: ABI and error contracts
def test_neighbor_symbols_load():
    lib = nv.lib()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
    assert lib.gs_abi_version() == 3
    for name in ("knn_raw", "knn", "knn_normals_raw", "_KnnFn"):
        assert hasattr(ops, name), name
    for name in ("knn", "estimate_normals", "remove_radius_outliers", "remove_statistical_outliers"):
        assert hasattr(gs.Pointclouds, name), name


@pytest.mark.parametrize("B,Ns,Nt,K", [(1, 1, 1, 1), (1, 130, 49, 8), (2, 5000, 3000, 9), (3, 327, 1000, 32), (1, 307200, 307200, 16)])
def test_knn_workspace_sizes_follow_the_layout(B, Ns, Nt, K):
    """The layouts documented in include/gradslam_hip.h, piece by piece, each rounded up to 256 bytes."""
    lib = nv.lib()
    fwd = _align256(16 * B * Nt) + 2 * _align256(4 * B * Ns) + _align256(4 * B * Nt) + _align256(B * 2 * 3 * 129 * 4)
    fwd += _align256(32 * B) + _align256(B * 2 * 3 * 128 * 4) + 2 * _align256(4 * B * _cells(Nt, K))
    assert lib.gs_knn_ws_bytes(B, Ns, Nt, K) == fwd
    assert lib.gs_knn_backward_ws_bytes(B, Ns, Nt, K) == _align256(48 * B * Nt) + _align256(4 * B * Nt) + _align256(4)


def test_knn_workspace_queries_return_zero_for_bad_arguments():
    lib = nv.lib()
    for fn in (lib.gs_knn_ws_bytes, lib.gs_knn_backward_ws_bytes):
        assert fn(1, 10, 7, 8) > 0
        for bad in ((0, 10, 7, 8), (-1, 10, 7, 8), (1, 0, 7, 8), (1, -3, 7, 8), (1, 10, 0, 8), (1, 10, -1, 8), (1, 10, 7, 0),
                    (1, 10, 7, 33), (1, 10, 7, -1)):
            assert fn(*bad) == 0, bad


def test_knn_refuses_bad_arguments_before_any_device_work():
    """NULL pointers and bad sizes return -1, a missing or short workspace -2 (the pointers below are never read: every check
    happens on the host before the first launch)."""
    lib = nv.lib()
    P = 4096  # a non-NULL stand-in
    ok = [P, P, 10, P, P, 7, 1, 8, P, P, 1 << 24, None]
    for pos in (0, 1, 3, 4, 8):  # src, src_counts, tgt, tgt_counts, keys
        args = list(ok)
        args[pos] = None
        assert lib.gs_knn(*args) == -1, pos
    for pos, bad in ((2, 0), (2, -4), (5, 0), (6, 0), (6, -1), (7, 0), (7, 33)):  # Ns_max, Nt_max, B, K
        args = list(ok)
        args[pos] = bad
        assert lib.gs_knn(*args) == -1, (pos, bad)
    assert b"gs_knn" in lib.gs_last_error()
    args = list(ok)
    args[9], args[10] = None, 0
    assert lib.gs_knn(*args) == -2
    args = list(ok)
    args[10] = lib.gs_knn_ws_bytes(1, 10, 7, 8) - 1
    assert lib.gs_knn(*args) == -2
    assert b"gs_knn:" in lib.gs_last_error()

    okb = [P, P, 10, P, P, 7, 1, 8, P, P, P, 2 * P, P, 1 << 24, None]
    for pos in (0, 1, 3, 4, 8, 9, 10, 11):
        args = list(okb)
        args[pos] = None
        assert lib.gs_knn_backward(*args) == -1, pos
    for pos, bad in ((2, 0), (5, -1), (6, 0), (7, 0), (7, 33)):
        args = list(okb)
        args[pos] = bad
        assert lib.gs_knn_backward(*args) == -1, (pos, bad)
    args = list(okb)
    args[11] = args[10]  # one buffer for both adjoints
    assert lib.gs_knn_backward(*args) == -1
    args = list(okb)
    args[12], args[13] = None, 0
    assert lib.gs_knn_backward(*args) == -2
    args = list(okb)
    args[13] = lib.gs_knn_backward_ws_bytes(1, 10, 7, 8) - 1
    assert lib.gs_knn_backward(*args) == -2
    assert b"gs_knn_backward" in lib.gs_last_error()

    okn = [P, P, 10, P, P, 7, 1, 8, P, 0, None, P, None, None]
    for pos in (0, 1, 3, 4, 8, 11):
        args = list(okn)
        args[pos] = None
        assert lib.gs_knn_normals(*args) == -1, pos
    for pos, bad in ((2, 0), (5, 0), (6, 0), (7, 0), (7, 33), (9, -1), (9, 3), (9, 1), (9, 2)):  # modes 1, 2 without `orient`
        args = list(okn)
        args[pos] = bad
        assert lib.gs_knn_normals(*args) == -1, (pos, bad)
    assert b"gs_knn_normals" in lib.gs_last_error()


def test_neighbor_front_error_contracts():
    pts = torch.rand(2, 10, 3)
    cnt = torch.full((2,), 10, dtype=torch.int32)
    pc = gs.Pointclouds(pts)
    with pytest.raises(RuntimeError, match="HIP"):  # no CPU fallback
        ops.knn_raw(pts, pts, cnt, cnt, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.knn(pts, pts, cnt, cnt, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        pc.knn(4)
    with pytest.raises(RuntimeError, match="HIP"):
        pc.estimate_normals(8)
    with pytest.raises(RuntimeError, match="HIP"):
        pc.remove_radius_outliers(0.1, 3)
    with pytest.raises(RuntimeError, match="HIP"):
        pc.remove_statistical_outliers(4, 2.0)
    for K in (0, 33, -1, 2.0, True):
        with pytest.raises((ValueError, RuntimeError)) as e:
            pc.knn(K)
        assert e.type is ValueError or "HIP" in str(e.value)
    for K in (0, 2, 33):
        with pytest.raises(ValueError):
            pc.estimate_normals(K)
    with pytest.raises(ValueError):
        pc.estimate_normals(8, orient="inwards")
    with pytest.raises(ValueError):
        pc.estimate_normals(8, orient="normals")  # the cloud has none
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.remove_radius_outliers(radius, 3)
    for m in (0, 33, 1.5):
        with pytest.raises(ValueError):
            pc.remove_radius_outliers(0.1, m)
    for K in (0, 32):
        with pytest.raises(ValueError):
            pc.remove_statistical_outliers(K, 2.0)
    with pytest.raises(ValueError):
        pc.remove_statistical_outliers(4, float("nan"))
    with pytest.raises(ValueError):
        gs.Pointclouds().knn(4)
    empty = gs.Pointclouds()
    assert empty.remove_radius_outliers(0.1, 3) is empty and empty.remove_statistical_outliers(4, 2.0) is empty
    assert empty.estimate_normals(8) is empty


def test_knn_unpack_on_hand_cases():
    d = np.array([0.0, 1.5, 3.0e-39], np.float32)
    keys = (d.view(np.uint32).astype(np.int64) << 32) | np.array([7, 0, 2 ** 31 - 1], np.int64)
    keys = torch.from_numpy(np.concatenate([keys, [KEY_NONE]]))
    d2, idx = ops.knn_unpack(keys)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64
    assert np.array_equal(d2.numpy().view(np.uint32), np.concatenate([d, [0.0]]).astype(np.float32).view(np.uint32))
    assert idx.tolist() == [7, 0, 2 ** 31 - 1, -1]


# ------------------------------------------------------------------ the oracle and the scenes
def pair_d2(s, t):
    """All pairs in float32: (dx*dx + dy*dy) + dz*dz, no fused operation (numpy has none)."""
    d = s[:, None, :] - t[None, :, :]
    assert d.dtype == np.float32
    sq = d * d
    d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    assert d2.dtype == np.float32
    return d2


def oracle_keys(src, tgt, src_counts, tgt_counts, K):
    """(B, Ns, K) int64: per row below its count the first K of the targets sorted by (d2, j); KEY_NONE everywhere else."""
    B, Ns = src.shape[:2]
    out = np.full((B, Ns, K), KEY_NONE, np.int64)
    for b in range(B):
        ns, nt = int(src_counts[b]), int(tgt_counts[b])
        if ns == 0 or nt == 0:
            continue
        d2 = pair_d2(src[b, :ns], tgt[b, :nt])
        jj = np.broadcast_to(np.arange(nt, dtype=np.int64), d2.shape)
        order = np.lexsort((jj, d2), axis=-1)[:, :K]
        dk = np.take_along_axis(d2, order, axis=1)
        out[b, :ns, : order.shape[1]] = (dk.view(np.uint32).astype(np.int64) << 32) | order
    return out


def _pad(x, cap):
    """(n, 3) -> (cap, 3) padded with NaN: rows at or beyond a count are never read."""
    out = np.full((cap, 3), np.nan, np.float32)
    out[: len(x)] = x
    return out


def _surface(rs, h, w):
    """An image-ordered cloud: a smooth depth surface back-projected pixel by pixel, row-major."""
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = 2.0 + 0.3 * np.sin(u / 7.0) + 0.2 * np.cos(v / 5.0) + 0.002 * rs.rand(h, w)
    return np.stack([(u - w / 2) * z / 60.0, (v - h / 2) * z / 60.0, z], -1).reshape(-1, 3).astype(np.float32)


def _lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


@lru_cache(maxsize=None)
def scene(name):
    """name -> (src (B,Ns,3), tgt (B,Nt,3) or None for the self-query, src_counts, tgt_counts, extra Ks)."""
    rs = np.random.RandomState(sum(map(ord, name)))
    one = lambda s, t, ks=(): (s[None], None if t is None else t[None], np.array([len(s)], np.int32),
                               np.array([len(s) if t is None else len(t)], np.int32), ks)
    if name == "random":
        return one(rs.rand(1000, 3).astype(np.float32), rs.rand(777, 3).astype(np.float32))
    if name == "self_image_order":
        return one(_surface(rs, 30, 50), None)
    if name == "self_shuffled":
        return one(_surface(rs, 30, 50)[rs.permutation(1500)], None)
    if name == "lattice":  # massive exact ties: the lowest row must win
        lat = _lattice(12)
        q = np.concatenate([lat[rs.permutation(len(lat))[:400]], lat[rs.permutation(len(lat))[:400]] + np.float32(0.5),
                            lat[:200] + np.array([0.5, 0.0, 0.0], np.float32)])
        return one(q, lat[rs.permutation(len(lat))])
    if name == "lattice_duplicated":
        lat = _lattice(12)
        q = np.concatenate([lat[:300], lat[-300:] + np.float32(0.5)])
        return one(q, np.repeat(lat, 2, axis=0)[rs.permutation(2 * len(lat))])
    if name == "few_targets":  # tgt_counts = 5 with K = 8, and tgt_counts = 0, inside larger padded buffers
        s = np.stack([_pad(rs.rand(50, 3), 64), _pad(rs.rand(64, 3), 64)])
        t = np.stack([_pad(rs.rand(5, 3), 40), _pad(np.zeros((0, 3)), 40)])
        return s, t, np.array([50, 64], np.int32), np.array([5, 0], np.int32), (8,)
    if name == "ragged_batch":
        s = np.stack([_pad(rs.rand(1000, 3), 1000), _pad(rs.rand(1, 3), 1000), _pad(np.zeros((0, 3)), 1000)])
        t = np.stack([_pad(np.zeros((0, 3)), 777), _pad(rs.rand(777, 3), 777), _pad(rs.rand(300, 3), 777)])
        return s, t, np.array([1000, 1, 0], np.int32), np.array([0, 777, 300], np.int32), ()
    if name == "all_targets_equal":
        return one(rs.rand(200, 3).astype(np.float32), np.tile(np.array([[0.25, -1.0, 3.0]], np.float32), (300, 1)))
    if name == "collinear":
        t = np.outer(rs.rand(500), np.array([1.0, 2.0, -0.5])).astype(np.float32)
        return one(np.concatenate([t[:100], rs.rand(200, 3).astype(np.float32)]), t)
    if name == "planar":
        t = np.concatenate([rs.rand(900, 2), np.full((900, 1), 0.75)], 1).astype(np.float32)
        return one(np.concatenate([t[:100], rs.rand(200, 3).astype(np.float32)]), t)
    if name == "two_clusters":  # K = 32 > 20: the box must cross the empty cells between the clusters
        a = (rs.rand(20, 3) * 0.02).astype(np.float32)
        t = np.concatenate([a, a[::-1] + np.array([1.0, 0.0, 0.0], np.float32)])
        return one(np.concatenate([t, rs.rand(30, 3).astype(np.float32)]), t[rs.permutation(40)])
    if name == "far_query":  # one query 1000 extents away from a 2000-row cluster
        t = rs.rand(2000, 3).astype(np.float32)
        return one(np.concatenate([np.array([[1000.0, 1000.0, -1000.0]], np.float32), t[:50]]), t)
    if name == "outside_the_box":  # queries beyond the targets' bounding box on every side, edge and corner
        t = rs.rand(1500, 3).astype(np.float32)
        dirs = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.float32)
        q = np.float32(0.5) + dirs[None] * np.array([0.6, 1.5, 40.0], np.float32)[:, None, None]
        return one((q.reshape(-1, 3) + (rs.rand(81, 3) * 0.2).astype(np.float32)).astype(np.float32), t)
    if name == "full_4096":  # several blocks of queries
        return one(rs.rand(4096, 3).astype(np.float32), (rs.rand(4096, 3) * np.array([1.0, 0.5, 0.1])).astype(np.float32))
    raise KeyError(name)


SCENES = ["random", "self_image_order", "self_shuffled", "lattice", "lattice_duplicated", "few_targets", "ragged_batch",
          "all_targets_equal", "collinear", "planar", "two_clusters", "far_query", "outside_the_box", "full_4096"]


@lru_cache(maxsize=None)
def scene_oracle(name):
    """The oracle's keys at the largest K; a smaller K is a prefix of it."""
    src, tgt, cs, ct, extra = scene(name)
    return oracle_keys(src, src if tgt is None else tgt, cs, ct, max(KS + tuple(extra)))


def gpu_keys(src, tgt, cs, ct, K):
    """knn_raw into a buffer pre-filled with a sentinel: every element must be written."""
    s = torch.from_numpy(src).to(DEV)
    t = s if tgt is None else torch.from_numpy(tgt).to(DEV)
    out = torch.full((src.shape[0], src.shape[1], K), SENTINEL, dtype=torch.int64, device=DEV)
    keys = ops.knn_raw(s, t, torch.from_numpy(cs).to(DEV), torch.from_numpy(ct).to(DEV), K, out=out)
    assert keys.data_ptr() == out.data_ptr()
    return keys


# ------------------------------------------------------------------ GPU: the keys
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_keys_equal_the_all_pairs_oracle_under_every_grid(name):
    src, tgt, cs, ct, extra = scene(name)
    want_all = scene_oracle(name)
    lib = nv.lib()
    try:
        for K in KS + tuple(extra):
            want = torch.from_numpy(np.ascontiguousarray(want_all[..., :K]))
            for g in GRIDS:
                lib.gs_set_knn_grid(g)
                got = gpu_keys(src, tgt, cs, ct, K).cpu()
                assert not bool((got == SENTINEL).any()), (K, g)
                assert torch.equal(got, want), (name, K, g, int((got != want).sum()))
    finally:
        lib.gs_set_knn_grid(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "self_shuffled", "lattice_duplicated", "ragged_batch"])
def test_first_key_equals_the_one_nearest_neighbour_search(name):
    """K = 1 against the product's K = 1 path (gs_knn1), per batch element."""
    src, tgt, cs, ct, _ = scene(name)
    tgt = src if tgt is None else tgt
    keys = gpu_keys(src, None if tgt is src else tgt, cs, ct, 1)
    for b in range(src.shape[0]):
        ns, nt = int(cs[b]), int(ct[b])
        if ns == 0 or nt == 0:
            assert bool((keys[b] == KEY_NONE).all())
            continue
        one = ops.knn1_raw(torch.from_numpy(src[b, :ns]).to(DEV), torch.from_numpy(tgt[b, :nt]).to(DEV))
        assert torch.equal(keys[b, :ns, 0], one), (name, b)


@pytest.mark.gpu
def test_keys_do_not_depend_on_the_row_order_of_either_cloud_nor_on_the_run():
    src, tgt, cs, ct, _ = scene("random")
    rs = np.random.RandomState(5)
    ps, pt = rs.permutation(src.shape[1]), rs.permutation(tgt.shape[1])
    base = gpu_keys(src, tgt, cs, ct, 16)
    assert torch.equal(base, gpu_keys(src, tgt, cs, ct, 16))
    moved = gpu_keys(np.ascontiguousarray(src[:, ps]), np.ascontiguousarray(tgt[:, pt]), cs, ct, 16).cpu().numpy()
    # the same distances for the same source, and the same neighbours once the target rows are mapped back
    back = base.cpu().numpy()[:, ps]
    assert np.array_equal(moved >> 32, back >> 32)
    same_d = (back >> 32)[..., 1:] == (back >> 32)[..., :-1]
    assert not same_d.any()  # no ties in this scene: the neighbour lists are then the same as sets AND in order
    assert np.array_equal(pt[moved & 0xFFFFFFFF], back & 0xFFFFFFFF)


# ------------------------------------------------------------------ GPU: the reverse pass
def backward_oracle(src, tgt, ns, nt, keys, g):
    """One batch element.  g_src: float32 in slot order.  g_tgt: the exact integer sum of the fp32 terms, rounded once."""
    K = keys.shape[-1]
    g_src = np.zeros((src.shape[0], 3), np.float32)
    g_tgt = np.zeros((tgt.shape[0], 3), np.float32)
    idx = (keys & 0xFFFFFFFF).astype(np.int64)
    valid = (keys != KEY_NONE) & (idx < nt)
    valid[ns:] = False
    acc = np.zeros((src.shape[0], 3), np.float32)
    terms = [[[] for _ in range(3)] for _ in range(tgt.shape[0])]
    lo, hi = np.inf, 0.0
    for k in range(K):
        j = np.where(valid[:, k], idx[:, k], 0)
        with np.errstate(invalid="ignore"):
            c = np.float32(2.0) * g[:, k]
            v = c[:, None] * (src - tgt[j])
        assert v.dtype == np.float32
        acc = np.where(valid[:, k, None], acc + v, acc)
        rows = np.nonzero(valid[:, k])[0]
        ints = f32_to_int((-v[rows]).view(np.uint32))
        for n, i in enumerate(rows):
            for c3 in range(3):
                terms[j[i]][c3].append(ints[3 * n + c3])
        nz = np.abs(v[rows][v[rows] != 0])
        if nz.size:
            lo, hi = min(lo, float(nz.min())), max(hi, float(nz.max()))
    g_src[:ns] = acc[:ns]
    for j in range(nt):
        for c3 in range(3):
            g_tgt[j, c3] = int_to_f32(sum(terms[j][c3]))
    return g_src, g_tgt, lo, hi


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("name,K", [("random", 8), ("self_shuffled", 16), ("lattice", 8), ("ragged_batch", 3)])
def test_reverse_pass_is_bitwise_the_stated_sums(name, K):
    """g_src: ((0 + v_0) + v_1) + ... in float32.  g_tgt: the exact sum rounded once.  The kernel carries at least 102 - lg
    binary places below the largest |v| of the call, lg = ceil(log2(Ns_max K)) <= 17 here, i.e. >= 85 places; the terms of
    these scenes span fewer than 2^40 in magnitude (asserted), so nothing is truncated and the comparison is bit for bit."""
    src, tgt, cs, ct, _ = scene(name)
    tgt_np = src if tgt is None else tgt
    keys_np = np.ascontiguousarray(scene_oracle(name)[..., :K])
    rs = np.random.RandomState(11)
    g = ((0.5 + rs.rand(*keys_np.shape)) * rs.choice([-1.0, 1.0], keys_np.shape)).astype(np.float32)
    s = torch.from_numpy(src).to(DEV)
    t = s if tgt is None else torch.from_numpy(tgt).to(DEV)
    csd, ctd = torch.from_numpy(cs).to(DEV), torch.from_numpy(ct).to(DEV)
    keys, gd = torch.from_numpy(keys_np).to(DEV), torch.from_numpy(g).to(DEV)
    g_src, g_tgt = ops.knn_backward_raw(s, t, csd, ctd, keys, gd)
    lo, hi = np.inf, 0.0
    for b in range(src.shape[0]):
        ws, wt, l, h = backward_oracle(src[b], tgt_np[b], int(cs[b]), int(ct[b]), keys_np[b], g[b])
        lo, hi = min(lo, l), max(hi, h)
        assert np.array_equal(g_src[b].cpu().numpy().view(np.uint32), ws.view(np.uint32)), (name, b)
        assert np.array_equal(g_tgt[b].cpu().numpy().view(np.uint32), wt.view(np.uint32)), (name, b)
    assert hi < lo * 2.0 ** 40
    again = ops.knn_backward_raw(s, t, csd, ctd, keys, gd)
    assert torch.equal(bits(again[0]), bits(g_src)) and torch.equal(bits(again[1]), bits(g_tgt))
    with_det = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(not with_det)
    try:  # one path: the switch changes nothing
        other = ops.knn_backward_raw(s, t, csd, ctd, keys, gd)
    finally:
        torch.use_deterministic_algorithms(with_det)
    assert torch.equal(bits(other[0]), bits(g_src)) and torch.equal(bits(other[1]), bits(g_tgt))


@pytest.mark.gpu
def test_target_adjoint_does_not_depend_on_the_order_of_the_query_rows():
    src, tgt, cs, ct, _ = scene("random")
    K = 16
    keys_np = np.ascontiguousarray(scene_oracle("random")[..., :K])
    rs = np.random.RandomState(12)
    g = rs.randn(*keys_np.shape).astype(np.float32)
    p = rs.permutation(src.shape[1])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    a = ops.knn_backward_raw(dev(src), dev(tgt), dev(cs), dev(ct), dev(keys_np), dev(g))
    b = ops.knn_backward_raw(dev(src[:, p]), dev(tgt), dev(cs), dev(ct), dev(keys_np[:, p]), dev(g[:, p]))
    assert torch.equal(bits(a[1]), bits(b[1]))
    assert torch.equal(bits(a[0][:, p]), bits(b[0]))


@pytest.mark.gpu
def test_reverse_pass_with_non_finite_upstream_entries():
    """g_d2 = NaN at one slot, +inf at another, +inf and -inf at two slots of one target.  A target element that receives a
    non-finite term holds what a float sum of its terms gives; every other element holds the bits of the same call with those
    four entries set to zero (non-finite terms stay out of the maximum, a zero term adds nothing to an exact sum)."""
    B, Ns, Nt, K = 2, 300, 70, 3
    rs = np.random.RandomState(23)
    cs, ct = np.array([300, 137], np.int32), np.array([41, 70], np.int32)
    src = np.stack([_pad(rs.rand(n, 3), Ns) for n in cs])
    tgt = np.stack([_pad(rs.rand(n, 3), Nt) for n in ct])
    keys = oracle_keys(src, tgt, cs, ct, K)
    idx = keys & 0xFFFFFFFF
    g = ((0.5 + rs.rand(B, Ns, K)) * rs.choice([-1.0, 1.0], (B, Ns, K))).astype(np.float32)
    # the pair: two slots of the target that the last slot of batch element 0 (row 299: another block) points to, whose
    # coordinate differences agree in sign on some axes (there both infinities meet) and not on the others
    j_pair = int(idx[0, 299, K - 1])
    slots = [tuple(s) for s in np.argwhere(idx[0] == j_pair)]
    up = (src[0, :, None, :] - tgt[0][idx[0]]) > 0
    pair = next(((p, q) for p in slots for q in slots if p != q and 0 < (up[p] == up[q]).sum() < 3), None)
    assert pair is not None, "no two slots of target %d agree in sign on some axes only: choose another seed" % j_pair
    bad = {(0,) + pair[0]: np.inf, (0,) + pair[1]: -np.inf, (0, 70, 1): np.nan, (1, 130, 0): np.inf}
    rows = {(0, j_pair), (0, int(idx[0, 70, 1])), (1, int(idx[1, 130, 0]))}
    assert len(bad) == 4 and len(rows) == 3
    g_bad, g_zero = g.copy(), g.copy()
    for at, val in bad.items():
        g_bad[at], g_zero[at] = val, 0.0
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    args = (dev(src), dev(tgt), dev(cs), dev(ct), dev(keys))
    got_src, got_tgt = (x.cpu().numpy() for x in ops.knn_backward_raw(*args, dev(g_bad)))
    ref_src, ref_tgt = (x.cpu().numpy() for x in ops.knn_backward_raw(*args, dev(g_zero)))
    hit = np.zeros((B, Nt, 3), bool)
    for b in range(B):
        ns, nt = int(cs[b]), int(ct[b])
        with np.errstate(invalid="ignore"):
            v = (np.float32(2.0) * g_bad[b, :ns])[..., None] * (src[b, :ns, None, :] - tgt[b][idx[b, :ns]])  # (ns, K, 3)
        assert v.dtype == np.float32 and (idx[b, :ns] < nt).all()
        for j in np.unique(idx[b, :ns][~np.isfinite(v).all(-1)]):
            terms = -v[idx[b, :ns] == j]  # (slots of j, 3)
            for c in range(3):
                if not np.isfinite(terms[:, c]).all():
                    hit[b, j, c] = True
                    want, have = exact_sum_f32(terms[:, c]), got_tgt[b, j, c]
                    assert (np.isnan(want) and np.isnan(have)) or want.view(np.uint32) == have.view(np.uint32), (b, j, c, want, have)
    assert {(b, j) for b, j, _ in np.argwhere(hit)} == rows and hit.sum() == 9  # (no coordinate difference is zero)
    assert np.isnan(got_tgt[hit]).any() and np.isposinf(got_tgt[hit]).any() and np.isneginf(got_tgt[hit]).any()
    assert np.isnan(got_tgt[0, j_pair]).any() and np.isinf(got_tgt[0, j_pair]).any()
    assert np.array_equal(got_tgt.view(np.uint32)[~hit], ref_tgt.view(np.uint32)[~hit])
    touched = np.zeros((B, Ns), bool)
    for b, i, _ in bad:
        touched[b, i] = True
    assert (~np.isfinite(got_src[touched])).all() and np.array_equal(got_src.view(np.uint32)[~touched], ref_src.view(np.uint32)[~touched])


@pytest.mark.gpu
def test_autograd_through_a_self_query_adds_both_roles():
    src, _, cs, _, _ = scene("self_shuffled")
    K = 8
    pts = torch.from_numpy(src).to(DEV).requires_grad_(True)
    cnt = torch.from_numpy(cs).to(DEV)
    d2, idx = ops.knn(pts, pts, cnt, cnt, K)
    want = torch.from_numpy(np.ascontiguousarray(scene_oracle("self_shuffled")[..., :K])).to(DEV)
    wd2, widx = ops.knn_unpack(want)
    assert torch.equal(bits(d2), bits(wd2)) and torch.equal(idx, widx) and not idx.requires_grad
    w = torch.from_numpy(np.random.RandomState(13).randn(*d2.shape).astype(np.float32)).to(DEV)
    (d2 * w).sum().backward()
    g_src, g_tgt = ops.knn_backward_raw(pts.detach(), pts.detach(), cnt, cnt, want, w)
    assert torch.equal(bits(pts.grad), bits(g_src + g_tgt))
    # two clouds: each receives its own role
    a, b, ca, cb, _ = scene("random")
    A, Bt = torch.from_numpy(a).to(DEV).requires_grad_(True), torch.from_numpy(b).to(DEV).requires_grad_(True)
    cad, cbd = torch.from_numpy(ca).to(DEV), torch.from_numpy(cb).to(DEV)
    d2, _ = ops.knn(A, Bt, cad, cbd, 3)
    d2.sum().backward()
    keys = torch.from_numpy(np.ascontiguousarray(scene_oracle("random")[..., :3])).to(DEV)
    g_a, g_b = ops.knn_backward_raw(A.detach(), Bt.detach(), cad, cbd, keys, torch.ones_like(d2))
    assert torch.equal(bits(A.grad), bits(g_a)) and torch.equal(bits(Bt.grad), bits(g_b))


# ------------------------------------------------------------------ GPU: normals
SPHERE_C = np.array([6.0, 0.0, 0.0])


@lru_cache(maxsize=None)
def normals_scene():
    """600 rows on a sphere of radius 1.5 around SPHERE_C, then 600 on a slightly noisy plane z ~ 3 above the origin."""
    rs = np.random.RandomState(21)
    d = rs.randn(600, 3)
    sphere = SPHERE_C + 1.5 * d / np.linalg.norm(d, axis=1, keepdims=True)
    plane = np.concatenate([rs.rand(600, 2) * 2.0 - 1.0, 3.0 + 0.01 * rs.randn(600, 1)], 1)
    return np.concatenate([sphere, plane]).astype(np.float32)


def covariances(pts, idx):
    """float64 covariance of every row's neighbours, its eigenvalues ascending and eigenvectors."""
    x = pts.astype(np.float64)[idx]  # (n, K, 3)
    d = x - x.mean(1, keepdims=True)
    C = np.einsum("nki,nkj->nij", d, d) / idx.shape[1]
    lam, vec = np.linalg.eigh(C)
    return C, lam, vec


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 8, 16])
def test_normals_are_unit_eigenvectors_of_the_smallest_eigenvalue(K):
    """The kernel computes in fp64 and rounds a unit vector once to fp32: a perturbation of at most sqrt(3) 2^-24 in norm, hence
    a residual of at most 1.74 2^-24 (l2 - l0); 8 is a margin of about 4.5 over that.  No spectral gap is needed."""
    pts = normals_scene()
    cnt = np.array([len(pts)], np.int32)
    keys_np = oracle_keys(pts[None], pts[None], cnt, cnt, K)
    idx = (keys_np[0] & 0xFFFFFFFF).astype(np.int64)
    C, lam, _ = covariances(pts, idx)
    P, cd = torch.from_numpy(pts[None]).to(DEV), torch.from_numpy(cnt).to(DEV)
    keys = ops.knn_raw(P, P, cd, cd, K)
    assert torch.equal(keys.cpu(), torch.from_numpy(keys_np))
    normals, variation = ops.knn_normals_raw(P, P, cd, cd, keys, 0, None, True)
    n = normals[0].cpu().numpy().astype(np.float64)
    l0, l2 = lam[:, 0], lam[:, 2]
    norm_err = np.abs(np.linalg.norm(n, axis=1) - 1.0)
    Cn = np.einsum("nij,nj->ni", C, n)
    ray = np.einsum("ni,ni->n", n, Cn)
    resid = np.linalg.norm(Cn - ray[:, None] * n, axis=1)
    print("K", K, "norm", norm_err.max() / U, "residual / l2", (resid / l2).max() / U, "rayleigh", ((ray - l0) / l2).max() / U)
    assert (norm_err <= 4 * U).all()
    assert (resid <= 8 * U * l2).all()
    assert (ray - l0 <= 8 * U * l2).all()
    var = variation[0].cpu().numpy().astype(np.float64)
    assert np.abs(var - l0 / lam.sum(1)).max() <= 1e-6


@pytest.mark.gpu
def test_normals_orientation_modes():
    pts = normals_scene()
    K = 16
    cnt = torch.tensor([len(pts)], dtype=torch.int32, device=DEV)
    P = torch.from_numpy(pts[None]).to(DEV)
    keys = ops.knn_raw(P, P, cnt, cnt, K)
    free = ops.knn_normals_raw(P, P, cnt, cnt, keys, 0)[0][0].cpu().numpy()
    x = pts.astype(np.float64)
    # mode 1: the sphere seen from its centre, the plane seen from the origin
    for view, rows in ((SPHERE_C, slice(0, 600)), (np.zeros(3), slice(600, 1200))):
        v = torch.tensor(view[None], dtype=torch.float32, device=DEV)
        n = ops.knn_normals_raw(P, P, cnt, cnt, keys, 1, v)[0][0].cpu().numpy()
        assert np.array_equal(np.abs(n), np.abs(free))  # only signs change
        dot = np.einsum("ni,ni->n", n.astype(np.float64)[rows], view[None] - x[rows])
        assert (np.abs(dot) > 1e-3).all()  # the band is empty: every row is decided
        assert (dot > 0).all()
    # mode 2: reference normals with arbitrary signs; a zero reference does not flip
    rs = np.random.RandomState(22)
    ref = np.concatenate([(x[:600] - SPHERE_C) / 1.5, np.tile([[0.0, 0.0, 1.0]], (600, 1))])
    ref = (ref * rs.choice([-1.0, 1.0], (1200, 1))).astype(np.float32)
    zero = rs.permutation(1200)[:100]
    ref[zero] = 0.0
    n = ops.knn_normals_raw(P, P, cnt, cnt, keys, 2, torch.from_numpy(ref[None]).to(DEV))[0][0].cpu().numpy()
    assert np.array_equal(np.abs(n), np.abs(free))
    dot = np.einsum("ni,ni->n", n.astype(np.float64), ref.astype(np.float64))
    live = np.ones(1200, bool)
    live[zero] = False
    assert (np.abs(dot[live]) > 1e-3).all() and (dot[live] > 0).all()
    assert np.array_equal(n[zero].view(np.uint32), free[zero].view(np.uint32))


@pytest.mark.gpu
def test_normals_edge_cases_and_the_pointclouds_method():
    rs = np.random.RandomState(23)
    # batch element 0: two targets only (fewer than three valid slots); 1: a regular cloud with padding rows
    pts = np.stack([_pad(rs.rand(2, 3), 300), _pad(rs.rand(260, 3), 300)])
    cnt = np.array([2, 260], np.int32)
    P, cd = torch.from_numpy(pts).to(DEV), torch.from_numpy(cnt).to(DEV)
    keys = ops.knn_raw(P, P, cd, cd, 8)
    normals, variation = ops.knn_normals_raw(P, P, cd, cd, keys, 0, None, True)
    assert not bool(normals[0].any()) and not bool(variation[0].any())
    assert not bool(normals[1, 260:].any()) and not bool(variation[1, 260:].any())
    assert bool((normals[1, :260].norm(dim=1) > 0.5).all())

    scene_pts = normals_scene()
    colors = torch.rand(1, len(scene_pts), 3, device=DEV)
    feats = torch.rand(1, len(scene_pts), 2, device=DEV)
    X = torch.from_numpy(scene_pts[None]).to(DEV)
    pc = gs.Pointclouds(X, colors=colors, features=feats)
    out, var = pc.estimate_normals(K=16, viewpoint=[0.0, 0.0, 0.0], return_variation=True)
    assert out is not pc and not pc.has_normals and out.has_normals
    assert torch.equal(out.points_padded, X) and torch.equal(out.colors_padded, colors) and torch.equal(out.features_padded, feats)
    cnt1 = torch.tensor([len(scene_pts)], dtype=torch.int32, device=DEV)
    want, wvar = ops.knn_normals_raw(X, X, cnt1, cnt1, ops.knn_raw(X, X, cnt1, cnt1, 16), 1, torch.zeros(1, 3, device=DEV), True)
    assert torch.equal(bits(out.normals_padded), bits(want)) and torch.equal(bits(var), bits(wvar))
    # orient="auto" on a cloud that has normals keeps their side
    flipped = gs.Pointclouds(X, normals=-want)
    again = flipped.estimate_normals(K=16)
    assert torch.equal(bits(again.normals_padded), bits(-want))
    d2, idx = pc.knn(4)
    assert d2.shape == (1, len(scene_pts), 4) and bool((idx[0, :, 0] == torch.arange(len(scene_pts), device=DEV)).all())
    d2o, idxo = pc.knn(1, other=gs.Pointclouds(X[:, :100]))
    assert idxo.shape == (1, len(scene_pts), 1) and int(idxo.max()) < 100 and bool((d2o[0, :100, 0] == 0).all())


# ------------------------------------------------------------------ GPU: outlier removal
def _cloud_with_attributes(pts, seed):
    rs = np.random.RandomState(seed)
    n = pts.shape[1]
    mk = lambda c: torch.from_numpy(rs.rand(pts.shape[0], n, c).astype(np.float32)).to(DEV)
    X = torch.from_numpy(pts).to(DEV).requires_grad_(True)
    return X, gs.Pointclouds(X, normals=mk(3), colors=mk(3), features=mk(2))


def _check_removal(pc, X, out, mask, want_mask):
    """The mask is the oracle's; kept rows keep their order and their attributes; gradients reach exactly the kept rows."""
    want = torch.from_numpy(want_mask).to(DEV)
    assert mask.dtype == torch.bool and torch.equal(mask, want)
    for b in range(len(pc)):
        keep = want[b]
        assert int(out.num_points_per_pointcloud[b]) == int(keep.sum())
        for a in ("points", "normals", "colors", "features"):
            got, src = getattr(out, a + "_list")[b], getattr(pc, a + "_padded")[b]
            assert torch.equal(got.detach(), src.detach()[keep]), (a, b)
    out.points_padded.sum().backward()
    assert torch.equal(X.grad, want.unsqueeze(-1).expand_as(X).float())


SQRT2 = np.float32(np.sqrt(2.0))  # fp32(sqrt 2)^2 = 1.9999999 in fp32: a neighbour at d2 == 2 is OUTSIDE this radius
SQRT2_UP = np.nextafter(SQRT2, np.float32(2.0))  # the next float: its square is 2.0000002, the same neighbour is inside


@pytest.mark.gpu
@pytest.mark.parametrize("radius,m,kept", [(1.0, 6, 154), (1.0, 7, 38), (SQRT2, 7, 38), (SQRT2, 16, 0), (SQRT2_UP, 16, 81),
                                           (SQRT2_UP, 19, 7), (0.5, 1, 300), (0.5, 2, 0)])
def test_radius_rule_is_exact_on_a_lattice(radius, m, kept):
    """Lattice rows have their m-th neighbour at d2 == 1 or 2 exactly: `<= fp32(r) * fp32(r)` with no tolerance decides.  At
    r = 1 the m-th d2 equals r * r; fp32(sqrt 2) and the next float lie on either side of d2 == 2.  `kept` is the oracle's
    count (numpy, computed without the code under test): it pins that the cases decide what they are meant to decide."""
    rs = np.random.RandomState(31)
    lat = _lattice(7)
    lat = lat[rs.permutation(len(lat))[:300]]  # a thinned lattice: neighbour counts vary from row to row
    pts = lat[None]
    cnt = np.array([300], np.int32)
    d2m = oracle_keys(pts, pts, cnt, cnt, m)[0, :, m - 1]
    r2 = np.float32(radius) * np.float32(radius)
    assert r2.dtype == np.float32
    want = (d2m != KEY_NONE) & ((d2m >> 32).astype(np.uint32).view(np.float32) <= r2)
    assert int(want.sum()) == kept
    X, pc = _cloud_with_attributes(pts, 32)
    out, mask = pc.remove_radius_outliers(radius, m, return_mask=True)
    _check_removal(pc, X, out, mask, want[None])


def statistical_oracle(pts, K, ratio):
    cnt = np.array([len(pts)], np.int32)
    keys = oracle_keys(pts[None], pts[None], cnt, cnt, K + 1)[0, :, 1:]
    d = np.sqrt((keys >> 32).astype(np.uint32).view(np.float32).astype(np.float64))
    mean = d.mean(1)
    mu, sigma = mean.mean(), mean.std()
    thr = mu + ratio * sigma
    return mean <= thr, np.abs(mean - thr) <= 1e-9 * thr


@lru_cache(maxsize=None)
def speck_scene():
    rs = np.random.RandomState(41)
    body = np.concatenate([rs.rand(1200, 2) * 2.0, 0.02 * rs.randn(1200, 1)], 1)
    specks = rs.rand(30, 3) * 2.0 + np.array([0.0, 0.0, 0.5])
    return np.concatenate([body, specks])[rs.permutation(1230)].astype(np.float32)


def test_statistical_oracle_has_no_row_near_its_threshold():
    """CPU, the oracle alone: on both scenes no row lies within relative 1e-9 of the threshold, so the GPU tests below compare
    every row."""
    for pts in (speck_scene(), normals_scene()):
        keep, band = statistical_oracle(pts, 8, 2.0)
        assert not band.any() and 0 < (~keep).sum() < len(pts) // 4


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["specks", "sphere_and_plane"])
def test_statistical_rule_matches_the_float64_oracle(which):
    pts = speck_scene() if which == "specks" else normals_scene()
    want, band = statistical_oracle(pts, 8, 2.0)
    assert band.sum() <= 2
    X, pc = _cloud_with_attributes(pts[None], 42)
    out, mask = pc.remove_statistical_outliers(8, 2.0, return_mask=True)
    got = mask[0].cpu().numpy()
    assert np.array_equal(got[~band], want[~band])
    if which == "specks":
        assert (~want).sum() >= 15  # most specks go
    _check_removal(pc, X, out, mask, got[None])


@pytest.mark.gpu
def test_outlier_removal_on_a_ragged_batch():
    rs = np.random.RandomState(51)
    a, b = rs.rand(200, 3).astype(np.float32), rs.rand(1, 3).astype(np.float32)
    pc = gs.Pointclouds([torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)])
    out, mask = pc.remove_radius_outliers(0.2, 4, return_mask=True)
    cnt = np.array([200], np.int32)
    d2m = oracle_keys(a[None], a[None], cnt, cnt, 4)[0, :, 3]
    want = (d2m >> 32).astype(np.uint32).view(np.float32) <= np.float32(0.2) * np.float32(0.2)
    assert np.array_equal(mask[0].cpu().numpy(), want) and not bool(mask[1].any())
    assert out.num_points_per_pointcloud.tolist() == [int(want.sum()), 0]
    out2, mask2 = pc.remove_statistical_outliers(4, 1.0, return_mask=True)
    assert bool(mask2[1, 0]) and not bool(mask2[1, 1:].any())  # a lone point has no statistic and stays
    assert out2.num_points_per_pointcloud.tolist()[1] == 1
