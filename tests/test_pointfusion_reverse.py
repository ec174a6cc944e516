"""The reverse of the one-call PointFusion update (gs_pointfusion_update_taped / gs_pointfusion_update_backward), called
directly through _native and compared with float64 torch autograd through oracle.fusion.fuse_with_map.

Every buffer the pair may forget to write is poisoned: the tape and both workspaces hold 0xFF bytes (NaN as floats, -1 as
ints) before each call, the four frame adjoints hold NaN before the reverse.  The upstream adjoints G_* are distinct odd
multiples of 2^-25 in (-0.5, 0.5): no two elements of the four arrays are equal, so a row read at the wrong index, a
pixel written from the wrong row or a swapped attribute cannot pass, and the confidence counts' and normals' adjoints are
as large as the points', so the weight path (c_bar, a_bar, alpha -> g_vertex) is visible (test_reference_has_teeth_*).

Scenes: the engineered 6 x 8 inputs of test_map_update_edges (variants main / none / b1_only; the whole reverse is one
256-thread block and one compaction block there), "seams" (B = 2, 36 x 61: 2196 pixels per element are three compaction
blocks with a partial last one and put the b = 0 / b = 1 boundary inside a workgroup of fuse_bwd_matched_k; counts
(3000, 1500) with Nmax = 5196 = 3000 + 2196 sit exactly at the capacity contract), and "two" (a second frame on the arena
the first one left, reversed in turn).  The CPU tests prove that the float32 and the float64 oracle take identical
decisions on every scene; the GPU tests then allow no flipped decision and first require the forward's stats to be the
oracle's.

Contract pinned here (include/gradslam_hip.h): the pair assumes live rows with counts > 0.  An unmatched row with count 0,
in a frame that has any correspondence, is zeroed by the forward as in the reference, and the reverse leaves its G and its
zeros in place (the reference's adjoint there is 0).  Those rows -- selected by computation, 403 of them in variant main,
b = 0 -- are checked bit for bit against that statement and are the only rows left out of the reference comparison.
"""
import functools
import warnings

import pytest
import torch

from tests.helpers import rel_err
from tests.test_map_update_edges import (B, COUNTS, DIST_TH, DOT_TH, H, NMAX, R1, SIGMA, T1, VARIANTS, W, _HAND, _case, _oracle,
                                         _rot, _same_bits, _to_world)

DEV = "cuda:0"
NAMES = ("points", "normals", "colors", "feats")
MAP_OUT = ("G_points", "G_normals", "G_colors", "G_ccounts")
FRAME_OUT = ("g_vertex", "g_gvertex", "g_gnormal", "g_rgb")
FRAME_LEAVES = ("V", "gV", "gN", "rgb")
F32, F64 = torch.float32, torch.float64

# "seams"
SH, SW = 36, 61
S_COUNTS, S_NMAX = (3000, 1500), 5196
S_HOLES = ((0, 33), (3, 7), (12, 0), (20, 45), (35, 60))   # first row, first column, and the element's last pixel
# "two": the second frame's holes.  (1, 1) is one of them because the row placed there with a normal dot product EQUAL to the
# threshold is re-rounded by frame 1's merge, (3 x + 0) * (1 / 3), to one ulp above it in float32 and not in float64
HOLES2 = ((1, 1), (4, 6))
SCENES = VARIANTS + ("seams", "two")


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ---------------------------------------------------------------------------------------------- scenes
def _sray(h, w, z):
    """Pixel (h, w)'s ray at depth z for f = 32, cx = 30, cy = 18 (exact for the dyadic z used)."""
    return ((w - 30) * z / 32.0, (h - 18) * z / 32.0, z)


def _seam_scene():
    g = torch.Generator().manual_seed(20261)
    depth = torch.full((B, 1, SH, SW, 1), 2.0)
    for h, w in S_HOLES:
        depth[:, :, h, w] = 0.0
    rgb = torch.rand((B, 1, SH, SW, 3), generator=g)
    K = torch.eye(4).view(1, 1, 4, 4).repeat(B, 1, 1, 1)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2] = 32.0, 32.0, 30.0, 18.0
    pose = torch.eye(4).view(1, 1, 4, 4).repeat(B, 1, 1, 1)
    pose[1, 0, :3, :3] = torch.tensor(R1)
    pose[1, 0, :3, 3] = torch.tensor(T1)
    # a third of the pixels gets no map point at all (they are appended), holes get none either
    free = [(h, w) for h in range(SH) for w in range(SW) if (h * SW + w) % 3 and (h, w) not in S_HOLES]
    normals = ((0.0, 0.0, 1.0), (0.0, 0.25, 0.96875), (0.0, 0.5, 0.75))
    cvals = (0.5, 1.0, 2.0, 3.0)                        # counts > 0 only: the contract of the taped pair
    # depths 2 + k / 64 with no two |k| alike: two rows of one pixel and one count either share a depth (bit-equal keys, the
    # index decides) or differ in ray distance by far more than rounding -- z = 2 +- d would be an exact tie that the
    # float32 and the float64 oracle may break differently
    ks = (-5, -3, -1, 0, 2, 4, 6)
    ri = lambda n: int(torch.randint(0, n, (1,), generator=g))
    pts, nrms, cols, ccs = [], [], [], []
    for b in range(B):
        rows = []
        for _ in range(S_COUNTS[b]):
            h, w = free[ri(len(free))]
            rows.append((_sray(h, w, 2.0 + ks[ri(7)] / 64.0), normals[ri(3)], cvals[ri(4)]))
        behind = torch.rand((8, 6), generator=g)         # live, never active, full-mantissa coordinates
        for i in range(8):
            x = behind[i].tolist()
            rows[700 + 97 * i] = ((x[0], x[1], -1.0 - x[2]), (x[3], x[4], x[5]), 3.0)
        pts.append(torch.tensor([_to_world(p, b) for p, _, _ in rows], dtype=F32))
        nrms.append(torch.tensor([_rot(n, b) for _, n, _ in rows], dtype=F32))
        ccs.append(torch.tensor([[c] for _, _, c in rows], dtype=F32))
        cols.append(torch.rand((len(rows), 3), generator=g))
    return dict(H=SH, W=SW, counts=S_COUNTS, nmax=S_NMAX, frames=[dict(depth=depth, rgb=rgb, K=K, pose=pose)], points=pts,
                normals=nrms, colors=cols, feats=ccs)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """Float32 CPU tensors: frames (each depth (B,1,H,W,1), rgb, K, pose) and the map as four per-element lists."""
    if name == "seams":
        return _seam_scene()
    c = _case("main" if name == "two" else name)
    frames = [dict(depth=c["depth"], rgb=c["rgb"], K=c["K"], pose=c["pose"])]
    if name == "two":  # the same plane 2^-6 further away, other holes, other colours
        depth2 = torch.full((B, 1, H, W, 1), 2.0 + 2.0 ** -6)
        for h, w in HOLES2:
            depth2[:, :, h, w] = 0.0
        rgb2 = torch.rand((B, 1, H, W, 3), generator=torch.Generator().manual_seed(20262))
        frames.append(dict(depth=depth2, rgb=rgb2, K=c["K"], pose=c["pose"]))
    return dict(H=H, W=W, counts=COUNTS, nmax=NMAX, frames=frames, points=c["points"], normals=c["normals"], colors=c["colors"],
                feats=c["feats"])


def _appended_pixels(depth, unique, Hh, Ww):
    valid = (depth > 0)[:, 0, :, :, 0]
    out = []
    for b in range(B):
        taken = {(int(r[2]), int(r[3])) for r in unique if int(r[0]) == b}
        out.append([(h, w) for h in range(Hh) for w in range(Ww) if bool(valid[b, h, w]) and (h, w) not in taken])
    return out


@functools.lru_cache(maxsize=None)
def _chain(name, dtype):
    """The oracle frame after frame in `dtype`, tables from the same dtype: per frame the map it met (cloud_in), the three
    tables, the appended pixel lists and the updated map.  The engineered variants take theirs from the sibling's _oracle."""
    from oracle import fusion
    from oracle.cloud import Cloud

    sc = _scene(name)
    cloud = Cloud(*[[x.to(dtype) for x in sc[k]] for k in NAMES])
    steps = []
    for fi, f in enumerate(sc["frames"]):
        if fi == 0 and name != "seams":
            o = _oracle("main" if name == "two" else name, dtype)
            st = {k: o[k] for k in ("fr", "active", "similar", "unique", "out", "appended")}
        else:
            fr = fusion.make_frame(f["rgb"].to(dtype), f["depth"].to(dtype), f["K"].to(dtype), f["pose"].to(dtype))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                active = fusion.find_active_map_points(cloud, fr)
                similar, _ = fusion.find_similar_map_points(cloud, fr, active, DIST_TH, DOT_TH)
                unique = fusion.find_best_unique_correspondences(cloud, fr, similar)
                out = fusion.fuse_with_map(cloud, fr, unique, SIGMA)
            st = dict(fr=fr, active=active, similar=similar, unique=unique, out=out,
                      appended=_appended_pixels(f["depth"], unique, sc["H"], sc["W"]))
        st["cloud_in"], st["n_before"] = cloud, cloud.counts
        cloud = st["out"]
        steps.append(st)
    return steps


def _matched(st, b):
    """(n_before[b]) bool: the rows of element b that the frame merged into, and their pixels (row-major index)."""
    m = torch.zeros(st["n_before"][b], dtype=torch.bool)
    u = st["unique"]
    u = u[u[:, 0] == b]
    m[u[:, 1]] = True
    return m, u


def _count0_unmatched(st, b):
    """The rows outside the pair's contract: count 0, not merged into, in a frame that merged (the reference merges the
    whole padded batch as soon as ANY element has a correspondence)."""
    z = st["cloud_in"].feats[b][:, 0] == 0
    if st["unique"].shape[0] == 0:
        return torch.zeros_like(z)
    return z & ~_matched(st, b)[0]


@functools.lru_cache(maxsize=None)
def _excluded(name):
    """(B, nmax) bool: rows that were count-0-unmatched in some frame (float32 oracle)."""
    sc = _scene(name)
    ex = torch.zeros((B, sc["nmax"]), dtype=torch.bool)
    for st in _chain(name, F32):
        for b in range(B):
            z = _count0_unmatched(st, b)
            ex[b, : z.shape[0]] |= z
    return ex


def _final_counts(name, nmax):
    return [min(n, nmax) for n in _chain(name, F32)[-1]["out"].counts]


@functools.lru_cache(maxsize=None)
def _distinct():
    return torch.randperm(2 ** 24, generator=torch.Generator().manual_seed(20263), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _G(name, nmax):
    """The four upstream adjoints (B, nmax, C), float32: (2 k + 1 - 2^24) / 2^25 for distinct k < 2^24 -- odd numerators below
    2^24 in magnitude, so every value is exact in float32, non-zero, inside (-0.5, 0.5) and met once only.  Zero beyond
    each element's new count."""
    total = B * nmax * 10
    k = _distinct()[SCENES.index(name) * 200000:][:total].double()
    v = ((2.0 * k + 1.0 - 2.0 ** 24) / 2.0 ** 25).to(F32)
    assert v.numel() == total and v.unique().numel() == total and float(v.abs().max()) < 0.5 and float(v.abs().min()) > 0
    out, at = [], 0
    for width in (3, 3, 3, 1):
        a = v[at: at + B * nmax * width].view(B, nmax, width).clone()
        at += B * nmax * width
        for b, n in enumerate(_final_counts(name, nmax)):
            a[b, n:] = 0.0
        out.append(a)
    return tuple(out)


# ---------------------------------------------------------------------------------------------- the reference
def _fuse_restated(cloud, fr, pc2im, sigma, detach_weights):
    """oracle.fusion.fuse_with_map statement for statement, with a switch that cuts the merge weights out of the graph (no
    c_bar, no a_bar: the counts keep only c2 = c + a).  Used by test_reference_has_teeth alone, which first proves that
    with the switch off it gives the oracle's gradients."""
    from oracle import fusion
    from oracle.cloud import Cloud

    gV, gN, rgb = fr["gV"], fr["gN"], fr["rgb"]
    alpha = fusion.get_alpha(fr["V"], dim=4, keepdim=True, sigma=sigma)
    merged = cloud
    if pc2im.shape[0] != 0:
        b, n, h, w = pc2im.unbind(1)
        mp, mn, mc, cc = (cloud.padded(k) for k in NAMES)
        fp, fn, fc, fa = (torch.zeros_like(x) for x in (mp, mn, mc, cc))
        fp[b, n], fn[b, n], fc[b, n], fa[b, n] = gV[b, 0, h, w], gN[b, 0, h, w], rgb[b, 0, h, w], alpha[b, 0, h, w]
        cc2 = cc + fa
        wc, wa, w2 = (cc.detach(), fa.detach(), cc2.detach()) if detach_weights else (cc, fa, cc2)
        inv = 1 / torch.where(w2 == 0, torch.ones_like(w2), w2)
        merged = Cloud(cloud.points, cloud.normals, cloud.colors, cloud.feats)
        merged.set_from_padded("points", ((wc * mp) + (wa * fp)) * inv)
        merged.set_from_padded("normals", ((wc * mn) + (wa * fn)) * inv)
        merged.set_from_padded("colors", ((wc * mc) + (wa * fc)) * inv)
        merged.set_from_padded("feats", cc2)
    new = torch.ones_like(gV[..., 0], dtype=bool)
    if pc2im.shape[0] != 0:
        new[pc2im[:, 0], 0, pc2im[:, 2], pc2im[:, 3]] = 0
    new = new * (fr["depth"] > 0).squeeze(-1)
    fresh = Cloud([gV[b][new[b]] for b in range(B)], [gN[b][new[b]] for b in range(B)], [rgb[b][new[b]] for b in range(B)],
                  [alpha[b][new[b]] for b in range(B)])
    return merged.append(fresh)


@functools.lru_cache(maxsize=None)
def _autograd(name, dtype, nmax, mode="full"):
    """torch autograd in `dtype` through the chained fuse_with_map calls, correspondence tables constant (the float32
    oracle's), loss = sum(out.padded(name)[:, :nmax] * G_name).  Leaves: the map's four lists, every frame's V, gV, gN, rgb.
    -> {"G_points".. : (B, nmax, C) with the rows beyond the old counts zero, (frame, "g_vertex").. : (B, H, W, 3)}.
    mode: "full" (the oracle), "restated" / "weights_detached" (_fuse_restated), "no_appended" (G zeroed behind the old
    counts of the last frame: the appended rows' adjoints dropped)."""
    from oracle import fusion
    from oracle.cloud import Cloud

    sc, steps = _scene(name), _chain(name, F32)
    G = [g.to(dtype).clone() for g in _G(name, nmax)]
    if mode == "no_appended":
        for g in G:
            for b in range(B):
                g[b, steps[-1]["n_before"][b]:] = 0.0
    leaves = [[x.to(dtype).clone().requires_grad_() for x in sc[k]] for k in NAMES]
    cloud = Cloud(*leaves)
    frs = []
    for f, st in zip(sc["frames"], steps):
        fr = dict(fusion.make_frame(f["rgb"].to(dtype), f["depth"].to(dtype), f["K"].to(dtype), f["pose"].to(dtype)))
        for k in FRAME_LEAVES:
            fr[k] = fr[k].detach().clone().requires_grad_()
        frs.append(fr)
        if mode in ("full", "no_appended"):
            cloud = fusion.fuse_with_map(cloud, fr, st["unique"], SIGMA)
        else:
            cloud = _fuse_restated(cloud, fr, st["unique"], SIGMA, mode == "weights_detached")
    loss = 0.0
    for i, k in enumerate(NAMES):
        P = cloud.padded(k)
        n = min(P.shape[1], nmax)
        loss = loss + (P[:, :n] * G[i][:, :n]).sum()
    flat = [x for xs in leaves for x in xs] + [fr[k] for fr in frs for k in FRAME_LEAVES]
    grads = torch.autograd.grad(loss, flat, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for x, g in zip(flat, grads)]
    out = {}
    for i, k in enumerate(MAP_OUT):
        a = torch.zeros((B, nmax, G[i].shape[2]), dtype=dtype)
        for b in range(B):
            a[b, : sc["counts"][b]] = grads[i * B + b]
        out[k] = a
    for fi in range(len(frs)):
        for j, k in enumerate(FRAME_OUT):
            out[(fi, k)] = grads[4 * B + 4 * fi + j][:, 0]
    return out


def _compare_rows(name):
    """(B, nmax) bool: the rows of the map adjoint that are compared with the reference: every live row but the excluded."""
    sc = _scene(name)
    m = torch.zeros((B, sc["nmax"]), dtype=torch.bool)
    for b in range(B):
        m[b, : sc["counts"][b]] = True
    return m & ~_excluded(name)


def _own_and_bound(name, nmax, key):
    """The float32 oracle's rel_err against the float64 oracle on output `key`, and the bound for the GPU:
    max(4 x own, 2^-22) -- two expf implementations may each be an ulp or two off in opposite directions and the merge
    multiplies by the weight once (the convention of test_map_update_edges._check_fusion)."""
    r32, r64 = _autograd(name, F32, nmax)[key], _autograd(name, F64, nmax)[key]
    if key in MAP_OUT:
        rows = _compare_rows(name)[:, :nmax]
        r32, r64 = r32[rows], r64[rows]
    own = rel_err(r32, r64)
    return own, max(4.0 * own, 2.0 ** -22)


# ---------------------------------------------------------------------------------------------- CPU-only tests
@pytest.mark.parametrize("name", SCENES)
def test_scenes_are_unambiguous(name):
    """float32 and float64 oracle take identical decisions in every frame of every scene; the scene holds what its name says."""
    sc, c32, c64 = _scene(name), _chain(name, F32), _chain(name, F64)
    assert len(c32) == len(c64) == len(sc["frames"])
    for s32, s64 in zip(c32, c64):
        for k in ("active", "similar", "unique"):
            assert torch.equal(s32[k], s64[k]), k
        assert s32["appended"] == s64["appended"] and s32["n_before"] == s64["n_before"]
        assert s32["out"].counts == s64["out"].counts == [n + len(a) for n, a in zip(s32["n_before"], s32["appended"])]
    assert c32[0]["n_before"] == list(sc["counts"])
    assert all(n + sc["H"] * sc["W"] <= sc["nmax"] for st in c32 for n in st["n_before"])  # the capacity contract holds
    ex = _excluded(name)
    if name == "main":
        # the count-0 rows that no pixel takes, recomputed from the inputs a second way
        c0 = set((_case("main")["feats"][0][:, 0] == 0).nonzero()[:, 0].tolist())
        won = {int(r[1]) for r in c32[0]["unique"] if int(r[0]) == 0}
        assert int(ex[0].sum()) == len(c0 - won) == 403 and int(ex[1].sum()) == 0
        assert _HAND["c0_nearer"][0] in c0 & won and len(c0 & won) >= 1       # a MATCHED count-0 row exists
    if name == "none":
        assert int(ex.sum()) == 0 and c32[0]["unique"].shape[0] == 0            # no merge ran: nothing is outside the contract
    if name == "b1_only":
        assert int(ex[0].sum()) == int((_case(name)["feats"][0][:, 0] == 0).sum()) > 0 and int(ex[1].sum()) == 0
    if name == "seams":
        st = c32[0]
        assert int(ex.sum()) == 0 and all(bool((x > 0).all()) for x in sc["feats"])
        assert sc["counts"][0] + SH * SW == sc["nmax"] and (SH * SW) % 256 != 0 and 2 * 1024 < SH * SW < 3 * 1024
        for b in range(B):
            m, u = _matched(st, b)
            pix = (u[:, 2] * SW + u[:, 3]).tolist()
            app = [h * SW + w for h, w in st["appended"][b]]
            # matched and appended pixels in each of the three compaction blocks and on both sides of the element seam
            for lo, hi in ((0, 1024), (1024, 2048), (2048, SH * SW)):
                few = (hi - lo) // 10
                assert sum(lo <= p < hi for p in pix) >= few and sum(lo <= p < hi for p in app) >= few, (b, lo)
            assert 300 <= len(pix) and 300 <= len(app) and int((~m).sum()) >= 300
            last, first = SH * SW - (SH * SW * (b + 1)) % 256, 256 - (SH * SW * b) % 256
            assert any(p >= last for p in pix) and any(p >= last for p in app)
            assert any(p < first for p in pix) and any(p < first for p in app)
        assert (SH - 1, SW - 1) in S_HOLES
    if name == "two":
        s1, s2 = c32
        for b in range(B):
            m2, u2 = _matched(s2, b)
            assert int(m2[sc["counts"][b]:].sum()) >= 5, "rows appended by frame 1 are matched in frame 2"
            assert int(m2[: sc["counts"][b]].sum()) >= 1 and len(s2["appended"][b]) >= 1
        m1, m2 = _matched(s1, 0)[0], _matched(s2, 0)[0]
        assert int((m1 & m2[: m1.shape[0]]).sum()) >= 5, "rows merged by both frames"
        # what frame 1 zeroed stays outside the contract in frame 2, and nothing joins it
        assert torch.equal(_count0_unmatched(s2, 0)[: m1.shape[0]], _count0_unmatched(s1, 0))
        assert not _count0_unmatched(s2, 0)[m1.shape[0]:].any() and not _count0_unmatched(s2, 1).any()


@pytest.mark.parametrize("name", ("main", "b1_only", "seams", "two"))
def test_reference_has_teeth_on_the_weight_path(name):
    """With the merge weights cut out of the graph the float64 reference moves by more than 100 bounds on the counts'
    adjoint and on g_vertex: the chosen G makes c_bar, a_bar and alpha's adjoint visible."""
    nmax = _scene(name)["nmax"]
    full, same, cut = (_autograd(name, F64, nmax, m) for m in ("full", "restated", "weights_detached"))
    for k in full:
        assert torch.equal(full[k], same[k]), k  # the restatement is the oracle when the switch is off
    rows = _compare_rows(name)
    for key in ["G_ccounts"] + [(fi, "g_vertex") for fi in range(len(_scene(name)["frames"]))]:
        _, bound = _own_and_bound(name, nmax, key)
        a, b = (cut[key][rows], full[key][rows]) if key in MAP_OUT else (cut[key], full[key])
        moved = rel_err(a, b)
        print("%s/%s: weights detached moves the reference by %.3e = %.0f bounds" % (name, key, moved, moved / bound))
        assert moved > 100.0 * bound, (key, moved, bound)


@pytest.mark.parametrize("name", ("main", "none", "b1_only", "seams", "two"))
def test_reference_has_teeth_on_the_appended_rows(name):
    """With the appended rows' adjoints dropped the reference moves by more than 100 bounds on all four frame adjoints."""
    nmax = _scene(name)["nmax"]
    full, cut = _autograd(name, F64, nmax), _autograd(name, F64, nmax, "no_appended")
    fi = len(_scene(name)["frames"]) - 1
    for k in FRAME_OUT:
        _, bound = _own_and_bound(name, nmax, (fi, k))
        moved = rel_err(cut[(fi, k)], full[(fi, k)])
        assert moved > 100.0 * bound, (k, moved, bound)


def test_clamped_reference_is_the_truncated_one():
    """The clamp case's reference: the seven dropped pixels of b = 0 get no adjoint, b = 1 and every kept pixel keep theirs
    up to the rows of G that the smaller arena no longer has (those are other random numbers: only zeros are compared)."""
    st = _chain("main", F32)[0]
    nmax = st["out"].counts[0] - 7
    assert nmax > COUNTS[0] and nmax >= st["out"].counts[1] and len(st["appended"][0]) > 7
    r = _autograd("main", F64, nmax)
    for h, w in st["appended"][0][-7:]:
        assert all(not r[(0, k)][0, h, w].any() for k in FRAME_OUT)
    for h, w in st["appended"][0][:-7]:
        assert all(r[(0, k)][0, h, w].any() for k in FRAME_OUT)


# ---------------------------------------------------------------------------------------------- GPU side
def _poison(nbytes):
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=DEV)


def _frame_dev(f):
    return f["depth"][:, 0].contiguous().to(DEV), f["rgb"][:, 0].contiguous().to(DEV), f["K"].to(DEV), f["pose"].to(DEV)


class _Run:
    """One arena on the device walked forward through a scene's frames and back, with snapshots on the CPU."""

    def __init__(self, name, nmax):
        from gradslam_amd import _native as nv

        self.nv, self.name, self.nmax = nv, name, nmax
        sc = self.sc = _scene(name)
        self.H, self.W = sc["H"], sc["W"]
        self.arena = []
        for k, width in zip(NAMES, (3, 3, 3, 1)):
            a = torch.zeros((B, nmax, width), dtype=F32)
            for b in range(B):
                a[b, : sc["counts"][b]] = sc[k][b]
            self.arena.append(a.to(DEV))
        self.counts = torch.tensor(sc["counts"], dtype=torch.int32, device=DEV)
        self.G = [g.to(DEV) for g in _G(name, nmax)]
        self.tapes = []

    def snap(self):
        torch.cuda.synchronize()
        return dict(arena=[a.cpu() for a in self.arena], counts=self.counts.cpu().tolist(), G=[g.cpu() for g in self.G])

    def forward(self, fi):
        nv, Hh, Ww, nmax = self.nv, self.H, self.W, self.nmax
        depth, rgb, K, pose = _frame_dev(self.sc["frames"][fi])
        tape = _poison(nv.ws_bytes("gs_pointfusion_update_tape_bytes", B, Hh, Ww))
        ws = _poison(nv.ws_bytes("gs_pointfusion_update_ws_bytes", B, Hh, Ww, nmax))
        stats = torch.zeros(4 + B, dtype=torch.int32, device=DEV)
        nv.call("gs_pointfusion_update_taped", nv.ptr(depth), nv.ptr(rgb), nv.ptr(K), nv.ptr(pose), B, Hh, Ww,
                *[nv.ptr(a) for a in self.arena], nv.ptr(self.counts), nmax, DIST_TH, DOT_TH, SIGMA, nv.ptr(stats), nv.ptr(tape),
                tape.numel(), nv.ptr(ws), ws.numel(), nv.stream())
        torch.cuda.synchronize()
        self.tapes.append(tape)
        return stats.cpu().tolist()

    def reverse(self, fi):
        nv, Hh, Ww, nmax = self.nv, self.H, self.W, self.nmax
        depth, rgb, K, pose = _frame_dev(self.sc["frames"][fi])
        g = [torch.full((B, Hh, Ww, 3), float("nan"), dtype=F32, device=DEV) for _ in FRAME_OUT]
        ws = _poison(nv.ws_bytes("gs_pointfusion_update_backward_ws_bytes", B, Hh, Ww))
        tape = self.tapes[fi]
        nv.call("gs_pointfusion_update_backward", nv.ptr(depth), nv.ptr(rgb), nv.ptr(K), nv.ptr(pose), B, Hh, Ww,
                *[nv.ptr(a) for a in self.arena], nv.ptr(self.counts), nmax, SIGMA, nv.ptr(tape), tape.numel(),
                *[nv.ptr(x) for x in self.G], *[nv.ptr(x) for x in g], nv.ptr(ws), ws.numel(), nv.stream())
        torch.cuda.synchronize()
        return dict(zip(FRAME_OUT, [x.cpu() for x in g]))


def _check_forward(name, fi, nmax, stats, after, clamped=()):
    """The forward took the oracle's decisions: stats and counts."""
    st = _chain(name, F32)[fi]
    want = [min(n + len(a), nmax) for n, a in zip(st["n_before"], st["appended"])]
    assert all((want[b] < st["n_before"][b] + len(st["appended"][b])) == (b in clamped) for b in range(B))
    assert after["counts"] == want
    assert stats[0] == st["active"].shape[0] and stats[1] == st["unique"].shape[0] and stats[2] == (1 if clamped else 0)
    assert stats[4:] == [want[b] - st["n_before"][b] for b in range(B)]
    return want


def _check_exact(name, fi, nmax, before, after, back, g, want):
    """Everything about one reverse step that is exact.  before / after / back: snapshots before the frame's forward,
    after it (with the G the reverse was given), and after the reverse; g: the four frame adjoints; want: the counts the
    forward left."""
    sc, st = _scene(name), _chain(name, F32)[fi]
    Hh, Ww = sc["H"], sc["W"]
    assert back["counts"] == st["n_before"], "map_counts restored"
    for k in FRAME_OUT:
        assert not torch.isnan(g[k]).any(), (k, "holds a word the reverse never wrote")
    holes = (sc["frames"][fi]["depth"] > 0)[:, 0, :, :, 0].logical_not()
    assert int(holes.sum()) >= 2 * B
    for k in FRAME_OUT:
        assert not g[k][holes].any(), (k, "pixels without depth")
    for b in range(B):
        nb = st["n_before"][b]
        m, u = _matched(st, b)
        ex = _count0_unmatched(st, b)
        c_in = before["arena"][3][b, :nb, 0]
        for i, k in enumerate(NAMES):
            a0, af, ar = before["arena"][i][b], after["arena"][i][b], back["arena"][i][b]
            assert _same_bits(ar[:nb][m], a0[:nb][m]), (k, b, "matched rows get their pre-forward bits back")
            assert _same_bits(ar[:nb][~m], af[:nb][~m]), (k, b, "unmatched live rows keep the forward's re-rounded bits")
            assert _same_bits(ar[nb:], af[nb:]), (k, b, "rows behind the previous count are not touched")
            Gi, Go = after["G"][i][b], back["G"][i][b]
            assert _same_bits(Go[:nb][~m], Gi[:nb][~m]), (k, b, "an unmatched row's adjoint passes through")
            assert _same_bits(Go[nb:], Gi[nb:]), (k, b, "G behind the previous count is left as it was")
            # outside the contract (count 0, unmatched, the frame merged): the forward's zeros and the row's G stay
            assert not af[:nb][ex].any() and not ar[:nb][ex].any(), (k, b, "count-0 unmatched rows hold zeros")
            assert _same_bits(Go[:nb][ex], Gi[:nb][ex]), (k, b, "count-0 unmatched rows keep their G")
            if k != "feats":  # a matched count-0 row: x' = xf, the map row's own adjoint is exactly 0
                assert not Go[:nb][m & (c_in == 0)].any(), (k, b, "matched count-0 row")
        # appended pixels: row n_before + k is the k-th unmatched valid pixel in row-major order
        kept = want[b] - nb
        hw = torch.tensor(st["appended"][b], dtype=torch.int64).view(-1, 2)
        pix = hw[:, 0] * Ww + hw[:, 1]
        assert kept == min(pix.shape[0], nmax - nb)
        for k, i in (("g_gvertex", 0), ("g_gnormal", 1), ("g_rgb", 2)):
            flat = g[k][b].reshape(Hh * Ww, 3)
            assert _same_bits(flat[pix[:kept]], after["G"][i][b, nb: nb + kept]), (k, b, "appended pixels")
            assert flat[pix[:kept]].abs().min() > 0
        for k in FRAME_OUT:  # the pixels whose rows a clamped forward dropped
            assert not g[k][b].reshape(Hh * Ww, 3)[pix[kept:]].any(), (k, b, "dropped pixels")


def _check_reference(name, nmax, G_back, frame_g):
    """Map adjoints (every live row but the excluded) and each frame's four adjoints against float64 autograd."""
    ref = _autograd(name, F64, nmax)
    rows = _compare_rows(name)[:, :nmax]
    got = {k: G_back[i] for i, k in enumerate(MAP_OUT)}
    for fi, g in frame_g.items():
        got.update({(fi, k): g[k] for k in FRAME_OUT})
    bad = []
    for key, x in got.items():
        own, bound = _own_and_bound(name, nmax, key)
        err = rel_err(x[rows], ref[key][rows]) if key in MAP_OUT else rel_err(x, ref[key])
        print("%s/%s: rel_err GPU %.3e, float32 oracle %.3e, bound %.3e" % (name, key, err, own, bound))
        if not err <= bound:
            bad.append((key, err, bound))
    # Measured on an MI355X, GPU / float32 oracle / bound (2.384e-7 is the floor 2^-22):
    #   main     G_points 8.970e-8 / 1.049e-7 / 4.198e-7, G_normals 9.425e-8 / 9.201e-8 / 3.680e-7, G_colors 8.369e-8 / 6.956e-8 /
    #            2.782e-7, G_ccounts 8.588e-7 / 3.978e-7 / 1.591e-6, g_vertex 1.564e-7 / 5.398e-7 / 2.159e-6, g_gvertex 3.165e-8 /
    #            3.165e-8 / floor, g_gnormal 2.411e-8 / 3.338e-8 / floor, g_rgb 3.216e-8 / 3.216e-8 / floor
    #   none     the map adjoints and g_gvertex, g_gnormal, g_rgb 0 / 0 / floor (copies); g_vertex 1.649e-7 / 1.649e-7 / 6.597e-7
    #   b1_only  G_points 4.614e-8 / 5.962e-8 / 2.385e-7, G_normals 6.161e-8 / 6.161e-8 / 2.465e-7, G_colors 5.288e-8 / 5.961e-8 /
    #            floor, G_ccounts 1.226e-7 / 4.175e-7 / 1.670e-6, g_vertex 3.128e-7 / 2.196e-7 / 8.785e-7, g_gvertex 1.629e-8 /
    #            1.346e-8 / floor, g_gnormal 1.091e-8 / 1.091e-8 / floor, g_rgb 1.476e-8 / 5.134e-9 / floor
    #   seams    G_points 1.224e-7 / 1.385e-7 / 5.539e-7, G_normals 1.112e-7 / 1.409e-7 / 5.636e-7, G_colors 1.017e-7 / 1.265e-7 /
    #            5.059e-7, G_ccounts 4.350e-7 / 3.819e-7 / 1.528e-6, g_vertex 3.983e-7 / 4.507e-7 / 1.803e-6, g_gvertex 5.806e-8 /
    #            6.432e-8 / 2.573e-7, g_gnormal 6.552e-8 / 6.519e-8 / 2.608e-7, g_rgb 5.677e-8 / 5.677e-8 / floor
    #   two      G_points 1.206e-7 / 1.808e-7 / 7.234e-7, G_normals 1.300e-7 / 1.855e-7 / 7.421e-7, G_colors 1.390e-7 / 1.418e-7 /
    #            5.672e-7, G_ccounts 1.163e-6 / 1.133e-6 / 4.532e-6; frame 1: g_vertex 7.152e-7 / 2.134e-6 / 8.534e-6, g_gvertex
    #            1.084e-7 / 1.084e-7 / 4.337e-7, g_gnormal 9.983e-8 / 8.096e-8 / 3.238e-7, g_rgb 9.664e-8 / 6.665e-8 / 2.666e-7;
    #            frame 2: g_vertex 7.242e-7 / 9.381e-7 / 3.752e-6, g_gvertex 1.378e-7 / 1.378e-7 / 5.511e-7, g_gnormal 1.104e-7 /
    #            9.909e-8 / 3.963e-7, g_rgb 1.276e-7 / 1.276e-7 / 5.102e-7
    #   main clamped to Nmax = 2084: G_points 8.970e-8 / 1.049e-7 / 4.198e-7, G_normals 9.066e-8 / 9.382e-8 / 3.753e-7, G_colors
    #            8.836e-8 / 8.497e-8 / 3.399e-7, G_ccounts 3.254e-7 / 7.744e-7 / 3.098e-6, g_vertex 1.835e-7 / 4.595e-7 / 1.838e-6,
    #            g_gvertex 3.145e-8 / 3.145e-8 / floor, g_gnormal 1.656e-8 / 6.018e-8 / 2.407e-7, g_rgb 1.989e-8 / 1.989e-8 / floor
    # The counts' adjoint and g_vertex carry the cancelling sums (x - x') . g and exp, hence their larger own error.
    assert not bad, bad


def _single_frame(name, nmax, clamped=()):
    run = _Run(name, nmax)
    before = run.snap()
    stats = run.forward(0)
    after = run.snap()
    want = _check_forward(name, 0, nmax, stats, after, clamped)
    g = run.reverse(0)
    back = run.snap()
    _check_exact(name, 0, nmax, before, after, back, g, want)
    return run, before, after, back, g


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
def test_reverse_engineered_frame(gs, name):
    """Case (a): restoration, pass-through, the append run backwards, holes, and all eight adjoints against float64."""
    run, before, after, back, g = _single_frame(name, NMAX)
    assert back["counts"] == list(COUNTS)
    if name == "none":  # no merge ran: every live row's G and bits are unchanged, count-0 rows included
        for i in range(4):
            for b in range(B):
                assert _same_bits(back["G"][i][b, : COUNTS[b]], after["G"][i][b, : COUNTS[b]])
                assert _same_bits(back["arena"][i][b, : COUNTS[b]], before["arena"][i][b, : COUNTS[b]])
    _check_reference(name, NMAX, back["G"], {0: g})


@pytest.mark.gpu
def test_reverse_across_block_and_batch_seams(gs):
    """Case (b): three compaction blocks per element with a partial last one, the element boundary inside a 256-thread
    workgroup, b * Nmax + n with Nmax = count + H * W exactly."""
    run, before, after, back, g = _single_frame("seams", S_NMAX)
    _check_reference("seams", S_NMAX, back["G"], {0: g})


@pytest.mark.gpu
def test_reverse_two_frames_on_one_arena(gs):
    """Case (c): frame 2 merges into rows frame 1 appended and appends itself; reverse frame 2, then frame 1."""
    name = "two"
    run = _Run(name, NMAX)
    s0 = run.snap()
    st1 = run.forward(0)
    s1 = run.snap()
    w1 = _check_forward(name, 0, NMAX, st1, s1)
    st2 = run.forward(1)
    s2 = run.snap()
    w2 = _check_forward(name, 1, NMAX, st2, s2)
    g2 = run.reverse(1)
    r2 = run.snap()
    _check_exact(name, 1, NMAX, s1, s2, r2, g2, w2)
    assert r2["counts"] == s1["counts"] == w1
    g1 = run.reverse(0)
    r1 = run.snap()
    _check_exact(name, 0, NMAX, s0, r2, r1, g1, w1)  # frame 1's reverse meets the arena and the G that frame 2's left
    assert r1["counts"] == list(COUNTS)
    _check_reference(name, NMAX, r1["G"], {0: g1, 1: g2})


@pytest.mark.gpu
def test_reverse_of_a_clamped_forward(gs):
    """count + unmatched = Nmax + 7 for b = 0: the seven pixels whose rows the forward dropped get exact zeros (not the
    first rows of b = 1, which is where n_before + pos points at for them), everything else is as in case (a) against the
    oracle truncated to Nmax rows; b = 1 is not affected."""
    full = _chain("main", F32)[0]["out"].counts
    nmax = full[0] - 7
    assert nmax > COUNTS[0] and nmax >= full[1]
    run, before, after, back, g = _single_frame("main", nmax, clamped=(0,))
    assert after["counts"] == [nmax, full[1]]
    dropped = _chain("main", F32)[0]["appended"][0][-7:]
    for h, w in dropped:
        for k in FRAME_OUT:
            assert not g[k][0, h, w].any(), (k, h, w)
    assert after["G"][0][1, :7].abs().min() > 0  # what an unguarded read would have delivered
    _check_reference("main", nmax, back["G"], {0: g})
