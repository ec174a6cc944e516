"""The localisation front end of csrc/project.hip -- the projection of the map into the previous camera, the ICP target in
reference order, its pixel-bucketed scan order and the live frame's ds-grid source cloud -- against an exact reference, in all
three forms: the batch chain (gs_project_active, gs_build_icp_target / gs_bucket_by_pixel), project_target1 and the fused
project_front1 (both through gs_slam_localize with numiters = 0), plus gs_gather_table_rows and gs_table_ds_mask.

Reference (numpy / torch in this module, no code shared with the product):
  table      oracle.fusion.find_active_map_points; ds > 0 keeps the rows with h % ds == 0 and w % ds == 0
  target     per batch element the table's rows in order: tgt[b, k] = points[b, n_k], tnrm likewise, tgt_index[b, k] = n_k,
             counts[b] = number of rows, tgt_pix[b, k] = (h // ds) * Wd + w // ds with Wd = ceil(W / ds)
  buckets    pix_start[b] = exclusive cumsum of bincount(tgt_pix[b], npix), npix + 1 long; scan_orig[b, :count] is a permutation
             whose slot s lies in the bucket of tgt_pix[b, scan_orig[b, s]] (the order inside a pixel is arrival order and left
             free); scan_points[b, s] is bit-equal to tgt[b, scan_orig[b, s]]
  source     every ds-th pixel of every ds-th row with depth > 0 in row-major order: src = gvertex there, src_pix = r * Wd + c
All outputs are integers or copies of input floats: every comparison is bitwise, no tolerance anywhere.

Inputs are engineered so that fp32 takes no decision of its own (as in test_map_update_edges.py): focal lengths are powers of
two, principal points multiples of 1/4, poses signed-permutation rotations (24 of them; non-symmetric ones with -R^T t != 0
among them, identity for b = 0 of a batch) with dyadic translations, map points sit at (u, v) with few fractional bits on
depths {1, 2, 4} x (1 + k / 8).  Every product and sum of the projection is then exact in fp32 in any contraction order and
u = (u z) / z is exact.  Every batch element has its own pose and intrinsics.  test_engineered_inputs_are_unambiguous (CPU)
is the proof: for EVERY input set a GPU test of this module uses, the float32 oracle and the same oracle in float64 give the
same table, and the hand-placed rows (_hand) meet the fate their names state.  No row is left out of any comparison.

Seams reached: the LDS-camera branch and the Cam-array branch of gs_project_active (B = 1, 2, 32 | 33) with ds in {0, 1, 2, 4},
counts from 0 (also in the middle of a batch) to Nmax with a partial last 1024-row block, the compaction's scan launch under
the Cam-array branch (B x Nmax > 1024 x 1024); pix_scan_k's `per` == 1, == 2 with a clipped last thread, one full tile, a
second tile of one bin, three tiles; grids that ds divides on neither side; every point in one pixel, exactly one point per
pixel; empty batch elements between non-empty ones in the `starts` searches; the k >= cap and slot >= cap clamps; both
optional outputs NULL; bucket_scatter_k's `per` > 1 and its second grid-stride trip (nt > 128 x 1024); the last ds-grid size
that takes the fused form (24576) and the first that does not (24577); an empty map, a map behind the camera, a depth frame
with holes on and off the ds-grid; workspaces and outputs poisoned with 0xFF bytes, and workspaces left dirty by another shape.
Rows by name: u, v at -2^-10 (in) and -2^-9 (out), at W - 1 + 2^-10 (in) and W - 1 + 2^-9 (out) and likewise H, half pixels on
both sides of an even and of an odd pixel (round half to even; 1.5 | 2.5 decide ds-grid membership at ds = 2, 3.5 | 4.5 at
ds = 4), z == 0, z < 0 with an in-frame projection, padded rows that would be active, an on-grid pixel beside an off-grid one.

NOT reached: the exact fp32 border value umax = fp32(W - 0.999) (u < umax against u <= umax).  It is not dyadic, so no
engineered row sits on it, with one exception that proves the rule: at W = 3511 fp32(3510.001) IS 3510 + 2^-10, and there the
float32 and the float64 reference disagree about that very row -- the input would be ambiguous.  Sides of 513 pixels and more
therefore take 2^-11 for their inner row.  tgt_index of the two one-sequence forms is not reached either: it exists only in the
tape of gs_slam_localize_taped, whose layout is stated nowhere but in slam.hip's carving; the batch chain's is checked.
"""
import functools
import itertools
import warnings

import numpy as np
import pytest
import torch

from tests.test_fused_setup import localize  # (hands back test_fused_setup.front_views' view of the workspace)

DEV = "cuda:0"
E9, E10, E11 = 2.0 ** -9, 2.0 ** -10, 2.0 ** -11


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ---------------------------------------------------------------------------------------------- the engineered inputs
def _rotations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = torch.zeros((3, 3), dtype=torch.float64)
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if float(torch.det(R)) > 0:
                out.append(R)
    return out


ROTS = _rotations()  # the 24 proper signed permutations; ROTS[0] is the identity
_ASYM = [i for i, R in enumerate(ROTS) if not torch.equal(R, R.t())]
# batch element b takes ROTS[ORDER[b % 24]]: identity, then the non-symmetric ones, then the half turns
ORDER = [0] + _ASYM + [i for i in range(1, 24) if i not in _ASYM]
ASYM = _ASYM[0]

# ds-grid sizes of the target build: npix -> (H, W, ds)
SHAPES = {1: (3, 4, 4), 1024: (32, 32, 1), 1025: (25, 41, 1), 1056: (63, 65, 2), 24576: (128, 192, 1), 24577: (7, 3511, 1),
          49153: (247, 199, 1)}
_PATTERN = (2077, 5, 0, 300, 1024, 1, 0, 97, 2200, 64, 1500)  # very unequal, empty elements, a partial last block, a full one


def _counts(B):
    return {1: (2077,), 2: (2077, 5), 3: (2077, 0, 300)}.get(B) or tuple(_PATTERN[b % len(_PATTERN)] for b in range(B))


CASES = {}


def _add(name, B, H, W, counts=None, nmax=2200, kind="mixed", ds=1):
    CASES[name] = dict(B=B, H=H, W=W, counts=tuple(counts or _counts(B)), Nmax=nmax, kind=kind, ds=ds, seed=len(CASES))


for _B in (1, 2, 32, 33):
    _add("pa_b%d" % _B, _B, 63, 65)
_add("pa_big", 33, 63, 65, counts=[32768 if b in (0, 32) else _PATTERN[b % 11] for b in range(33)], nmax=32768)
for _npix, (_H, _W, _ds) in SHAPES.items():
    for _B in (1, 3, 33):
        _add("t%d_b%d" % (_npix, _B), _B, _H, _W, ds=_ds)
_add("one_pixel", 3, 25, 41, kind="onepix")
_add("per_pixel_1025", 3, 25, 41, counts=(1025, 0, 1025), nmax=1100, kind="perpix")
_add("per_pixel_24577", 1, 7, 3511, counts=(24577,), nmax=24600, kind="perpix")
_add("per_pixel_49153", 1, 247, 199, counts=(49153,), nmax=49200, kind="perpix")
_add("dense", 1, 128, 192, counts=(140000,), nmax=140000, kind="dense")
_add("empty", 1, 25, 41, counts=(0,))
_add("behind", 1, 25, 41, kind="behind")


def _hand(H, W):
    """name -> (u, v, z, pixel or None): rows placed by hand in every batch element that holds enough rows; the fates are
    asserted by name in test_engineered_inputs_are_unambiguous.  um, vm are multiples of 4: on the ds-grid for every ds used."""
    um, vm = (W // 2) // 4 * 4, (H // 2) // 4 * 4
    eu, ev = (E10 if W - 1 < 512 else E11), (E10 if H - 1 < 512 else E11)  # (see NOT reached in the module's docstring)
    rows = {
        "u_lo_in": (-E10, vm, 2.0, (vm, 0)), "u_lo_out": (-E9, vm, 2.0, None),
        "u_hi_in": (W - 1 + eu, vm, 2.0, (vm, W - 1)), "u_hi_out": (W - 1 + E9, vm, 2.0, None),
        "v_lo_in": (um, -E10, 2.0, (0, um)), "v_lo_out": (um, -E9, 2.0, None),
        "v_hi_in": (um, H - 1 + ev, 2.0, (H - 1, um)), "v_hi_out": (um, H - 1 + E9, 2.0, None),
        "z_zero": (um, vm, 0.0, None), "z_neg": (um, vm, -2.0, None),
        "on_grid": (um, vm, 4.0, (vm, um)), "last_pixel": (W - 1, H - 1, 1.0, (H - 1, W - 1)),
    }
    if um + 1 < W:
        rows["off_grid"] = (um + 1, vm, 4.0, (vm, um + 1))
    for x, px in ((1.5, 2), (2.5, 2), (3.5, 4), (4.5, 4)):  # round half to even: both sides of pixel 2 and of pixel 3
        if W >= 6:
            rows["half_u_%s" % x] = (x, vm, 2.0, (vm, px))
        if H >= 6:
            rows["half_v_%s" % x] = (um, x, 2.0, (px, um))
    return rows


def _fill(kind, n, H, W, ds, g):
    """(u, v, z) of n map points in their camera's frame, float64; few fractional bits each."""
    if n == 0:
        return tuple(torch.zeros(0, dtype=torch.float64) for _ in range(3))
    ri = lambda hi: torch.randint(0, hi, (n,), generator=g)
    z = (2.0 ** ri(3).double()) * (1.0 + ri(8).double() / 8.0)
    off = torch.tensor([0.0, 0.0, 0.0, 0.25, -0.25, 0.5], dtype=torch.float64)
    if kind in ("mixed", "behind"):
        u, v = ri(W).double() + off[ri(6)], ri(H).double() + off[ri(6)]
        fate = ri(16)
        u = torch.where(fate == 0, -2.0 - ri(3).double(), u)        # left of the frame
        u = torch.where(fate == 1, W + 1.0 + ri(3).double(), u)     # right of it
        v = torch.where(fate == 2, torch.full_like(v, H + 0.75), v)  # below it
        z = torch.where(fate == 3, -z, z)                           # behind the camera, projection in frame
        z = torch.where(fate == 4, torch.zeros_like(z), z)
        if kind == "behind":
            z = -z.abs() - 1.0
    elif kind == "dense":  # every row in frame: several per pixel
        u, v = ri(W).double(), ri(H).double()
        v = v + off[ri(4)] * (v < H - 1)
    elif kind == "onepix":
        u, v = torch.full((n,), float((W // 2) // 4 * 4), dtype=torch.float64), torch.full((n,), float((H // 2) // 4 * 4), dtype=torch.float64)
    elif kind == "perpix":  # exactly one point on every ds-grid pixel, in a shuffled order
        Hd, Wd = cdiv(H, ds), cdiv(W, ds)
        assert n == Hd * Wd
        q = torch.randperm(n, generator=g)
        u, v = (q % Wd).double() * ds, (q // Wd).double() * ds
        u, v = u + off[ri(4)] * (u < W - 1), v + off[ri(4)] * (v < H - 1)  # (a quarter pixel off, where that stays in the frame)
    else:
        raise ValueError(kind)
    return u, v, z


@functools.lru_cache(maxsize=None)
def _case(name):
    """float32 CPU tensors: points, normals (B, Nmax, 3) with every padded row holding a point that would be active, poses and
    K (B, 4, 4), counts, hand[b] = {name: (row, pixel or None)}, and for one sequence a depth frame (H, W) with holes."""
    s = CASES[name]
    B, H, W, Nmax, counts = s["B"], s["H"], s["W"], s["Nmax"], s["counts"]
    g = torch.Generator().manual_seed(4100 + s["seed"])
    poses = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    K = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    points = torch.zeros((B, Nmax, 3), dtype=torch.float64)
    hand = {}
    for b in range(B):
        R = ROTS[ASYM if B == 1 else ORDER[b % 24]]
        t = torch.tensor([0.5 * (b % 5) - 1.0, 0.25 * (b % 7) + 0.25, 0.5 * (b // 8) - 0.125 * (b % 3)], dtype=torch.float64)
        f, cx, cy = (4.0, 8.0, 2.0, 16.0)[b % 4], W // 2 + 0.5 * (b % 3), H // 2 + 0.25 * (b % 5)
        poses[b, :3, :3], poses[b, :3, 3] = R, t
        K[b, 0, 0], K[b, 1, 1], K[b, 0, 2], K[b, 1, 2] = f, f, cx, cy
        n = counts[b]
        u, v, z = _fill(s["kind"], n, H, W, s["ds"], g)
        hand[b] = {}
        rows = _hand(H, W)
        if s["kind"] in ("mixed", "dense") and n >= 4 * len(rows):
            for i, (nm, (hu, hv, hz, px)) in enumerate(rows.items()):
                at = 3 + i * ((n - 6) // len(rows))  # spread over all of the element's 1024-row blocks
                u[at], v[at], z[at] = hu, hv, hz
                hand[b][nm] = (at, px)
        # padded rows: the point of pixel (0, 0) at depth 1, active if the count did not exclude it
        u, v, z = (torch.cat([x, torch.full((Nmax - n,), pad, dtype=torch.float64)]) for x, pad in ((u, 0.0), (v, 0.0), (z, 1.0)))
        zz = torch.where(z == 0, torch.ones_like(z), z)  # (z == 0 rows keep x and y off the axis)
        pc = torch.stack([(u - cx) * zz / f, (v - cy) * zz / f, z], -1)
        points[b] = pc @ R.t() + t
    p32 = points.float()
    assert torch.equal(p32.double(), points), "a map point is not a float32 value"
    if B > 1:
        assert any(not torch.equal(poses[b, :3, :3], poses[b, :3, :3].t()) and bool((poses[b, :3, :3].t() @ poses[b, :3, 3]).any())
                   for b in range(B)) and torch.equal(poses[0, :3, :3], torch.eye(3, dtype=torch.float64))
        assert len({tuple(poses[b].flatten().tolist()) for b in range(B)}) == B == len({tuple(K[b].flatten().tolist()) for b in range(B)})
    else:
        assert not torch.equal(poses[0, :3, :3], poses[0, :3, :3].t()) and bool((poses[0, :3, :3].t() @ poses[0, :3, 3]).any())
    normals = torch.rand((B, Nmax, 3), generator=g) - 0.5  # full-mantissa values: copied, never computed with
    out = dict(s, points=p32, normals=normals, poses=poses.float(), K=K.float(), hand=hand)
    if B == 1 and H >= 2 and W >= 2:
        depth = 2.0 * (torch.rand((H, W), generator=g) >= 0.1).float()
        um, vm = (W // 2) // 4 * 4, (H // 2) // 4 * 4
        for h, w in ((0, 0), (vm, um), (1, 1), (vm, min(um + 1, W - 1))):  # holes on the ds-grid and (ds > 1) off it
            depth[h, w] = 0.0
        depth[H - 1, W - 1] = 2.0
        out["depth"] = depth
    return out


@functools.lru_cache(maxsize=None)
def _table(name, dtype=torch.float32):
    """The reference's table [b, n, h, w] for a case (ds-free), computed once."""
    from oracle import fusion
    from oracle.cloud import Cloud

    c = _case(name)
    B, H, W = c["B"], c["H"], c["W"]
    fr = dict(depth=torch.empty((B, 1, H, W, 1)), pose=c["poses"].to(dtype).unsqueeze(1), K=c["K"].to(dtype).unsqueeze(1))
    cloud = Cloud([c["points"][b, :n].to(dtype) for b, n in enumerate(c["counts"])])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "No active map points were found" (empty, behind)
        return fusion.find_active_map_points(cloud, fr)


@functools.lru_cache(maxsize=None)
def _ref(name, ds):
    """table (R, 4) filtered to the ds-grid, and per batch element n_k, tgt_pix and pix_start (numpy, int64)."""
    c = _case(name)
    t = _table(name).numpy()
    if ds > 0:
        t = t[(t[:, 2] % ds == 0) & (t[:, 3] % ds == 0)]
    out = dict(table=t, n=[], pix=[], start=[])
    if ds > 0:
        Wd = cdiv(c["W"], ds)
        npix = cdiv(c["H"], ds) * Wd
        for b in range(c["B"]):
            sel = t[t[:, 0] == b]
            pix = (sel[:, 2] // ds) * Wd + sel[:, 3] // ds
            out["n"].append(sel[:, 1]); out["pix"].append(pix)
            out["start"].append(np.concatenate([[0], np.cumsum(np.bincount(pix, minlength=npix))]))
    return out


# ---------------------------------------------------------------------------------------------- 1. CPU proof
@pytest.mark.parametrize("name", sorted(CASES))
def test_engineered_inputs_are_unambiguous(name):
    """The float32 and the float64 reference give the same table on every input set of this module (no row is exempt), and
    every hand-placed row meets the fate its name states."""
    c = _case(name)
    t32, t64 = _table(name), _table(name, torch.float64)
    assert t32.dtype == torch.int64 and torch.equal(t32, t64)
    H, W = c["H"], c["W"]
    ats = {at for hb in c["hand"].values() for at, _ in hb.values()}
    rows = {(r[0], r[1]): (r[2], r[3]) for r in t32.tolist() if r[1] in ats}
    placed = 0
    for b, hb in c["hand"].items():
        for nm, (at, px) in hb.items():
            assert rows.get((b, at)) == px, (name, b, nm, rows.get((b, at)), px)
            assert (px is None) == (nm.endswith("_out") or nm in ("z_zero", "z_neg")), nm
            placed += 1
        if hb:  # the names the issue lists are all there (the half pixels where the image has six pixels a side)
            want = {"u_lo_in", "u_lo_out", "u_hi_in", "u_hi_out", "v_lo_in", "v_lo_out", "v_hi_in", "v_hi_out", "z_zero", "z_neg", "on_grid"}
            assert want <= set(hb) and (W < 6 or {"half_u_1.5", "half_u_2.5", "half_u_3.5", "half_u_4.5"} <= set(hb))
            assert (H < 6 or {"half_v_1.5", "half_v_2.5", "half_v_3.5", "half_v_4.5"} <= set(hb)) and (W < 2 or "off_grid" in hb)
    if c["kind"] in ("mixed", "dense"):
        assert placed >= len(_hand(H, W)) * sum(n >= 4 * len(_hand(H, W)) for n in c["counts"]) and (placed > 0 or max(c["counts"]) == 0)
    # no row at or beyond an element's count, and the padded rows WOULD be active: the same arena with full counts
    cnt = torch.tensor(c["counts"])
    assert bool((t32[:, 1] < cnt[t32[:, 0]]).all())
    if name != "pa_big" and c["Nmax"] <= 2200:
        from oracle import fusion
        from oracle.cloud import Cloud

        fr = dict(depth=torch.empty((c["B"], 1, H, W, 1)), pose=c["poses"].unsqueeze(1), K=c["K"].unsqueeze(1))
        full = fusion.find_active_map_points(Cloud([c["points"][b] for b in range(c["B"])]), fr)
        for b, n in enumerate(c["counts"]):
            pad = full[(full[:, 0] == b) & (full[:, 1] >= n)]
            assert pad.shape[0] == c["Nmax"] - n and not pad[:, 2:].any(), (name, b)
    # what the kinds promise
    if c["kind"] == "perpix":
        for b, n in enumerate(c["counts"]):
            r = _ref(name, c["ds"])
            assert n == 0 or (len(r["pix"][b]) == n and np.array_equal(np.sort(r["pix"][b]), np.arange(n)))
    elif c["kind"] == "onepix":
        r = _ref(name, 1)
        assert all(len(set(p.tolist())) <= 1 for p in r["pix"]) and len(r["pix"][0]) == c["counts"][0]
    elif c["kind"] in ("behind",) or name == "empty":
        assert t32.shape[0] == 0
    elif c["kind"] == "dense":
        assert t32.shape[0] > 128 * 1024  # bucket_scatter_k's second grid-stride trip
    elif max(c["counts"]) >= 2077:  # mixed: in-frame rows, rows outside on every side, rows behind, rows on half pixels
        assert 0.4 * sum(c["counts"]) < t32.shape[0] < 0.9 * sum(c["counts"])
        for ds in (2, 4):
            assert 0 < _ref(name, ds)["table"].shape[0] < t32.shape[0] or H * W <= 16


# ---------------------------------------------------------------------------------------------- GPU side
def _poison(shape, dtype):
    """A device tensor whose every byte is 0xFF: NaN as a float, -1 as an integer."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _untouched(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == 0xFF).all())


def _dev(c):
    return dict(points=c["points"].to(DEV), normals=c["normals"].to(DEV), poses=c["poses"].to(DEV), K=c["K"].to(DEV),
                counts=torch.tensor(c["counts"], dtype=torch.int32, device=DEV))


def _project(c, d, ds, ws=None):
    """gs_project_active on poisoned buffers -> (rows buffer (B * Nmax, 4), count (1,)) on the device."""
    from gradslam_amd import _native as nv

    B, Nmax = c["B"], c["Nmax"]
    rows, cnt = _poison((B * Nmax, 4), torch.int64), _poison((1,), torch.int32)
    if ws is None:
        ws = _poison((nv.ws_bytes("gs_project_active_ws_bytes", B, Nmax),), torch.uint8)
    nv.call("gs_project_active", nv.ptr(d["points"]), nv.ptr(d["counts"]), B, Nmax, nv.ptr(d["poses"]), nv.ptr(d["K"]), c["H"], c["W"], ds,
            nv.ptr(rows), nv.ptr(cnt), nv.ptr(ws), ws.numel(), nv.stream())
    torch.cuda.synchronize()
    return rows, cnt


def _check_table(name, ds, rows, cnt):
    want = torch.from_numpy(_ref(name, ds)["table"])
    n = int(cnt)
    assert n == want.shape[0], (name, ds, n, want.shape[0])
    got = rows[:n].cpu()
    if not torch.equal(got, want):
        bad = (got != want).any(1).nonzero()[:, 0]
        print("%s ds=%d: %d of %d rows differ, first %s: got %s want %s" % (name, ds, len(bad), n, int(bad[0]), got[bad[0]].tolist(),
                                                                           want[bad[0]].tolist()))
    assert torch.equal(got, want), (name, ds)
    assert _untouched(rows[n:]), (name, ds, "rows beyond the count")


# ---- 1. gs_project_active
@pytest.mark.gpu
@pytest.mark.parametrize("ds", [0, 1, 2, 4])
@pytest.mark.parametrize("B", [1, 2, 32, 33])
def test_project_active_every_branch(gs, B, ds):
    """B <= 32: cameras in LDS (ActivePredL / ActiveWriterL); B = 33: build_cams_k and the Cam array (ActivePred / ActiveWriter)."""
    name = "pa_b%d" % B
    c = _case(name)
    rows, cnt = _project(c, _dev(c), ds)
    _check_table(name, ds, rows, cnt)
    # by name, on the device's table: every hand-placed row that the ds-grid keeps sits on its pixel, the others are absent
    got = {(int(r[0]), int(r[1])): (int(r[2]), int(r[3])) for r in rows[:int(cnt)].cpu()}
    for b, hb in c["hand"].items():
        for nm, (at, px) in hb.items():
            keep = px is not None and (ds <= 0 or (px[0] % ds == 0 and px[1] % ds == 0))
            assert got.get((b, at)) == (px if keep else None), (b, nm)


@pytest.mark.gpu
def test_project_active_scan_launch_under_the_cam_array(gs):
    """33 x 32768 rows are 1056 blocks: the compaction's scan launch, with rows in front of and behind its 1024-block carry."""
    c = _case("pa_big")
    assert c["B"] * c["Nmax"] > 1024 * 1024
    rows, cnt = _project(c, _dev(c), 2)
    _check_table("pa_big", 2, rows, cnt)
    t = _ref("pa_big", 2)["table"]
    assert (t[:, 0] == 0).any() and (t[:, 0] == 32).any()


# ---- 2. gs_build_icp_target / gs_bucket_by_pixel
_TARGET_OUT = (("tgt", 3, torch.float32), ("tnrm", 3, torch.float32), ("scan", 3, torch.float32), ("scan_orig", 1, torch.int32),
               ("tgt_index", 1, torch.int32), ("tgt_pix", 1, torch.int32))


def _target_ws(c, ds):
    from gradslam_amd import _native as nv

    return _poison((nv.ws_bytes("gs_build_icp_target_ws_bytes", c["B"], c["H"], c["W"], ds),), torch.uint8)


def _build_target(c, d, rows, cnt, ds, cap, optional=True, entry="gs_build_icp_target", ws=None):
    """One call on poisoned outputs (and a poisoned workspace unless one is handed in) -> dict of CPU tensors."""
    from gradslam_amd import _native as nv

    B, H, W, Nmax = c["B"], c["H"], c["W"], c["Nmax"]
    npix = cdiv(H, ds) * cdiv(W, ds)
    o = {k: _poison((B, cap, w) if w > 1 else (B, cap), dt) for k, w, dt in _TARGET_OUT}
    o["counts"], o["pix_start"] = _poison((B,), torch.int32), _poison((B, npix + 1), torch.int32)
    if ws is None:
        assert nv.ws_bytes("gs_bucket_by_pixel_ws_bytes", B, H, W, ds) == nv.ws_bytes("gs_build_icp_target_ws_bytes", B, H, W, ds)
        ws = _target_ws(c, ds)
    opt = [nv.ptr(o["tgt_index"]) if optional else None, nv.ptr(o["tgt_pix"]) if optional else None]
    if entry == "gs_build_icp_target":
        nv.call(entry, nv.ptr(rows), nv.ptr(cnt), B * Nmax, B, H, W, ds, nv.ptr(d["points"]), nv.ptr(d["normals"]), Nmax, cap, nv.ptr(o["tgt"]),
                nv.ptr(o["tnrm"]), nv.ptr(o["counts"]), nv.ptr(o["scan"]), nv.ptr(o["scan_orig"]), nv.ptr(o["pix_start"]), *opt, nv.ptr(ws),
                ws.numel(), nv.stream())
    else:
        nv.call(entry, nv.ptr(rows), nv.ptr(cnt), B * Nmax, B, H, W, ds, nv.ptr(d["points"]), Nmax, cap, nv.ptr(o["scan"]), nv.ptr(o["scan_orig"]),
                nv.ptr(o["pix_start"]), opt[1], nv.ptr(ws), ws.numel(), nv.stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check_buckets(n_k, pix, start, cap, scan, scan_orig, points, where):
    """The scan order of one batch element: scan_orig (>= min(count, cap)), scan (.., 3) against the reference rows n_k / pix /
    start.  Slots below cap hold distinct rows of their own pixel and that row's point; under a clamp a row k >= cap may sit
    in a slot < cap (the slot rule does not look at k), so the point is compared with the map's."""
    cnt = len(n_k)
    m = min(cnt, cap)
    orig = scan_orig[:m].long().numpy()
    assert ((orig >= 0) & (orig < cnt)).all(), where
    slot_pix = np.searchsorted(start, np.arange(m), side="right") - 1
    assert np.array_equal(pix[orig], slot_pix), (where, "a slot holds a row of another pixel")
    assert len(np.unique(orig)) == m, (where, "a row sits in two slots")
    if m == cnt:  # with both of the above: per pixel, the sorted slots ARE the rows of that pixel
        assert np.array_equal(np.sort(orig), np.arange(cnt)), where
    assert torch.equal(_bits(scan[:m]), _bits(points[torch.from_numpy(n_k[orig])])), (where, "scan point")


def _check_target(name, ds, cap, o, optional=True, gathered=True):
    c, r = _case(name), _ref(name, ds)
    for b in range(c["B"]):
        n_k, pix, start = r["n"][b], r["pix"][b], r["start"][b]
        m, where = min(len(n_k), cap), (name, ds, cap, b)
        idx = torch.from_numpy(n_k[:m])
        assert torch.equal(o["pix_start"][b].long(), torch.from_numpy(start)), where
        if gathered:
            assert int(o["counts"][b]) == len(n_k), where  # (the row count, not clamped to cap: see the header)
            assert torch.equal(_bits(o["tgt"][b, :m]), _bits(c["points"][b][idx])), where
            assert torch.equal(_bits(o["tnrm"][b, :m]), _bits(c["normals"][b][idx])), where
            if optional:
                assert torch.equal(o["tgt_index"][b, :m].long(), idx), where
        if optional:
            assert torch.equal(o["tgt_pix"][b, :m].long(), torch.from_numpy(pix[:m])), where
        _check_buckets(n_k, pix, start, cap, o["scan"][b], o["scan_orig"][b], c["points"][b], where)
        written = dict(scan=True, scan_orig=True, tgt=gathered, tnrm=gathered, tgt_index=gathered and optional, tgt_pix=optional)
        for k, _, _ in _TARGET_OUT:  # nothing at or beyond min(count, cap); outputs the call was not given stay whole
            assert _untouched(o[k][b, (m if written[k] else 0):]), (where, k)
    if not gathered:
        assert _untouched(o["counts"])


def _run_target_chain(name, ds, cap=None, dirty_from=None):
    c = _case(name)
    d = _dev(c)
    rows, cnt = _project(c, d, ds)
    _check_table(name, ds, rows, cnt)
    cap = cap or c["Nmax"]
    ws = None
    if dirty_from:  # the workspace another shape left behind, sized for the larger of the two
        c2 = _case(dirty_from[0])
        d2 = _dev(c2)
        rows2, cnt2 = _project(c2, d2, dirty_from[1])
        a, b = _target_ws(c, ds), _target_ws(c2, dirty_from[1])
        ws = a if a.numel() >= b.numel() else b
        _check_target(dirty_from[0], dirty_from[1], c2["Nmax"], _build_target(c2, d2, rows2, cnt2, dirty_from[1], c2["Nmax"], ws=ws))
    _check_target(name, ds, cap, _build_target(c, d, rows, cnt, ds, cap, ws=ws))
    _check_target(name, ds, cap, _build_target(c, d, rows, cnt, ds, cap, optional=False, ws=ws), optional=False)
    _check_target(name, ds, cap, _build_target(c, d, rows, cnt, ds, cap, entry="gs_bucket_by_pixel", ws=ws), gathered=False)
    _check_target(name, ds, cap, _build_target(c, d, rows, cnt, ds, cap, optional=False, entry="gs_bucket_by_pixel", ws=ws), optional=False,
                  gathered=False)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("npix", sorted(SHAPES))
def test_build_icp_target_and_bucket_by_pixel(gs, npix, B):
    """The batch chain on the table of gs_project_active, with and without the optional outputs.  B = 3 has an empty middle
    element, B = 33 several between non-empty ones."""
    H, W, ds = SHAPES[npix]
    assert cdiv(H, ds) * cdiv(W, ds) == npix
    _run_target_chain("t%d_b%d" % (npix, B), ds)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_pixel", "per_pixel_1025", "per_pixel_24577", "per_pixel_49153"])
def test_build_icp_target_one_pixel_and_one_point_per_pixel(gs, name):
    """Every point in one bin; every bin exactly one point (pix_start is then 0, 1, 2, .. across the tiles' carry)."""
    _run_target_chain(name, _case(name)["ds"])


@pytest.mark.gpu
def test_build_icp_target_on_a_dirty_workspace(gs):
    _run_target_chain("t1025_b3", 1, dirty_from=("t1056_b3", 2))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["t1056_b3", "t1025_b33", "one_pixel"])
def test_build_icp_target_capacity_clamps(gs, name):
    """cap below the row count of some elements (and above that of others): slots below cap are right, nothing at or beyond
    cap is written, counts and pix_start still state the whole row count."""
    ds = _case(name)["ds"]
    sizes = [len(n) for n in _ref(name, ds)["n"]]
    cap = 100
    assert max(sizes) > 2 * cap and any(0 < s for s in sizes)
    _run_target_chain(name, ds, cap=cap)


# ---- 3. the two one-sequence forms through gs_slam_localize
def _front(gs, name, ds, fused, ws=None):
    """gs_slam_localize with numiters = 0 on a 0xFF workspace -> (views of the loop's inputs, gvertex (H, W, 3), workspace)."""
    c = _case(name)
    d = _dev(c)
    H, W, Nmax = c["H"], c["W"], c["Nmax"]
    if ws is None:
        ws = _poison((gs._native.lib().gs_slam_localize_ws_bytes(1, H, W, ds, Nmax),), torch.uint8)
    depth = c["depth"].view(1, 1, H, W, 1).to(DEV).contiguous()
    res = localize(gs, depth, d["K"].view(1, 1, 4, 4), d["poses"].view(1, 1, 4, 4), d["points"], d["normals"], d["counts"], ds, 0, fused, ws)
    return res[5], res[3][0, 0], ws


def _check_front(name, ds, v, gV):
    c, r = _case(name), _ref(name, ds)
    H, W = c["H"], c["W"]
    # the source cloud
    keep = (c["depth"][::ds, ::ds] > 0).flatten()
    ns = int(v["ns"][0])
    assert ns == int(keep.sum()), (name, "ns")
    assert torch.equal(v["src_pix"][:ns].long(), keep.nonzero()[:, 0]), (name, "src_pix")
    assert torch.equal(_bits(v["src"][:3 * ns]), _bits(gV[::ds, ::ds].reshape(-1, 3)[keep].flatten())), (name, "src")
    # the target
    n_k, pix, start = r["n"][0], r["pix"][0], r["start"][0]
    nt = int(v["nt"][0])
    assert nt == len(n_k), (name, "nt", nt, len(n_k))
    idx = torch.from_numpy(n_k)
    assert torch.equal(_bits(v["tgt"][:3 * nt].view(-1, 3)), _bits(c["points"][0][idx])), (name, "tgt")
    assert torch.equal(_bits(v["tnrm"][:3 * nt].view(-1, 3)), _bits(c["normals"][0][idx])), (name, "tnrm")
    assert torch.equal(v["pix_start"].long(), torch.from_numpy(start)), (name, "pix_start")
    _check_buckets(n_k, pix, start, nt, v["scan"].view(-1, 3), v["scan_orig"], c["points"][0], name)
    assert torch.equal(_bits(v["scan"][:3 * nt].view(-1, 3)), _bits(v["tgt"][:3 * nt].view(-1, 3)[v["scan_orig"][:nt].long()]))
    return ns, nt


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("npix", [1025, 1056, 24576, 24577])
def test_one_sequence_front_ends_against_the_reference(gs, npix, fused):
    """project_front1 (fused, npix <= 24576) and project_target1 (switched off, or npix = 24577) on a depth frame with holes."""
    H, W, ds = SHAPES[npix]
    name = "t%d_b1" % npix
    v, gV, _ = _front(gs, name, ds, fused)
    ns, nt = _check_front(name, ds, v, gV)
    assert 0 < ns < npix and nt > 100
    c = _case(name)
    assert not c["depth"][::ds, ::ds].flatten()[0] and (ds == 1 or not c["depth"][1, 1])  # holes on the ds-grid and off it


@pytest.mark.gpu
def test_one_sequence_front_end_beyond_the_fused_limit_ignores_the_switch(gs):
    """24577 ds-grid pixels do not fit bucket_scatter_k's LDS: project_target1 runs whatever gs_set_fused_setup says.  One point
    per pixel makes every slot deterministic, so the two workspaces are the same byte for byte."""
    name = "per_pixel_24577"
    on, gV, ws_on = _front(gs, name, 1, True)
    off, _, ws_off = _front(gs, name, 1, False)
    _check_front(name, 1, on, gV)
    _check_front(name, 1, off, gV)
    assert torch.equal(ws_on, ws_off)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_one_sequence_front_end_second_stride_trip(gs, fused):
    """140 000 map points on a 128 x 192 grid, several per pixel: nt > 128 x 1024, bucket_scatter_k's second trip with its
    prefetched row (fused); tgt_scatter_gather1_k's grid-stride loop (separate)."""
    v, gV, _ = _front(gs, "dense", 1, fused)
    ns, nt = _check_front("dense", 1, v, gV)
    assert nt > 128 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("name", ["empty", "behind"])
def test_one_sequence_front_end_without_a_target(gs, name, fused):
    v, gV, _ = _front(gs, name, 1, fused)
    ns, nt = _check_front(name, 1, v, gV)
    assert nt == 0 and ns > 0 and not v["pix_start"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_one_sequence_front_end_on_a_dirty_workspace(gs, fused):
    """The workspace as the 63 x 65, ds = 2 call left it (other counters, other layout) serves the 25 x 41, ds = 1 call."""
    v, gV, ws = _front(gs, "t1056_b1", 2, fused)
    _check_front("t1056_b1", 2, v, gV)
    need = gs._native.lib().gs_slam_localize_ws_bytes(1, 25, 41, 1, _case("t1025_b1")["Nmax"])
    assert need <= ws.numel()
    v, gV, _ = _front(gs, "t1025_b1", 1, fused, ws=ws)
    _check_front("t1025_b1", 1, v, gV)


# ---- 4. gs_gather_table_rows, gs_table_ds_mask
def _gather(c, rows, cnt, attr, cap, with_counts=True):
    from gradslam_amd import _native as nv

    B, Nmax, C = attr.shape
    out, counts = _poison((B, max(cap, 1), C), torch.float32), _poison((B,), torch.int32)
    ws = _poison((nv.ws_bytes("gs_gather_table_rows_ws_bytes", B),), torch.uint8)
    nv.call("gs_gather_table_rows", nv.ptr(rows), nv.ptr(cnt), B * Nmax, nv.ptr(attr), B, Nmax, C, cap, nv.ptr(out),
            nv.ptr(counts) if with_counts else None, nv.ptr(ws), ws.numel(), nv.stream())
    torch.cuda.synchronize()
    return out.cpu(), counts.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("name", ["pa_b1", "pa_b33"])
def test_gather_table_rows(gs, name, C):
    """out[b, k] = attr[b, n_k] for the k-th table row of element b, k < cap; counts[b] = that element's row count.  With a cap
    that fits and one that clamps, with and without the counts output, and on an empty table."""
    c = _case(name)
    d = _dev(c)
    B, Nmax = c["B"], c["Nmax"]
    attr = (torch.rand((B, Nmax, C), generator=torch.Generator().manual_seed(C)) - 0.5)
    rows, cnt = _project(c, d, 2)
    r = _ref(name, 2)
    for cap in (Nmax, 100):
        for with_counts in (True, False):
            out, counts = _gather(c, rows, cnt, attr.to(DEV), cap, with_counts)
            for b in range(B):
                m = min(len(r["n"][b]), cap)
                assert torch.equal(_bits(out[b, :m]), _bits(attr[b][torch.from_numpy(r["n"][b][:m])])), (name, C, cap, b)
                assert _untouched(out[b, m:]), (name, C, cap, b)
            if with_counts:
                assert counts.tolist() == [len(n) for n in r["n"]], (name, C, cap)  # (the row count, not clamped: see the header)
            else:
                assert _untouched(counts)
    assert max(len(n) for n in r["n"]) > 100 and (B == 1 or min(len(n) for n in r["n"]) == 0)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, counts = _gather(c, rows, zero, attr.to(DEV), 100)
    assert _untouched(out) and counts.tolist() == [0] * B


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pa_b1", "pa_b33"])
def test_table_ds_mask(gs, name):
    from gradslam_amd import _native as nv

    c = _case(name)
    rows, cnt = _project(c, _dev(c), 0)
    n = int(cnt)
    t = torch.from_numpy(_ref(name, 0)["table"])
    assert n == t.shape[0] > 1024
    for ds in (1, 2, 4):
        mask = _poison((n + 8,), torch.uint8)
        nv.call("gs_table_ds_mask", nv.ptr(rows), n, ds, nv.ptr(mask), nv.stream())
        torch.cuda.synchronize()
        want = ((t[:, 2] % ds == 0) & (t[:, 3] % ds == 0)).to(torch.uint8)
        assert torch.equal(mask[:n].cpu(), want) and _untouched(mask[n:]) and (ds == 1 or 0 < int(want.sum()) < n)
    mask = _poison((8,), torch.uint8)
    nv.call("gs_table_ds_mask", nv.ptr(rows), 0, 2, nv.ptr(mask), nv.stream())
    torch.cuda.synchronize()
    assert _untouched(mask)
