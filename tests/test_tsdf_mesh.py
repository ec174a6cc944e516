"""Triangle meshes from TSDF volumes on the device: gs_tsdf_faces / ops.tsdf_faces_raw / TSDFVolume.extract_mesh.

References, written here and in tests/mc_reference.py in numpy, never taken from the code under test:
* faces: the case of every cube vectorised, a Python loop over the emitting cubes that reads only the generated table; the
  vertex rows from the numpy list of crossing edges.  Faces, counts and order are compared exactly; vertices, normals and colours
  bitwise against extract_pointcloud (whose own tests pin them against numpy);
* topology: every directed edge once and its reverse once -- independent of the table;
* gradients: the chain is cut at the vertices, which the device holds in fp32 and the first test pins bitwise.  Above the cut the
  loss (area + volume) is evaluated by the same formulas in float64 torch on the CPU at those vertices, with the faces held
  constant; below it the explicit float64 reverse formulas of the extraction (tests/test_tsdf.py: ref_extract_backward, there
  checked against float64 autograd) carry the float64 vertex adjoints to tsdf and color with the edge list held constant.
  The bound is c * 2^-24 * A per element, A the float64 sum of the absolute terms (grad_abs_terms below), c = 64 counted in
  test_gradients_against_the_float64_formulas.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import ops
from gradslam_amd.slam import KinectFusion
from gradslam_amd.synthetic import make_sequence
from tests import mc_reference as mc
from tests.test_meshes import read_ply
from tests.test_tsdf import DEV, H, TRUNC, U, V, W, fused, new_volume, ref_extract_backward, scene

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def volume_of(fields, weights=None, colors=None, v=0.05, origin=(-0.4, -0.3, 0.2)):
    """A TSDFVolume whose state is set directly: fields (B, nz, ny, nx) float32 numpy"""
    fields = np.asarray(fields, np.float32)
    B, nz, ny, nx = fields.shape
    vol = gs.TSDFVolume((nx, ny, nz), v, origin=origin, batch_size=B, color=colors is not None, device=DEV)
    vol.tsdf = torch.from_numpy(fields).to(DEV)
    vol.weight = torch.ones_like(vol.tsdf) if weights is None else torch.from_numpy(np.asarray(weights, np.float32)).to(DEV)
    if colors is not None:
        vol.color = torch.from_numpy(np.asarray(colors, np.float32)).to(DEV)
    return vol


def host_state(vol):
    return vol.tsdf.detach().cpu().numpy(), vol.weight.cpu().numpy()


def check_against_reference(vol, minw=1.0):
    """Check 1 of the issue for one volume -> (mesh, [reference (edge, faces, cube) per batch element])"""
    f, w = host_state(vol)
    B = len(vol)
    refs = [mc.reference_mesh(f[b], w[b] >= np.float32(minw)) for b in range(B)]
    nv, nf = [len(r[0]) for r in refs], [len(r[1]) for r in refs]
    mesh = vol.extract_mesh(minw)
    pc = vol.extract_pointcloud(minw)
    print("dims", tuple(vol.dims), "min_weight", minw, "vertices", nv, "faces", nf)
    assert isinstance(mesh, gs.Meshes) and len(mesh) == B
    assert mesh.num_verts_per_mesh.tolist() == nv and mesh.num_faces_per_mesh.tolist() == nf
    assert mesh.faces_padded.dtype == torch.int32 and tuple(mesh.faces_padded.shape) == (B, max(nf), 3)
    # the vertices are the point cloud's rows, bit for bit and in order
    bits = lambda x: x.detach().cpu().numpy().view(np.uint32)
    assert tuple(mesh.verts_padded.shape) == (B, max(nv), 3)
    assert np.array_equal(bits(mesh.verts_padded), bits(pc.points_padded)) and np.array_equal(bits(mesh.normals_padded), bits(pc.normals_padded))
    assert mesh.has_colors == vol.has_colors
    if vol.has_colors:
        assert np.array_equal(bits(mesh.colors_padded), bits(pc.colors_padded))
    faces = mesh.faces_padded.cpu().numpy()
    for b in range(B):
        assert np.array_equal(faces[b, : nf[b]], refs[b][1]), b  # the faces, their count and their order
        assert (faces[b, nf[b]:] == -1).all(), b
    # the counting call, and the raw op on the extraction's own edge list
    none, n0 = ops.tsdf_faces_raw(vol.tsdf, vol.weight, minw, None, None, fcap=0)
    assert none is None and n0.dtype == torch.int32 and n0.tolist() == nf
    if max(nf) > 0:
        _, _, _, edge, n_points = ops.tsdf_extract_raw(vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, minw, cap=max(nv))
        for b in range(B):
            assert np.array_equal(edge[b, : nv[b]].cpu().numpy(), refs[b][0])
        cap = max(nf) + 3  # rows past the count hold -1
        raw, n1 = ops.tsdf_faces_raw(vol.tsdf, vol.weight, minw, edge, n_points, fcap=cap)
        assert n1.tolist() == nf and torch.equal(raw[:, : max(nf)], mesh.faces_padded) and bool((raw[:, max(nf):] == -1).all())
        short = max(1, min(nf) // 2)  # fewer rows than faces: the first rows, the full count
        raw, n2 = ops.tsdf_faces_raw(vol.tsdf, vol.weight, minw, edge, n_points, fcap=short)
        assert n2.tolist() == nf and torch.equal(raw, mesh.faces_padded[:, :short])
    return mesh, refs


def euler_of(faces):
    return mc.euler_characteristic(faces)


# ------------------------------------------------------------------ 1: faces, counts and order against numpy
def test_one_cube_volumes_of_several_cases():
    """(2, 2, 2): one cube per batch element -- a corner, an ambiguous face, the hardest case, its complement, nothing."""
    cases = [0b00000001, 0b00001001, 0b01101001, 0b10010110, 0b11111111, 0]
    rng = np.random.RandomState(0)
    fields = np.stack([np.where([(cs >> c) & 1 for c in range(8)], -1.0, 1.0).reshape(2, 2, 2) * rng.uniform(0.2, 1, (2, 2, 2)) for cs in cases])
    mesh, refs = check_against_reference(volume_of(fields))
    counts = mc.table()[0]
    assert mesh.num_faces_per_mesh.tolist() == [int(counts[cs]) for cs in cases] == [1, 2, 4, 4, 0, 0]
    assert mesh.num_verts_per_mesh.tolist() == [3, 6, 12, 12, 0, 0]


@pytest.mark.parametrize("dims", [(1, 5, 4), (6, 1, 3)])
def test_volumes_without_cubes_have_vertices_and_no_faces(dims):
    f = mc.random_sign_field((dims[0] + 2, dims[1] + 2, dims[2] + 2), 5)[1:-1, 1:-1, 1:-1]
    mesh, _ = check_against_reference(volume_of(np.stack([f, -f])))
    assert mesh.num_faces_per_mesh.tolist() == [0, 0] and min(mesh.num_verts_per_mesh.tolist()) > 0
    assert tuple(mesh.faces_padded.shape) == (2, 0, 3)
    assert mesh.surface_area().tolist() == [0.0, 0.0] and mesh.volume().tolist() == [0.0, 0.0]


@pytest.mark.parametrize("minw", [1.0, 2.0])
def test_common_scene_matches_the_numpy_reference(minw):
    """dims (42, 22, 56), B = 2: nx is no multiple of 4 or 64, cubes straddle block boundaries, the region is partly observed,
    the counts differ (the -1 padding shows)."""
    vol = fused()
    mesh, refs = check_against_reference(vol, minw)
    nv, nf = mesh.num_verts_per_mesh.tolist(), mesh.num_faces_per_mesh.tolist()
    assert min(nf) > 500 and nf[0] != nf[1] and nv[0] != nv[1]
    f, w = host_state(vol)
    for b in range(2):
        obs = mc.cubes_observed(w[b] >= np.float32(minw))
        assert 0 < obs.sum() < obs.size  # partly observed
        assert len(np.unique(refs[b][1])) <= nv[b]  # (a vertex on the rim of the observed region may be referenced by no face)
        assert len(np.unique(refs[b][2] // 1024)) > 10  # the faces' cubes lie in many blocks


@lru_cache(maxsize=None)
def big_sphere():
    """130 x 97 x 100 = 1 261 000 voxels: 1232 blocks of 1024 voxel ids, more than one pass of the 1024-thread scanning block (and
    more than kSelfScanBlocks)."""
    dims = (130, 97, 100)
    assert -(-dims[0] * dims[1] * dims[2] // 1024) > 1024
    return volume_of(mc.sphere_field(dims)[None], v=0.01, origin=(-0.6, -0.5, 0.4))


def test_block_counts_beyond_one_pass_of_the_scan():
    mesh, refs = check_against_reference(big_sphere())
    faces = refs[0][1]
    assert len(faces) > 40000 and refs[0][2].max() // 1024 > 1024
    assert mc.directed_edge_defects(faces) == (0, 0) and euler_of(faces) == 2
    r = 0.36 * 97 * 0.01
    assert abs(float(mesh.volume()[0]) / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.01
    assert abs(float(mesh.surface_area()[0]) / (4.0 * np.pi * r ** 2) - 1.0) < 0.01


# ------------------------------------------------------------------ 2: topology on the device, independent of the table
def test_random_signs_fully_observed_are_closed_manifold_and_oriented():
    dims = (21, 10, 13)
    vol = volume_of(np.stack([mc.random_sign_field(dims, s) for s in (11, 12)]))
    mesh = vol.extract_mesh()
    for b in range(2):
        faces = mesh.faces_list[b].cpu().numpy()
        assert len(faces) > 2000 and faces.min() >= 0
        assert mc.directed_edge_defects(faces) == (0, 0)
        assert len(np.unique(faces)) == int(mesh.num_verts_per_mesh[b])  # fully observed: every vertex is used
        assert len(np.unique(mc.cube_cases(host_state(vol)[0][b]))) > 200
    assert (mesh.volume() > 0).all()


def test_random_weights_every_face_lies_in_an_observed_cube():
    dims = (21, 10, 13)
    nx, ny, nz = dims
    rng = np.random.RandomState(3)
    f = np.stack([mc.random_sign_field(dims, s) for s in (21, 22)])
    w = rng.choice([0.0, 0.5, 1.0, 3.0], f.shape, p=[0.05, 0.05, 0.45, 0.45]).astype(np.float32)
    vol = volume_of(f, weights=w)
    minw = 1.0
    mesh = vol.extract_mesh(minw)
    edge = ops.tsdf_extract_raw(vol.tsdf, vol.weight, None, vol.origin, vol.voxel_size, minw, cap=int(mesh.num_verts_per_mesh.max()))[3].cpu().numpy()
    counts = mc.table()[0]
    for b in range(2):
        obs_cube = mc.cubes_observed(w[b] >= minw)
        assert 0.3 < obs_cube.mean() < 0.9
        assert int(mesh.num_faces_per_mesh[b]) == int(counts[mc.cube_cases(f[b])][obs_cube].sum())
        faces = mesh.faces_list[b].cpu().numpy()
        assert faces.min() >= 0
        assert len(np.unique(faces)) < int(mesh.num_verts_per_mesh[b])  # vertices no observed cube touches: kept, referenced by no face
        ids = edge[b][faces]  # (F, 3) edge ids
        j, a = ids // 3, ids % 3
        lo = np.stack([j % nx, (j // nx) % ny, j // (nx * ny)], -1)  # (F, 3 corners, xyz): the lower end of every edge
        hi = lo + np.eye(3, dtype=np.int64)[a]
        # the cubes that contain all three edges: lowest corner q with q <= lo and hi <= q + 1 on every axis
        qmin, qmax = (hi.max(1) - 1).clip(min=0), lo.min(1)
        ok = np.zeros(len(faces), bool)
        for dx in range(2):
            for dy in range(2):
                for dz in range(2):
                    q = qmin + np.array([dx, dy, dz])
                    inside = ((q >= qmin) & (q <= qmax) & (q < np.array([nx - 1, ny - 1, nz - 1]))).all(1)
                    qq = np.minimum(q, [nx - 2, ny - 2, nz - 2])
                    ok |= inside & obs_cube[qq[:, 2], qq[:, 1], qq[:, 0]]
        assert ok.all()


# ------------------------------------------------------------------ 3: orientation
@lru_cache(maxsize=None)
def solids():
    """a sphere and a torus, fully observed, with colours: B = 2 of dims (24, 20, 22)"""
    dims = (24, 20, 22)
    rng = np.random.RandomState(8)
    f = np.stack([mc.sphere_field(dims), mc.torus_field(dims, ring_share=0.3, tube_share=0.13)])
    return volume_of(f / 4.0, colors=rng.uniform(0, 255, f.shape + (3,)))


def test_sphere_and_torus_are_oriented_outwards():
    vol = solids()
    mesh, refs = check_against_reference(vol)
    assert (mesh.volume() > 0).all()
    assert [euler_of(mesh.faces_list[b].cpu().numpy()) for b in range(2)] == [2, 0]
    for b in range(2):
        assert mc.directed_edge_defects(mesh.faces_list[b].cpu().numpy()) == (0, 0)
        fn, area = mesh.face_normals(b), mesh.face_areas(b)
        vn = mesh.normals_list[b][mesh.faces_list[b].long()].mean(1)  # the mean of the three vertex normals
        live = area > 1e-6 * area.max()
        dots = (fn * vn).sum(-1)[live]
        print("b", b, "faces", len(fn), "non-degenerate", int(live.sum()), "min dot", float(dots.min()))
        assert int(live.sum()) > 0.9 * len(fn) and float(dots.min()) > 0.0


# ------------------------------------------------------------------ 4: exact zeros, nothing observed
def test_exact_zeros_count_as_outside_and_nothing_is_nan():
    f = mc.sphere_field((24, 20, 22)) / 4.0
    shell_out = (f > 0) & (f < 0.2)
    shell_in = (f < 0) & (f > -0.2)
    rng = np.random.RandomState(1)
    z = f.copy()
    z[shell_out & (rng.uniform(size=f.shape) < 0.5)] = 0.0  # outside voxels at exactly zero: vertices at s = 0 on their edges
    z2 = f.copy()
    z2[shell_in & (rng.uniform(size=f.shape) < 0.3)] = 0.0  # inside voxels raised to zero: they become outside
    z2[shell_out & (rng.uniform(size=f.shape) < 0.2)] = -0.0  # minus zero is zero
    vol = volume_of(np.stack([z, z2]))
    assert int((vol.tsdf == 0).sum()) > 200
    mesh, refs = check_against_reference(vol)
    assert min(mesh.num_faces_per_mesh.tolist()) > 500
    for b in range(2):
        assert mc.directed_edge_defects(refs[b][1]) == (0, 0)  # still closed: coincident vertices stay distinct rows
    t = vol.tsdf.clone().requires_grad_(True)
    m2 = vol._with_state(t, vol.weight, None).extract_mesh()
    for x in (m2.verts_padded, m2.normals_padded, m2.face_normals(0), m2.face_areas(1), m2.surface_area(), m2.volume()):
        assert bool(torch.isfinite(x).all())
    assert int((m2.face_areas(0) == 0).sum()) > 0  # zero-area faces exist (several vertices at one voxel centre) ...
    (m2.surface_area().sum() + m2.volume().sum()).backward()
    assert bool(torch.isfinite(t.grad).all())      # ... and give no NaN


def test_a_min_weight_that_observes_nothing_gives_empty_meshes():
    vol = fused()
    mesh = vol.extract_mesh(min_weight=1e9)
    assert len(mesh) == 2 and mesh.num_verts_per_mesh.tolist() == [0, 0] and mesh.num_faces_per_mesh.tolist() == [0, 0]
    assert tuple(mesh.verts_padded.shape) == (2, 0, 3) and tuple(mesh.faces_padded.shape) == (2, 0, 3) and mesh.has_colors
    assert mesh.surface_area().tolist() == [0.0, 0.0] and len(mesh.pointclouds()) == 2
    fresh = new_volume().extract_mesh()  # nothing integrated yet
    assert fresh.num_verts_per_mesh.tolist() == [0, 0] and fresh.num_faces_per_mesh.tolist() == [0, 0]


# ------------------------------------------------------------------ 5: gradients
def mesh_loss(mesh, wc):
    return mesh.surface_area().sum() + mesh.volume().sum() + (mesh.colors_padded * wc).sum()


def abs_cross(a, b):
    """the cross product with every product and difference replaced by absolute values and sums"""
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)


def grad_abs_terms(verts, faces):
    """Per vertex and component, the float64 sum of the absolute terms of d(area + volume) / d verts at the fp32 vertices.
    Volume: d/dv0 = (v1 x v2) / 6 -> (|v1| x |v2|) / 6 with the abs cross.  Area: d/dv0 = 0.5 (v1 - v2) x n, n = c / |c|,
    c = (v1 - v0) x (v2 - v0): the differences of fp32 numbers carry one rounding each, the cancellation sits in c, whose
    absolute evaluation is C = |v1 - v0| x |v2 - v0| (abs cross); to first order the error of n_i is bounded, in units of the
    roundings, by nbar_i = C_i / |c| + |n_i| (sum_j |c_j| C_j) / |c|^2 >= |n_i|, and the term by 0.5 |v1 - v2| x nbar.
    A face whose c is exactly zero has a zero area gradient on both sides (the where of face_areas)."""
    fv = verts[faces]  # (F, 3, 3) float64
    out = np.zeros_like(verts)
    d1, d2 = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]
    c = np.cross(d1, d2)
    C = abs_cross(np.abs(d1), np.abs(d2))
    nc = np.sqrt((c * c).sum(1))
    live = nc > 0
    safe = np.where(live, nc, 1.0)[:, None]
    nbar = np.where(live[:, None], C / safe + np.abs(c) / safe * ((np.abs(c) * C).sum(1, keepdims=True) / safe ** 2), 0.0)
    for k in range(3):
        v1, v2 = fv[:, (k + 1) % 3], fv[:, (k + 2) % 3]
        term = abs_cross(np.abs(v1), np.abs(v2)) / 6.0 + 0.5 * abs_cross(np.abs(v1 - v2), nbar)
        np.add.at(out, faces[:, k], term)
    return out


def float64_vertex_adjoints(verts32, faces):
    """d(area + volume) / d verts by the same formulas in float64 torch on the CPU, at the fp32 vertices, faces constant"""
    v = torch.from_numpy(verts32.astype(np.float64)).requires_grad_(True)
    fv = v[torch.from_numpy(faces)]
    c = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=-1)
    sq = (c * c).sum(-1)
    area = 0.5 * torch.sqrt(sq[sq > 0]).sum()
    vol = (fv[:, 0] * torch.cross(fv[:, 1], fv[:, 2], dim=-1)).sum() / 6.0
    (area + vol).backward()
    return v.grad.numpy(), float(area.detach()), float(vol.detach())


def device_grads(vol, wc):
    t, c = vol.tsdf.detach().clone().requires_grad_(True), vol.color.detach().clone().requires_grad_(True)
    mesh = vol._with_state(t, vol.weight, c).extract_mesh()
    mesh_loss(mesh, wc).backward()
    return mesh, t.grad, c.grad


@pytest.mark.parametrize("which", ["solids", "scene"])
def test_gradients_against_the_float64_formulas(which):
    """c = 64 from the roundings of one term's path.  Above the cut, per face and vertex: two differences (2), the cross product
    (3), the sum of squares (5), the square root (1), the division (1), the reverse cross product (3) = 15 for the area, 4 for
    the volume; the index's reverse pass adds the faces of a vertex one by one: an edge belongs to 4 cubes of at most 5
    triangles, at most 20 additions; the two loss terms meet in one more: 36.  Below it the extraction's reverse pass: about 10
    per term (tests/test_tsdf.py) and the 6 passes that add a voxel's edges: 16.  52, stated as the next power of two."""
    vol = solids() if which == "solids" else fused()
    B = len(vol)
    g = torch.Generator(device="cpu").manual_seed(5)
    mesh0 = vol.extract_mesh()
    wc = (torch.randn(tuple(mesh0.colors_padded.shape), generator=g) / 255.0).to(DEV)
    mesh, g_t, g_c = device_grads(vol, wc)
    f, w = host_state(vol)
    col = vol.color.cpu().numpy()
    v32 = np.float32(vol.voxel_size)
    for b in range(B):
        nv, nf = int(mesh.num_verts_per_mesh[b]), int(mesh.num_faces_per_mesh[b])
        e, j0, j1, axis = mc.crossing_edges(f[b], w[b] >= 1.0)
        assert nv == len(e)
        verts = mesh.verts_list[b].detach().cpu().numpy()
        faces = mesh.faces_list[b].cpu().numpy().astype(np.int64)
        g_v, area, volume = float64_vertex_adjoints(verts, faces)
        assert abs(area - float(mesh.surface_area()[b].detach())) <= (nf + 16) * U * area  # (a sum of nf positive fp32 terms of about 16 roundings)
        wcb = wc[b, :nv].cpu().numpy().astype(np.float64)
        want_t, want_c = ref_extract_backward(f[b], col[b], v32, j0, j1, axis, g_v, wcb)
        A_t, A_c = ref_extract_backward(f[b], col[b], v32, j0, j1, axis, grad_abs_terms(verts.astype(np.float64), faces), wcb, absolute=True)
        got_t, got_c = g_t[b].reshape(-1).cpu().numpy().astype(np.float64), g_c[b].reshape(-1, 3).cpu().numpy().astype(np.float64)
        err_t, err_c = np.abs(got_t - want_t), np.abs(got_c - want_c)
        hit = A_t > 0
        print(which, "b", b, "vertices", nv, "faces", nf, "voxels with a gradient", int(hit.sum()), "max |g_tsdf|", np.abs(want_t).max(),
              "max err / (u A): tsdf", (err_t[hit] / (U * A_t[hit])).max(), "color", (err_c[A_c > 0] / (U * A_c[A_c > 0])).max())
        assert hit.sum() > 500 and np.abs(want_t).max() > 0 and np.abs(want_c).max() > 0
        assert (got_t[~hit] == 0).all() and (got_c[A_c == 0] == 0).all()
        assert (err_t <= 64 * U * A_t).all()
        assert (err_c <= 64 * U * A_c).all()


def test_gradients_are_the_same_bits_from_run_to_run():
    vol = fused()
    wc = torch.full(tuple(vol.extract_mesh().colors_padded.shape), 1.0 / 255.0, device=DEV)
    torch.use_deterministic_algorithms(True)
    try:
        _, t1, c1 = device_grads(vol, wc)
        _, t2, c2 = device_grads(vol, wc)
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(t1, t2) and torch.equal(c1, c2) and float(t1.abs().max()) > 0


def test_gradients_reach_the_depth_and_rgb_images_through_integrate():
    """The whole graph depth, rgb -> integrate -> extract_mesh -> loss in one backward equals, bit for bit, the two halves run
    one after the other (the adjoints of the state from the mesh, then the integration's reverse pass on them: exact sums)."""
    colors, depths, K, poses = scene()
    depth, rgb = depths.clone().requires_grad_(True), colors.clone().requires_grad_(True)
    vol = new_volume().integrate(gs.RGBDImages(rgb, depth, K, poses))
    mesh = vol.extract_mesh()
    wc = torch.full(tuple(mesh.colors_padded.shape), 1.0 / 255.0, device=DEV)
    torch.use_deterministic_algorithms(True)
    try:
        mesh_loss(mesh, wc).backward()
        _, g_t, g_c = device_grads(fused(), wc)
    finally:
        torch.use_deterministic_algorithms(False)
    assert depth.grad is not None and bool(torch.isfinite(depth.grad).all()) and bool(torch.isfinite(rgb.grad).all())
    assert int((depth.grad != 0).sum()) > 500 and int((rgb.grad != 0).sum()) > 500
    fresh = new_volume()
    _, _, g_depth, g_rgb = ops.tsdf_integrate_backward_raw(depths, K, poses, fresh.weight, fresh.origin, V, TRUNC, fresh.max_weight, g_t, g_c)
    assert torch.equal(g_depth.view_as(depth.grad), depth.grad) and torch.equal(g_rgb.view_as(rgb.grad), rgb.grad)


# ------------------------------------------------------------------ 6: end to end
def test_kinectfusion_to_a_ply_file(tmp_path):
    colors, depths, K, poses = (t.to(DEV) for t in make_sequence(1, 4, H, W, seed=0))
    slam = KinectFusion(dims=(56, 40, 24), voxel_size=0.05, origin=[(-1.4, -1.0, 1.4)], trunc=0.15, odom="icp", device=DEV)
    with torch.no_grad():
        volume, _ = slam(gs.RGBDImages(colors, depths, K, poses))
    mesh = volume.extract_mesh()
    nv, nf = int(mesh.num_verts_per_mesh[0]), int(mesh.num_faces_per_mesh[0])
    assert nv > 1000 and nf > 1000 and mesh.has_colors and mesh.has_normals
    path = str(tmp_path / "kf.ply")
    mesh.save_ply(path)
    names, vert, faces = read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert len(vert) == nv and len(faces) == nf and faces.min() >= 0 and faces.max() < nv
    assert np.array_equal(np.stack([vert[n] for n in "xyz"], 1).view(np.uint32), mesh.verts_list[0].cpu().numpy().view(np.uint32))
    assert np.array_equal(faces, mesh.faces_list[0].cpu().numpy())
    assert float(mesh.surface_area()[0]) > 1.0  # the wall: a few square metres
