"""gs.structures.Meshes on CPU tensors (container, geometry, PLY files), the ABI of gs_tsdf_faces and the error contracts of
ops.tsdf_faces_raw / TSDFVolume.extract_mesh.  Only the shape checks of the ops (which come after the device check) need a device."""
import os

import numpy as np
import pytest
import torch

import gradslam_amd as gs
from gradslam_amd import _native as nv
from gradslam_amd import ops

NEW_SYMBOLS = {"gs_tsdf_faces_ws_bytes": 4, "gs_tsdf_faces": 16}

TETRA_V = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
TETRA_F = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]  # counter-clockwise seen from outside


def cube_mesh(edge=2.0, shift=(0.5, -1.0, 3.0)):
    """8 corners, 12 outward triangles"""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float64) * edge + np.asarray(shift)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]  # -z +z -y +y -x +x, outward
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.asarray(f, np.int64)


def tetra(dtype=torch.float32, **kw):
    return gs.Meshes([torch.tensor(TETRA_V, dtype=dtype)], [torch.tensor(TETRA_F)], **kw)


# ------------------------------------------------------------------ the ABI
def test_mesh_symbols_load_and_are_declared():
    lib = nv.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in nv.SIGNATURES, name
        assert len(nv.SIGNATURES[name][1]) == nargs, name
        assert name + "(" in header, name
        decl = header[header.index(name + "("):]
        assert decl[: decl.index(";")].count(",") + 1 == nargs, name
    assert lib.gs_abi_version() == 3
    assert gs.structures.Meshes is gs.Meshes and hasattr(gs.TSDFVolume, "extract_mesh") and hasattr(ops, "tsdf_faces_raw")


def test_gs_tsdf_faces_refuses_bad_arguments_before_any_device_work():
    """Every check happens on the host before the first launch: the stand-in pointers below are never read."""
    lib = nv.lib()
    P = 4096
    nb = lambda n: -(-n // 1024)
    assert lib.gs_tsdf_faces_ws_bytes(2, 42, 22, 56) == 2 * (-(-(4 * 2 * nb(42 * 22 * 56)) // 256) * 256)
    assert lib.gs_tsdf_faces_ws_bytes(1, 2, 2, 2) == 512
    assert lib.gs_tsdf_faces_ws_bytes(0, 4, 4, 4) == 0 and lib.gs_tsdf_faces_ws_bytes(1, 4, 0, 4) == 0
    assert lib.gs_tsdf_faces_ws_bytes(1, 1024, 1024, 256) > 0  # 2^28 voxels
    assert lib.gs_tsdf_faces_ws_bytes(1, 1024, 1024, 257) == 0  # more: 5 faces per cube would not fit int32
    #     tsdf weight B nx ny nz minw edge n_points vcap fcap faces n_faces ws ws_bytes stream
    ok = [P, P, 1, 4, 4, 4, 1.0, P, P, 8, 8, P, P, P, 1 << 20, None]
    for pos in (0, 1, 12, 7, 8, 11):  # (the last three: rows need the edge list, its counts and the faces)
        args = list(ok)
        args[pos] = None
        assert lib.gs_tsdf_faces(*args) == -1, pos
    for pos, bad in ((2, 0), (2, 65536), (3, 0), (4, -2), (5, 0), (6, float("nan")), (9, -1), (10, -1)):
        args = list(ok)
        args[pos] = bad
        assert lib.gs_tsdf_faces(*args) == -1, (pos, bad)
    args = list(ok)
    args[3], args[4], args[5] = 1024, 1024, 257
    assert lib.gs_tsdf_faces(*args) == -1 and b"2^28" in lib.gs_last_error()
    args = list(ok)
    args[13], args[14] = None, 0
    assert lib.gs_tsdf_faces(*args) == -2
    args = list(ok)
    args[14] = lib.gs_tsdf_faces_ws_bytes(1, 4, 4, 4) - 1
    assert lib.gs_tsdf_faces(*args) == -2
    assert b"gs_tsdf_faces" in lib.gs_last_error()


def test_python_error_contracts():
    t, w = torch.ones(1, 4, 4, 4), torch.zeros(1, 4, 4, 4)
    e, n = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_faces_raw(t, w, 1.0, None, None, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tsdf_faces_raw(t, w, 1.0, e, n, 4)
    with pytest.raises(TypeError, match="tensor"):
        ops.tsdf_faces_raw([1.0], w, 1.0, None, None, 0)
    # an unconstructed volume with CPU state is enough: the ops look at the tensors before anything is launched
    vol = object.__new__(gs.TSDFVolume)
    vol._B, vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size = 1, t, w, None, (0.0, 0.0, 0.0), 0.1
    vol.device = torch.device("cpu")
    with pytest.raises(ValueError, match="no CPU fallback"):
        vol.extract_mesh()
    # (bad shapes on device tensors: test_device_ops_refuse_bad_shapes_with_the_house_messages)
    with pytest.raises(ValueError, match="same length"):
        gs.Meshes([torch.zeros(3, 3)], [torch.zeros(1, 3, dtype=torch.int64)] * 2)
    with pytest.raises(TypeError, match="lists"):
        gs.Meshes(torch.zeros(1, 3, 3), [torch.zeros(1, 3, dtype=torch.int64)])
    with pytest.raises(ValueError, match=r"shape \(V, 3\)"):
        gs.Meshes([torch.zeros(3, 2)], [torch.zeros(1, 3, dtype=torch.int64)])
    with pytest.raises(ValueError, match="integer"):
        gs.Meshes([torch.zeros(3, 3)], [torch.zeros(1, 3)])
    with pytest.raises(ValueError, match="index the 3 rows"):
        gs.Meshes([torch.zeros(3, 3)], [torch.tensor([[0, 1, 3]])])
    with pytest.raises(ValueError, match="normals"):
        gs.Meshes([torch.zeros(3, 3)], [torch.tensor([[0, 1, 2]])], normals=[torch.zeros(2, 3)])
    with pytest.raises(TypeError, match="int"):
        tetra().face_areas("0")
    with pytest.raises(IndexError):
        tetra().face_areas(1)


@pytest.mark.gpu
def test_device_ops_refuse_bad_shapes_with_the_house_messages():
    dev = "cuda:0"
    t, w = torch.ones(1, 4, 4, 4, device=dev), torch.zeros(1, 4, 4, 4, device=dev)
    e, n = torch.zeros(1, 4, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match=r"tsdf should have shape \(B, nz, ny, nx\)"):
        ops.tsdf_faces_raw(t[0], w[0], 1.0, None, None, 0)
    with pytest.raises(ValueError, match="weight should have the shape of tsdf"):
        ops.tsdf_faces_raw(t, w[:, :2], 1.0, None, None, 0)
    with pytest.raises(ValueError, match="min_weight should be a number"):
        ops.tsdf_faces_raw(t, w, float("nan"), None, None, 0)
    with pytest.raises(ValueError, match="fcap should lie in"):
        ops.tsdf_faces_raw(t, w, 1.0, e, n, -1)
    with pytest.raises(ValueError, match="need the edge list"):
        ops.tsdf_faces_raw(t, w, 1.0, None, n, 4)
    with pytest.raises(ValueError, match="edge should be int32"):
        ops.tsdf_faces_raw(t, w, 1.0, e.long(), n, 4)
    with pytest.raises(ValueError, match="n_points should be 1 int32"):
        ops.tsdf_faces_raw(t, w, 1.0, e, torch.zeros(2, dtype=torch.int32, device=dev), 4)
    with pytest.raises(ValueError, match="truncated"):
        ops.tsdf_faces_raw(t, w, 1.0, e, torch.full((1,), 5, dtype=torch.int32, device=dev), 4)


# ------------------------------------------------------------------ the container
def test_list_and_padded_views_round_trip_with_unequal_and_empty_meshes():
    cv, cf = cube_mesh()
    verts = [torch.tensor(TETRA_V), torch.zeros(0, 3), torch.tensor(cv, dtype=torch.float32)]
    faces = [torch.tensor(TETRA_F), torch.zeros(0, 3, dtype=torch.int64), torch.tensor(cf)]
    normals = [torch.randn(len(v), 3) for v in verts]
    colors = [torch.rand(len(v), 3) * 255 for v in verts]
    m = gs.Meshes(verts, faces, normals=normals, colors=colors)
    assert len(m) == 3 and m.has_normals and m.has_colors and m.device == torch.device("cpu")
    assert m.num_verts_per_mesh.tolist() == [4, 0, 8] and m.num_faces_per_mesh.tolist() == [4, 0, 12]
    assert m.verts_padded.shape == (3, 8, 3) and m.faces_padded.shape == (3, 12, 3) and m.faces_padded.dtype == torch.int32
    for b in range(3):
        assert torch.equal(m.verts_list[b], verts[b]) and torch.equal(m.faces_list[b].long(), faces[b])
        assert torch.equal(m.normals_list[b], normals[b]) and torch.equal(m.colors_list[b], colors[b])
        nv_, nf_ = len(verts[b]), len(faces[b])
        assert float(m.verts_padded[b, nv_:].abs().max() if nv_ < 8 else 0) == 0  # vertex attributes are padded with zeros
        assert float(m.normals_padded[b, nv_:].abs().max() if nv_ < 8 else 0) == 0
        assert bool((m.faces_padded[b, nf_:] == -1).all())                        # faces with -1
    again = gs.Meshes(m.verts_list, m.faces_list, normals=m.normals_list, colors=m.colors_list)
    assert torch.equal(again.verts_padded, m.verts_padded) and torch.equal(again.faces_padded, m.faces_padded)
    assert torch.equal(again.colors_padded, m.colors_padded)
    bare = gs.Meshes(verts, faces)
    assert not bare.has_normals and not bare.has_colors and bare.normals_list is None and bare.colors_padded is None
    # copies
    c = m.clone()
    assert torch.equal(c.verts_padded, m.verts_padded) and c.verts_padded.data_ptr() != m.verts_padded.data_ptr()
    assert m.to("cpu") is m and m.cpu() is m and m.to("cpu", copy=True).faces_padded.data_ptr() != m.faces_padded.data_ptr()
    leaf = torch.tensor(TETRA_V, requires_grad=True)
    g = gs.Meshes([leaf], [torch.tensor(TETRA_F)])
    assert g.verts_padded.requires_grad and not g.detach().verts_padded.requires_grad
    # the vertices as a point cloud: the same storage, the same graph
    pc = m.pointclouds()
    assert isinstance(pc, gs.Pointclouds) and len(pc) == 3 and pc.num_points_per_pointcloud.tolist() == [4, 0, 8]
    assert pc.points_padded.data_ptr() == m.verts_padded.data_ptr() and pc.has_normals and pc.has_colors
    assert torch.equal(pc.points_list[2], verts[2]) and torch.equal(pc.colors_list[0], colors[0])
    (g.pointclouds().points_padded * 2.0).sum().backward()
    assert torch.equal(leaf.grad, torch.full((4, 3), 2.0))


# ------------------------------------------------------------------ geometry against hand values
def test_tetrahedron_and_cube_against_hand_values():
    m = tetra(torch.float64)
    np.testing.assert_allclose(m.face_areas(0).numpy(), [0.5, 0.5, 0.5, np.sqrt(3) / 2], rtol=0, atol=1e-15)
    s = 1 / np.sqrt(3)
    np.testing.assert_allclose(m.face_normals(0).numpy(), [[0, 0, -1], [0, -1, 0], [-1, 0, 0], [s, s, s]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(m.volume().numpy(), [1 / 6], rtol=0, atol=1e-15)
    np.testing.assert_allclose(m.surface_area().numpy(), [1.5 + np.sqrt(3) / 2], rtol=0, atol=1e-15)
    assert m.face_vertices(0).shape == (4, 3, 3) and torch.equal(m.face_vertices(0)[3, 0], torch.tensor(TETRA_V[1], dtype=torch.float64))
    cv, cf = cube_mesh(edge=2.0)
    both = gs.Meshes([torch.tensor(TETRA_V, dtype=torch.float64), torch.tensor(cv)], [torch.tensor(TETRA_F), torch.tensor(cf)])
    np.testing.assert_allclose(both.volume().numpy(), [1 / 6, 8.0], rtol=0, atol=1e-12)  # (translation does not matter: closed)
    np.testing.assert_allclose(both.surface_area().numpy(), [1.5 + np.sqrt(3) / 2, 24.0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(both.face_areas(1).numpy(), np.full(12, 2.0), rtol=0, atol=1e-12)
    want = np.repeat(np.array([[0, 0, -1], [0, 0, 1], [0, -1, 0], [0, 1, 0], [-1, 0, 0], [1, 0, 0]], np.float64), 2, 0)
    np.testing.assert_allclose(both.face_normals(1).numpy(), want, rtol=0, atol=1e-15)
    # reversed faces: the negative volume, the opposite normals
    rev = gs.Meshes([torch.tensor(cv)], [torch.tensor(cf[:, ::-1].copy())])
    np.testing.assert_allclose(rev.volume().numpy(), [-8.0], rtol=0, atol=1e-12)
    # a zero-area face: area 0, normal 0, and no NaN in the gradient
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=torch.float64, requires_grad=True)
    deg = gs.Meshes([v], [torch.tensor([[0, 1, 2], [0, 1, 3]])])
    assert deg.face_areas(0).tolist() == [0.0, 0.5] and deg.face_normals(0)[0].tolist() == [0.0, 0.0, 0.0]
    (deg.surface_area().sum() + deg.face_normals(0).sum()).backward()
    assert torch.isfinite(v.grad).all()
    # an empty mesh
    e = gs.Meshes([torch.zeros(0, 3)], [torch.zeros(0, 3, dtype=torch.int64)])
    assert e.volume().tolist() == [0.0] and e.surface_area().tolist() == [0.0] and e.face_normals(0).shape == (0, 3)


def test_gradcheck_of_surface_area_and_volume():
    cv, cf = cube_mesh(edge=1.0)
    rng = np.random.RandomState(0)
    v0 = torch.tensor(cv + 0.1 * rng.randn(8, 3), requires_grad=True)
    v1 = torch.tensor(np.asarray(TETRA_V) + 0.1 * rng.randn(4, 3), requires_grad=True)
    faces = [torch.tensor(cf), torch.tensor(TETRA_F)]
    area = lambda a, b: gs.Meshes([a, b], faces).surface_area()
    vol = lambda a, b: gs.Meshes([a, b], faces).volume()
    assert torch.autograd.gradcheck(area, (v0, v1), eps=1e-6, atol=1e-8)
    assert torch.autograd.gradcheck(vol, (v0, v1), eps=1e-6, atol=1e-8)
    assert torch.autograd.gradcheck(lambda a, b: gs.Meshes([a, b], faces).face_normals(0), (v0, v1), eps=1e-6, atol=1e-7)


# ------------------------------------------------------------------ PLY files
def read_ply(path):
    """-> (names of the vertex properties, vertex columns as a dict, faces (F, 3)); little-endian binary or ascii"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    assert head[0] == "ply"
    binary = head[1] == "format binary_little_endian 1.0"
    assert binary or head[1] == "format ascii 1.0"
    nv_ = int([h for h in head if h.startswith("element vertex")][0].split()[2])
    nf_ = int([h for h in head if h.startswith("element face")][0].split()[2])
    props = [h.split()[1:] for h in head if h.startswith("property") and "list" not in h]
    assert "property list uchar int vertex_indices" in head
    dt = np.dtype([(n, {"float": "<f4", "uchar": "u1"}[t]) for t, n in props])
    if binary:
        vert = np.frombuffer(raw, dt, nv_, end)
        face = np.frombuffer(raw, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), nf_, end + nv_ * dt.itemsize)
        assert end + nv_ * dt.itemsize + nf_ * 13 == len(raw) and (face["n"] == 3).all()
        faces = face["v"]
    else:
        rows = raw[end:].decode("ascii").split("\n")
        assert rows[-1] == "" and len(rows) == nv_ + nf_ + 1
        vert = np.array([tuple(float(x) for x in r.split()) for r in rows[:nv_]], dtype=dt) if nv_ else np.zeros(0, dt)
        faces = np.array([[int(x) for x in r.split()] for r in rows[nv_: nv_ + nf_]], np.int64).reshape(-1, 4)
        assert (faces[:, 0] == 3).all()
        faces = faces[:, 1:]
    return [n for _, n in props], vert, np.asarray(faces, np.int64).reshape(-1, 3)


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
@pytest.mark.parametrize("attrs", [(), ("normals",), ("colors",), ("normals", "colors")], ids=["bare", "normals", "colors", "both"])
def test_save_ply_reads_back(tmp_path, binary, attrs):
    rng = np.random.RandomState(4)
    cv, cf = cube_mesh()
    verts = [torch.tensor(TETRA_V), torch.tensor((cv * np.pi + rng.randn(8, 3) * 1e-3).astype(np.float32)), torch.zeros(0, 3)]
    faces = [torch.tensor(TETRA_F), torch.tensor(cf), torch.zeros(0, 3, dtype=torch.int64)]
    normals = [torch.tensor(rng.randn(len(v), 3).astype(np.float32)) for v in verts] if "normals" in attrs else None
    colors = [torch.tensor(rng.uniform(-20, 280, (len(v), 3)).astype(np.float32)) for v in verts] if "colors" in attrs else None
    if colors is not None:
        colors[1][0] = torch.tensor([0.5, 1.5, 254.5])  # ties round to even: 0, 2, 254
    m = gs.Meshes(verts, faces, normals=normals, colors=colors)
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    for b in range(3):
        path = str(tmp_path / "m{}.ply".format(b))
        m.save_ply(path, index=b, binary=binary)
        names, vert, got_faces = read_ply(path)
        want = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + (["red", "green", "blue"] if colors else [])
        assert names == want
        assert len(vert) == len(verts[b]) and len(got_faces) == len(faces[b])
        assert np.array_equal(bits(np.stack([vert[n] for n in "xyz"], 1)), bits(verts[b].numpy()))  # bitwise, ascii too
        assert np.array_equal(got_faces, faces[b].numpy())
        if normals:
            assert np.array_equal(bits(np.stack([vert[n] for n in ("nx", "ny", "nz")], 1)), bits(normals[b].numpy()))
        if colors:
            rgb = np.stack([vert[n] for n in ("red", "green", "blue")], 1)
            assert rgb.dtype == np.uint8
            assert np.array_equal(rgb, np.clip(np.rint(colors[b].numpy().astype(np.float64)), 0, 255).astype(np.uint8))
            if b == 1:
                assert rgb[0].tolist() == [0, 2, 254] and rgb.min() == 0 and rgb.max() == 255
