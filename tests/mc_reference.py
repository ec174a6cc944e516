"""A numpy marching-cubes loop that reads nothing but the generated case table, and the table-independent topology checks the
mesh tests share (test_mc_table.py on the CPU, test_tsdf_mesh.py against the device)."""
import importlib.util
import os
from functools import lru_cache

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(REPO, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@lru_cache(maxsize=None)
def table():
    """(counts (256,), edges (256, 15)) as the generator builds them"""
    counts, edges = generator().build_table()
    return counts.astype(np.int64), edges.astype(np.int64)


def cube_cases(tsdf):
    """tsdf (nz, ny, nx) -> the case of every cube, (nz-1, ny-1, nx-1): bit c = dx + 2 dy + 4 dz set iff tsdf < 0 there"""
    nz, ny, nx = tsdf.shape
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        case |= (tsdf[dz: nz - 1 + dz, dy: ny - 1 + dy, dx: nx - 1 + dx] < 0).astype(np.int64) << c
    return case


def cubes_observed(obs):
    """obs (nz, ny, nx) bool -> all 8 corners observed, per cube"""
    nz, ny, nx = obs.shape
    out = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        out &= obs[dz: nz - 1 + dz, dy: ny - 1 + dy, dx: nx - 1 + dx]
    return out


def marching_cubes(tsdf, obs=None):
    """Faces as GLOBAL edge ids e = 3 j' + a (j' = (iz ny + iy) nx + ix the voxel at the edge's lower end), (F, 3) int64, in
    ascending cube id then table order; and the voxel id of every face's cube (F,).  A Python loop over the emitting cubes."""
    counts, edges = table()
    nz, ny, nx = tsdf.shape
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3), np.int64), np.zeros((0,), np.int64)
    case = cube_cases(tsdf)
    emit = counts[case] > 0
    if obs is not None:
        emit &= cubes_observed(obs)
    stride = (1, nx, nx * ny)
    faces, cube = [], []
    for iz, iy, ix in zip(*np.nonzero(emit)):  # (np.nonzero is z-major: ascending cube id)
        j = (iz * ny + iy) * nx + ix
        cs = case[iz, iy, ix]
        for k in edges[cs, : 3 * counts[cs]]:
            a, o1, o2 = k >> 2, k & 1, (k >> 1) & 1
            u, v = [x for x in range(3) if x != a]
            faces.append(3 * (j + o1 * stride[u] + o2 * stride[v]) + a)
        cube += [j] * int(counts[cs])
    return np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(cube, np.int64)


def edge_positions(tsdf, ids):
    """The crossing point of every edge id in grid units (voxel i at coordinate i), float64: (n, 3)"""
    nz, ny, nx = tsdf.shape
    f = tsdf.reshape(-1).astype(np.float64)
    j, a = ids // 3, ids % 3
    j1 = j + np.asarray([1, nx, nx * ny])[a]
    pos = np.stack([j % nx, (j // nx) % ny, j // (nx * ny)], 1).astype(np.float64)
    pos[np.arange(len(ids)), a] += f[j] / (f[j] - f[j1])
    return pos


def directed_edge_defects(faces):
    """Independent of any table: -> (directed edges that occur more than once, directed edges whose reverse does not
    occur).  Both 0 iff the mesh is closed, manifold along its edges and consistently oriented."""
    if len(faces) == 0:
        return 0, 0
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    m = int(f.max()) + 1
    fwd, fwd_n = np.unique(a * m + b, return_counts=True)
    rev = np.unique(b * m + a)
    repeated = int((fwd_n > 1).sum())
    unmatched = int((~np.isin(fwd, rev)).sum())  # (with repeated == 0 a reverse that occurs, occurs once)
    return repeated, unmatched


def euler_characteristic(faces):
    """V - E + F over the vertices the faces use"""
    f = np.asarray(faces, np.int64)
    und = np.unique(np.sort(np.stack([np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]])], 1), 1), axis=0)
    return len(np.unique(f)) - len(und) + len(f)


def signed_volume(pos, faces):
    """sum of v0 . (v1 x v2) / 6, float64"""
    v = pos[np.asarray(faces, np.int64)]
    return float((v[:, 0] * np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def grid(dims):
    """voxel index coordinates (x, y, z), each (nz, ny, nx) float64"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return x, y, z


def sphere_field(dims, radius_share=0.36):
    """distance to a sphere round the grid's centre, negative inside, positive on the border; (nz, ny, nx) float32"""
    x, y, z = grid(dims)
    c = [(n - 1) / 2.0 + 0.13 * (k + 1) for k, n in enumerate(dims)]  # off the lattice: no exact zeros
    r = radius_share * min(dims)
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)


def torus_field(dims, ring_share=0.29, tube_share=0.125):
    """distance to a torus round the z axis through the grid's centre, negative inside, positive on the border"""
    x, y, z = grid(dims)
    c = [(n - 1) / 2.0 + 0.07 * (k + 1) for k, n in enumerate(dims)]
    R, r = ring_share * min(dims), tube_share * min(dims)
    q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R
    return (np.sqrt(q ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)


def random_sign_field(dims, seed):
    """random values of both signs away from zero with a positive one-voxel border"""
    nx, ny, nz = dims
    rng = np.random.RandomState(seed)
    f = (rng.uniform(0.1, 1.0, (nz, ny, nx)) * rng.choice([-1.0, 1.0], (nz, ny, nx))).astype(np.float32)
    f[[0, -1]] = np.abs(f[[0, -1]])
    f[:, [0, -1]] = np.abs(f[:, [0, -1]])
    f[:, :, [0, -1]] = np.abs(f[:, :, [0, -1]])
    return f


def crossing_edges(tsdf, obs):
    """The extraction's rows in numpy: edge ids e = 3 j + a, ascending, of the grid edges whose two ends are observed and differ
    in the sign of tsdf (zero is outside) -> (e, j0, j1, axis), int64"""
    nz, ny, nx = tsdf.shape
    jidx = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    out = []
    for a in range(3):
        s0, s1 = [slice(None)] * 3, [slice(None)] * 3
        s0[2 - a], s1[2 - a] = slice(0, -1), slice(1, None)
        s0, s1 = tuple(s0), tuple(s1)
        cross = obs[s0] & obs[s1] & ((tsdf[s0] < 0) != (tsdf[s1] < 0))
        out.append(np.stack([3 * jidx[s0][cross] + a, jidx[s0][cross], jidx[s1][cross], np.full(int(cross.sum()), a)], 1))
    rows = np.concatenate(out)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


def reference_mesh(tsdf, obs):
    """-> (edge ids of the vertices (V,), faces as ROWS of that list (F, 3), the voxel id of every face's cube (F,)): every edge a
    face names must be a row (an emitting cube's crossing edges have observed ends)"""
    e = crossing_edges(tsdf, obs)[0]
    ids, cube = marching_cubes(tsdf, obs)
    rows = np.searchsorted(e, ids)
    assert ids.size == 0 or (rows.max() < len(e) and np.array_equal(e[rows], ids))
    return e, rows, cube
