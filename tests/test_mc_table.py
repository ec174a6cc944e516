"""The marching-cubes case table (tools/gen_mc_table.py -> gradslam_amd/csrc/gs_mc_table.hpp): derived by a rule, not copied.

The topology checks are independent of the table: a numpy marching-cubes loop (tests/mc_reference.py) reads only the table, and
the meshes it makes must be closed, manifold and consistently oriented -- every directed edge once, its reverse once."""
import os
import re

import numpy as np
import pytest

from tests import mc_reference as mc

HEADER = os.path.join(mc.REPO, "gradslam_amd", "csrc", "gs_mc_table.hpp")


def test_generator_reproduces_the_committed_header_byte_for_byte():
    with open(HEADER, "rb") as f:
        committed = f.read()
    assert committed == mc.generator().render_header().encode("ascii")
    rows = re.findall(rb"^\s*\{([^}]*)\},", committed, flags=re.M)
    assert len(rows) == 256
    counts, edges = mc.table()
    for case, row in enumerate(rows):  # the header's numbers are the table the tests read
        vals = [int(x) for x in row.split(b",")]
        assert len(vals) == 16 and vals[15] == counts[case] and vals[:15] == edges[case].tolist(), case


def test_known_answers_of_the_rule():
    counts, edges = mc.table()
    assert counts.shape == (256,) and edges.shape == (256, 15)
    assert int(counts.sum()) == 820 and int(counts.max()) == 5
    assert np.bincount(counts, minlength=6).tolist() == [2, 16, 50, 80, 76, 32]
    assert counts[0] == 0 and counts[255] == 0
    for case in range(256):
        used, unused = edges[case, : 3 * counts[case]], edges[case, 3 * counts[case]:]
        assert (unused == 255).all() and ((used >= 0) & (used < 12)).all(), case


def test_every_case_uses_exactly_its_crossing_edges_and_no_degenerate_triangle():
    counts, edges = mc.table()
    for case in range(256):
        crossing = set()
        for k in range(12):
            a, o1, o2 = k >> 2, k & 1, (k >> 1) & 1
            u, v = [x for x in range(3) if x != a]
            lo = [0, 0, 0]
            lo[u], lo[v] = o1, o2
            c0 = lo[0] + 2 * lo[1] + 4 * lo[2]
            c1 = c0 + (1, 2, 4)[a]
            if ((case >> c0) & 1) != ((case >> c1) & 1):
                crossing.add(k)
        tris = edges[case, : 3 * counts[case]].reshape(-1, 3)
        assert set(tris.reshape(-1).tolist()) == crossing, case
        assert all(len(set(t)) == 3 for t in tris.tolist()), case
        # a loop of n edges gives n - 2 triangles: with L loops, triangles = crossings - 2 L
        assert (len(crossing) - len(tris)) % 2 == 0 and len(tris) <= max(len(crossing) - 2, 0), case


def test_no_triangle_side_lies_in_a_cube_face_unless_it_is_a_segment_of_that_face():
    """A side of a triangle that joins two edges of one cube face lies in that face, where the neighbouring cube may draw it
    too.  Only the segments of the face rule may do that: they are the sides both cubes share, in opposite directions.  Every
    other side (a fan diagonal) must run through the cube's interior -- the fan of 18 loops starts later than at the lowest
    edge number for this."""
    counts, edges = mc.table()
    gen = mc.generator()
    faces_of = {}
    for k in range(12):
        a, o1, o2 = k >> 2, k & 1, (k >> 1) & 1
        u, v = [x for x in range(3) if x != a]
        faces_of[k] = {(u, o1), (v, o2)}  # the two faces an edge lies on: its offsets on the two other axes
    lowest_start = 0
    for case in range(256):
        seg = gen.case_segments(case)
        tris = edges[case, : 3 * counts[case]].reshape(-1, 3).tolist()
        for t in tris:
            for p, q in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                if faces_of[p] & faces_of[q]:
                    assert seg[p] == q, (case, t)  # a segment, in its direction
        # every segment is a side of exactly one triangle of the case
        sides = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
        assert all(sides.count((p, q)) == 1 for p, q in seg.items()), case
        lowest_start += sum(1 for t in tris if t[0] == min(seg))
    assert lowest_start > 0


def closed_and_oriented(tsdf):
    faces, cube = mc.marching_cubes(tsdf)
    assert len(faces) > 0 and (np.diff(cube) >= 0).all()
    assert mc.directed_edge_defects(faces) == (0, 0)
    ids = np.unique(faces)
    pos = mc.edge_positions(tsdf, ids)
    vol = mc.signed_volume(pos, np.searchsorted(ids, faces))
    return faces, vol


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_signs_give_a_closed_oriented_manifold(seed):
    """9 x 8 x 7 voxels of random sign inside a positive border: nearly every cube is a different case, ambiguous faces abound."""
    tsdf = mc.random_sign_field((9, 8, 7), seed)
    case = mc.cube_cases(tsdf)
    assert len(np.unique(case)) > 100
    faces, vol = closed_and_oriented(tsdf)
    assert vol > 0
    assert len(faces) == int(mc.table()[0][case].sum())


@pytest.mark.parametrize("seed", [11, 12])
def test_larger_random_volumes_stay_manifold(seed):
    """21 x 10 x 13: 2160 cubes.  With every fan started at its loop's lowest edge number these two volumes have 12 and more
    directed edges that occur twice (an in-face diagonal drawn by both cubes of an ambiguous face); 9 x 8 x 7 does not show it."""
    faces, vol = closed_and_oriented(mc.random_sign_field((21, 10, 13), seed))
    assert len(faces) > 5000 and vol > 0


def test_sphere_and_torus_have_their_euler_characteristics():
    for field, chi in ((mc.sphere_field, 2), (mc.torus_field, 0)):
        tsdf = field((12, 12, 12))
        assert (tsdf != 0).all() and (tsdf < 0).any()
        faces, vol = closed_and_oriented(tsdf)
        assert mc.euler_characteristic(faces) == chi, field.__name__
        assert vol > 0, field.__name__
    # the sphere's volume, roughly (linear interpolation of a distance field on a coarse grid)
    r = 0.36 * 12
    _, vol = closed_and_oriented(mc.sphere_field((12, 12, 12)))
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.05


def test_the_inverted_field_gives_the_mirrored_surface():
    """Negating the field swaps inside and outside: on a sphere (no ambiguous face) the same faces with the orientation reversed,
    a negative volume.  Zero is outside: a corner at exactly 0 behaves like a positive one."""
    inner = mc.sphere_field((12, 12, 12))[1:-1, 1:-1, 1:-1]
    faces_a, _ = mc.marching_cubes(inner)
    faces_b, _ = mc.marching_cubes(-inner)
    ids = np.unique(faces_a)
    canon = lambda f: sorted(tuple(np.roll(t, -int(np.argmin(t)))) for t in f.tolist())  # every face from its lowest vertex
    assert canon(faces_a) == canon(faces_b[:, ::-1])  # (no ambiguous face on a sphere: the same loops, walked backwards)
    pos = mc.edge_positions(inner, ids)
    va, vb = mc.signed_volume(pos, np.searchsorted(ids, faces_a)), mc.signed_volume(pos, np.searchsorted(ids, faces_b))
    assert va > 0 and vb < 0
    zero = mc.sphere_field((12, 12, 12)).copy()
    k = np.unravel_index(np.argmin(np.where(zero > 0, zero, np.inf)), zero.shape)  # the outside voxel nearest the surface
    moved = zero.copy()
    moved[k] = 0.0
    assert np.array_equal(mc.marching_cubes(zero)[0], mc.marching_cubes(moved)[0])
