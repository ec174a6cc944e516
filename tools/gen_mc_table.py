#!/usr/bin/env python3
"""The marching-cubes case table of gs_tsdf_faces, DERIVED by a rule and written to gradslam_amd/csrc/gs_mc_table.hpp.

    python tools/gen_mc_table.py            # rewrite the header
    python tools/gen_mc_table.py --check    # exit 1 if the committed header differs

The rule ("T", meshes):
* corner c = dx + 2 dy + 4 dz of a cube; case bit c is set iff the corner is inside (tsdf < 0; zero is outside);
* cube edge k = 4 a + o1 + 2 o2 runs along axis a from the corner whose offsets on the two OTHER axes (ascending axis order)
  are o1 and o2; its global vertex is edge slot 3 j' + a of gs_tsdf_extract, j' the voxel at the edge's lower end;
* on each of the six faces the crossing edges are joined into directed segments: walking round the face counter-clockwise as
  seen from outside the cube, every maximal run of inside corners is entered over one crossing edge and left over another, and
  the segment leads from the first to the second.  Two crossings: one segment.  Four crossings (the ambiguous face): two
  segments, each round ONE inside corner -- the face's four signs alone decide, so the two cubes that share it agree.  Seen
  from outside the cube the outside (tsdf >= 0) lies to the left of a segment;
* every crossing edge then has one outgoing and one incoming segment: they close into loops, taken in ascending order of their
  lowest edge number; a loop is fanned into (v0, v_i, v_i+1) from its lowest edge number -- unless a diagonal (v0, v_i) of that
  fan would join two edges of one cube face.  Such a diagonal lies IN the face (a loop can cross an ambiguous face twice), and
  the cube behind the face may draw the same one: four triangles on one edge.  Then the fan starts at the next edge of the
  loop, in loop order, whose fan has no such diagonal (18 loops of the 256 cases need it; every one of them has such a start).  Every diagonal then runs
  through its cube's interior and every segment is shared by exactly two cubes in opposite directions: the mesh is a closed
  oriented manifold wherever all cubes emit.
The triangles run counter-clockwise seen from free space.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gradslam_amd", "csrc", "gs_mc_table.hpp")
MAX_TRIS = 5
NONE = 255  # an unused slot of a case's 15 edge numbers


def other_axes(a):
    """the two axes that are not a, ascending"""
    return tuple(k for k in range(3) if k != a)


def corner_id(d):
    return d[0] + 2 * d[1] + 4 * d[2]


def edge_ends(k):
    """the two corner offsets (dx, dy, dz) of cube edge k, lower end first"""
    a, o1, o2 = k >> 2, k & 1, (k >> 1) & 1
    u, v = other_axes(a)
    lo = [0, 0, 0]
    lo[u], lo[v] = o1, o2
    hi = list(lo)
    hi[a] = 1
    return tuple(lo), tuple(hi)


EDGE_OF = {frozenset((corner_id(lo), corner_id(hi))): k for k in range(12) for lo, hi in [edge_ends(k)]}


# the (axis, side) faces of the cube an edge lies on: the axes along which both its ends have the same offset
EDGE_FACES = {k: frozenset((n, lo[n]) for n in range(3) if lo[n] == hi[n]) for k in range(12) for lo, hi in [edge_ends(k)]}


def face_cycles():
    """Per face the four corner ids in counter-clockwise order as seen from outside the cube."""
    out = []
    for n in range(3):
        for side in range(2):
            u, v = (n + 1) % 3, (n + 2) % 3  # e_u x e_v = e_n
            p, q = (u, v) if side else (v, u)  # (p, q, outward normal) right-handed
            cyc = []
            for cp, cq in ((0, 0), (1, 0), (1, 1), (0, 1)):
                d = [0, 0, 0]
                d[n], d[p], d[q] = side, cp, cq
                cyc.append(corner_id(d))
            out.append(cyc)
    return out


FACES = face_cycles()


def case_segments(case):
    """{from edge: to edge} over the six faces"""
    nxt = {}
    for cyc in FACES:
        ins = [(case >> c) & 1 for c in cyc]
        if sum(ins) in (0, 4):
            continue
        for i in range(4):
            if ins[i] and not ins[i - 1]:  # a run of inside corners starts at i: entered over the edge (i - 1, i)
                j = i
                while ins[(j + 1) % 4]:
                    j += 1
                enter = EDGE_OF[frozenset((cyc[i - 1], cyc[i]))]
                leave = EDGE_OF[frozenset((cyc[j % 4], cyc[(j + 1) % 4]))]
                assert enter not in nxt
                nxt[enter] = leave
    return nxt


def case_triangles(case):
    nxt = case_segments(case)
    crossing = sorted(k for k in range(12) if ((case >> corner_id(edge_ends(k)[0])) & 1) != ((case >> corner_id(edge_ends(k)[1])) & 1))
    assert sorted(nxt) == crossing and sorted(nxt.values()) == crossing, case
    tris, seen = [], set()
    for start in crossing:
        if start in seen:
            continue
        loop, k = [], start
        while k not in seen:
            seen.add(k)
            loop.append(k)
            k = nxt[k]
        assert k == start and len(loop) >= 3, case
        fans = [loop[r:] + loop[:r] for r in range(len(loop))]
        loop = next(fan for fan in fans if not any(EDGE_FACES[fan[0]] & EDGE_FACES[v] for v in fan[2:-1]))
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


def build_table():
    """-> (counts (256,) uint8, edges (256, 15) uint8, NONE where unused)"""
    counts = np.zeros(256, np.uint8)
    edges = np.full((256, 3 * MAX_TRIS), NONE, np.uint8)
    for case in range(256):
        tris = case_triangles(case)
        assert len(tris) <= MAX_TRIS
        counts[case] = len(tris)
        edges[case, : 3 * len(tris)] = np.asarray(tris, np.uint8).reshape(-1)
    return counts, edges


def render_header():
    counts, edges = build_table()
    lines = [
        "// gs_mc_table.hpp -- the marching-cubes case table.  GENERATED by tools/gen_mc_table.py: do not edit, run the generator.",
        "// Row `case` (bit c set iff corner c = dx + 2 dy + 4 dz has tsdf < 0): up to 5 triangles as 15 cube-edge numbers",
        "// k = 4 axis + o1 + 2 o2 (255: unused), then the number of triangles: 16 bytes, one 128-bit copy into LDS per case.",
        "#pragma once",
        "",
        "#ifndef GS_MC_TABLE_QUALIFIER",
        "#define GS_MC_TABLE_QUALIFIER static const",
        "#endif",
        "",
        "GS_MC_TABLE_QUALIFIER unsigned char GS_MC_CASES[256][16] __attribute__((aligned(16))) = {",
    ]
    for case in range(256):
        row = ", ".join("%3d" % x for x in list(edges[case]) + [counts[case]])
        lines.append("    {%s},  // %d" % (row, case))
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = render_header()
    if a.check:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("gs_mc_table.hpp", "is up to date" if same else "DIFFERS from the generator's output")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    counts, _ = build_table()
    print("wrote", HEADER, "triangles", int(counts.sum()), "by count", np.bincount(counts, minlength=6).tolist())
