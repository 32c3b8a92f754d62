#!/usr/bin/env python3
"""Writes endoscopydepthestimation-pytorch_amd/csrc/fusion_mesh_table.h: the marching-cubes case table of csrc/fusion_mesh.hip, built
by rule, not copied from anywhere.  Running it again gives the same bytes (tests/test_fusion_mesh_host.py checks that, and compares the
compiled table case by case with tests/fusion_mesh_restate.py, which states the same rule in its own code).

    python tools/gen_fusion_mesh_table.py [output path]

The rule.  Corner c of a cell is voxel (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)); bit c of the case index is tsdf[c] < 0.
Edge e = 4 a + p runs along axis a from its start corner, p = (bit o0 of the start corner) + 2 (bit o1), o0 < o1 the other two axes.
On each of the six faces, seen from outside the cell, the boundary between negative and positive corners is cut into directed segments
that keep the negative corners on their left: from the cell edge where a counter-clockwise walk of the face's corners enters a run of
negative corners to the one where it leaves the run.  Two diagonal negative corners are two runs: each is cut off on its own.  Only the
face's own four signs decide, so neighbouring cells agree and the mesh is closed.  The segments chain into loops; loops in the order of
their smallest edge id, each started there, are fanned into triangles (e0, e_m, e_(m+1)).  Normals point from negative to positive.
"""
import math
import os
import sys

AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def corner_position(c):
    return (float(c & 1), float((c >> 1) & 1), float((c >> 2) & 1))


def edge_of(c0, c1):
    """The id of the cell edge between two adjacent corners."""
    (axis,) = [a for a in range(3) if (c0 ^ c1) == 1 << a]
    start = min(c0, c1)
    others = [a for a in range(3) if a != axis]
    return 4 * axis + ((start >> others[0]) & 1) + 2 * ((start >> others[1]) & 1)


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def face_rings():
    """Per face, its four corners in counter-clockwise order as seen from outside: sorted by their angle around the outward normal."""
    rings = []
    for axis in range(3):
        for side in (0, 1):
            normal = tuple((2 * side - 1) * x for x in AXES[axis])
            u = AXES[(axis + 1) % 3]
            v = cross(normal, u)          # u x v = normal
            corners = [c for c in range(8) if ((c >> axis) & 1) == side]

            def angle(c):
                p = [x - 0.5 for x in corner_position(c)]
                return math.atan2(sum(a * b for a, b in zip(p, v)), sum(a * b for a, b in zip(p, u)))
            rings.append(sorted(corners, key=angle))
    return rings


def triangles(case, rings):
    nxt = {}
    for ring in rings:
        negative = [bool((case >> c) & 1) for c in ring]
        for at in range(4):
            before, here = ring[at - 1], ring[at]
            if negative[at] and not negative[at - 1]:          # a run of negative corners starts here
                end = at
                while negative[(end + 1) % 4]:
                    end += 1
                nxt[edge_of(before, here)] = edge_of(ring[end % 4], ring[(end + 1) % 4])
    out = []
    left = set(nxt)
    while left:
        first = min(left)
        loop = [first]
        left.discard(first)
        while nxt[loop[-1]] != first:
            loop.append(nxt[loop[-1]])
            left.discard(loop[-1])
        out.extend((loop[0], loop[m], loop[m + 1]) for m in range(1, len(loop) - 1))
    return out


def header_text():
    rings = face_rings()
    rows, counts = [], []
    for case in range(256):
        tris = triangles(case, rings)
        flat = [e for tri in tris for e in tri]
        assert len(flat) <= 15
        counts.append(len(tris))
        rows.append(flat + [-1] * (16 - len(flat)))
    lines = [
        "// Written by tools/gen_fusion_mesh_table.py (which states the rule): do not edit.  The marching-cubes case table of",
        "// fusion_mesh.hip: per case (bit c: corner c's tsdf < 0) the cell-edge ids of its triangles, three per triangle, padded with -1,",
        "// and the number of triangles.  %d triangles in all, at most %d per case." % (sum(counts), max(counts)),
        "#pragma once",
        "",
        "namespace endo {",
        "",
        "struct MeshCaseTable {",
        "    alignas(16) signed char edges[256][16];          // (a case is one 16-byte load)",
        "    unsigned char triangles[256];",
        "};",
        "",
        "constexpr MeshCaseTable kMeshCases = {",
        "    {",
    ]
    for case, row in enumerate(rows):
        lines.append("        {%s},  // 0x%02x" % (", ".join("%2d" % e for e in row), case))
    lines.append("    },")
    lines.append("    {")
    for at in range(0, 256, 32):
        lines.append("        %s," % ", ".join(str(n) for n in counts[at:at + 32]))
    lines += ["    },", "};", "", "}  // namespace endo", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    default = os.path.join(os.path.dirname(here), "endoscopydepthestimation-pytorch_amd", "csrc", "fusion_mesh_table.h")
    path = sys.argv[1] if len(sys.argv) > 1 else default
    with open(path, "w") as f:
        f.write(header_text())
    print("wrote", path)
