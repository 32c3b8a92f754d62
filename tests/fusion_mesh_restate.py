"""The numpy float32 statement of csrc/fusion_mesh.hip and fusion.TSDFVolume.extract_mesh: the surface of a TSDF volume as a triangle
mesh.  The vertices are fusion_restate.extract's rows (marching cubes puts every triangle corner on a grid edge whose two voxels differ
in sign, and extract has one row per such edge); this file adds which three rows form each triangle, and a normal per row.  The case
table is not typed in from anywhere: it follows from the rule below, stated here independently of tools/gen_fusion_mesh_table.py and
of the header that script writes; tests/test_fusion_mesh_host.py compares the two case by case.  A plain module: it reads nothing
outside the repository.

    corners      corner c of the cell of voxels (i..i+1, j..j+1, k..k+1) is voxel (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))
    case         sum of (tsdf[c] < 0) << c: extract's "negative", so 0 counts as positive
    edges        e = 4 a + p: a the edge's axis, o0 < o1 the two other axes, p = (bit o0 of the start corner) + 2 (bit o1 of it); the
                 edge runs from its start corner to start | (1 << a), and its vertex is extract's row of the start corner's voxel, edge a
    segments     the four corners of each of the six faces walked counter-clockwise as seen from outside the cell: every maximal run of
                 negative corners gives one directed segment from the cell edge where the walk enters the run to the one where it
                 leaves (none on a face that is all negative or all positive; two on a face with two diagonal negative corners, each
                 cutting off one of them).  Only the face's four signs decide, so two cells that share a face agree: the mesh is closed
    loops        every crossed edge starts one segment and ends one: closed loops, taken in the order of their smallest edge id, each
                 from that edge along the segments' direction
    triangles    a loop e0, e1, ..., e(n-1) gives (e0, e_m, e_(m+1)) for m = 1 .. n - 2; their normals (right-hand rule) point from
                 negative to positive tsdf: out of the surface, towards the cameras

    case_triangles    one case's triangles by the rule
    case_table        the (256, 16) int8 array: a case's edge ids in order, padded with -1
    cell_cases        which cells of a volume take part, and their cases
    mesh              (vertices, normals, faces) of a fusion_restate.Volume
    noise_volume      seeded test volumes: uniform tsdf in (-1, 1), random colours, optionally a shell of +1 and unobserved voxels
    sphere_volume     the smooth test volume
"""
import numpy as np

import fusion_restate as fr

F = fr.F


def corner_voxel(c):
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


def edge_id(axis, start):
    o0, o1 = [o for o in range(3) if o != axis]
    return 4 * axis + ((start >> o0) & 1) + 2 * ((start >> o1) & 1)


def edge_start(e):
    """(axis, start corner) of edge e."""
    axis, p = e >> 2, e & 3
    o0, o1 = [o for o in range(3) if o != axis]
    return axis, ((p & 1) << o0) | ((p >> 1) << o1)


def _edge_between(c0, c1):
    axis = (c0 ^ c1).bit_length() - 1
    assert c0 ^ c1 == 1 << axis
    return edge_id(axis, min(c0, c1))


def face_walks():
    """The six faces' corners, counter-clockwise as seen from outside: around +a the other two axes in cyclic order (u x v = a)."""
    walks = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            ring = [(0, 0), (1, 0), (1, 1), (0, 1)]
            if side == 0:          # the outward normal is -a: the other way round
                ring = ring[::-1]
            walks.append([(side << a) | (p << u) | (q << v) for p, q in ring])
    return walks


def case_segments(case):
    """{edge where a segment starts: edge where it ends}."""
    follow = {}
    for walk in face_walks():
        neg = [(case >> c) & 1 for c in walk]
        if sum(neg) in (0, 4):
            continue
        for m in range(4):
            if neg[m] and not neg[m - 1]:          # the walk enters a run of negative corners
                n = m
                while neg[(n + 1) % 4]:
                    n += 1
                enter = _edge_between(walk[m - 1], walk[m])
                leave = _edge_between(walk[n % 4], walk[(n + 1) % 4])
                assert enter not in follow
                follow[enter] = leave
    assert sorted(follow) == sorted(follow.values())
    return follow


def case_loops(case):
    follow = case_segments(case)
    loops, seen = [], set()
    for e in sorted(follow):
        if e in seen:
            continue
        loop = [e]
        while follow[loop[-1]] != e:
            loop.append(follow[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def case_triangles(case):
    return [(loop[0], loop[m], loop[m + 1]) for loop in case_loops(case) for m in range(1, len(loop) - 1)]


_table = []


def case_table():
    if not _table:
        table = np.full((256, 16), -1, np.int8)
        for case in range(256):
            flat = [e for tri in case_triangles(case) for e in tri]
            table[case, :len(flat)] = flat
        _table.append(table)
    return _table[0]


def case_table_counts():
    """(256,) the cases' numbers of triangles."""
    return (case_table() >= 0).sum(axis=1) // 3


def _edges(volume, min_weight):
    """extract's own test: has[k, j, i, e], and the (k, j, i, e) of its rows in their order."""
    t, w = volume.tsdf, volume.weight
    ok = w >= F(min_weight)
    neg = t < 0
    has = np.zeros(t.shape + (3,), bool)
    has[:, :, :-1, 0] = ok[:, :, :-1] & ok[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    has[:, :-1, :, 1] = ok[:, :-1, :] & ok[:, 1:, :] & (neg[:, :-1, :] != neg[:, 1:, :])
    has[:-1, :, :, 2] = ok[:-1] & ok[1:] & (neg[:-1] != neg[1:])
    return ok, neg, has


def cell_cases(volume, min_weight=1.0):
    """(taking part (nz-1, ny-1, nx-1) bool, case (nz-1, ny-1, nx-1) int)."""
    ok, neg, _ = _edges(volume, min_weight)
    nz, ny, nx = ok.shape
    part = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        x, y, z = corner_voxel(c)
        sl = (slice(z, nz - 1 + z), slice(y, ny - 1 + y), slice(x, nx - 1 + x))
        part &= ok[sl]
        case |= neg[sl].astype(np.int64) << c
    return part, case


def mesh(volume, min_weight=1.0):
    """endo_fusion_mesh_count / _vertices / _faces: vertices (P, 6) float32 = fusion_restate.extract's rows; normals (P, 3) float32;
    faces (T, 3) int32 into the vertices: the cells whose eight corners all have weight >= min_weight, in (k, j, i) order, a cell's
    triangles in table order."""
    vertices = fr.extract(volume, min_weight)
    t = volume.tsdf
    nz, ny, nx = t.shape
    _, _, has = _edges(volume, min_weight)
    k, j, i, e = np.nonzero(has)
    assert k.shape[0] == vertices.shape[0]

    # normals: the central difference without its division, neighbours clamped to the grid and used whatever their weight
    normals = np.zeros((k.shape[0], 3), F)
    if k.shape[0]:
        def clamp(n):
            idx = np.arange(n)
            return np.minimum(idx + 1, n - 1), np.maximum(idx - 1, 0)
        (xp, xm), (yp, ym), (zp, zm) = clamp(nx), clamp(ny), clamp(nz)
        g = [t[:, :, xp] - t[:, :, xm], t[:, yp, :] - t[:, ym, :], t[zp] - t[zm]]
        kb, jb, ib = k + (e == 2), j + (e == 1), i + (e == 0)
        ta, tb = t[k, j, i], t[kb, jb, ib]
        with np.errstate(all="ignore"):
            lam = ta / (ta - tb)
            v = [g[a][k, j, i] + lam * (g[a][kb, jb, ib] - g[a][k, j, i]) for a in range(3)]
            length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            good = np.isfinite(length) & (length > 0)
            for a in range(3):
                normals[:, a] = np.where(good, v[a] / length, F(0))
        assert all(x.dtype == F for x in v) and length.dtype == F

    # faces
    index = np.full(has.shape, -1, np.int64)
    index[k, j, i, e] = np.arange(k.shape[0])
    part, case = cell_cases(volume, min_weight)
    table = case_table().astype(np.int64)
    count = case_table_counts()
    ck, cj, ci = np.nonzero(part)          # (k, j, i) order
    cc = case[ck, cj, ci]
    reps = count[cc]
    cell = np.repeat(np.arange(cc.shape[0]), reps)
    within = np.arange(cell.shape[0]) - np.repeat(np.cumsum(reps) - reps, reps)
    faces = np.zeros((cell.shape[0], 3), np.int32)
    starts = [edge_start(edge) for edge in range(12)]
    axis = np.array([a for a, _ in starts])
    off = np.array([corner_voxel(s) for _, s in starts])
    for corner in range(3):
        edge = table[cc[cell], 3 * within + corner]
        assert (edge >= 0).all()
        got = index[ck[cell] + off[edge, 2], cj[cell] + off[edge, 1], ci[cell] + off[edge, 0], axis[edge]]
        assert (got >= 0).all()          # a crossed edge of a cell that takes part is one of extract's rows
        faces[:, corner] = got
    return vertices, normals, faces


# ---- test volumes -------------------------------------------------------------------------------------------------------------------
def noise_volume(dims, seed, shell=False, holes=0.0, low_weight=0.0, positive=False):
    """Uniform tsdf in (-1, 1) and uniform colours in [0, 255); shell: the outer voxels +1; holes: that fraction of the voxels at weight
    0; low_weight: that fraction at weight 1, all others 2 (without either, all weights 1); positive: |tsdf|."""
    rng = np.random.default_rng(seed)
    volume = fr.Volume((-1.5, 0.25, 3.0), 0.5, dims)
    shape = volume.tsdf.shape
    t = rng.uniform(-1.0, 1.0, shape).astype(F)
    if positive:
        t = np.abs(t)
    if shell:
        t[0], t[-1], t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = (F(1),) * 6
    volume.tsdf = t
    volume.color = rng.uniform(0.0, 255.0, (3,) + shape).astype(F)
    pick = rng.uniform(0.0, 1.0, shape)
    weight = np.full(shape, 2.0 if low_weight else 1.0, F)
    weight[pick < holes + low_weight] = F(1)
    weight[pick < holes] = F(0)
    volume.weight = weight
    return volume


SPHERE_CENTRE, SPHERE_RADIUS = np.array([8.3, 7.1, 6.2]), 4.3


def sphere_volume():
    """tsdf = clip((dist - 4.3) / 4, -1, 1) around (8.3, 7.1, 6.2) in 16 x 14 x 12 unit voxels from the origin, all weights 1."""
    volume = fr.Volume((0.0, 0.0, 0.0), 1.0, (16, 14, 12))
    cx, cy, cz = (c.astype(np.float64) for c in volume.centres())
    dist = np.sqrt((cx[None, None, :] - SPHERE_CENTRE[0]) ** 2 + (cy[None, :, None] - SPHERE_CENTRE[1]) ** 2
                   + (cz[:, None, None] - SPHERE_CENTRE[2]) ** 2)
    volume.tsdf = np.clip((dist - SPHERE_RADIUS) / 4.0, -1.0, 1.0).astype(F)
    volume.weight = np.ones_like(volume.tsdf)
    volume.color = np.full((3,) + volume.tsdf.shape, 128.0, F)
    return volume
