"""CPU-only checks of the fused surface as a triangle mesh: the case table compiled into the library (read through
endo_fusion_mesh_case) against the rule as tests/fusion_mesh_restate.py states it, the generator's output against the committed
header, and the restatement itself -- the numpy statement the device's vertices, normals and faces are compared with byte for byte --
held to what a mesh must be: closed and consistently oriented wherever every cell takes part, a sphere's volume, area and normals,
no face from a cell with an unobserved corner; and utils.write_mesh's round trips."""
import ctypes
import hashlib
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest

import fusion_mesh_restate as mr
import fusion_restate as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

ENTRIES = ("endo_fusion_mesh_case", "endo_fusion_mesh_workspace_bytes", "endo_fusion_mesh_count", "endo_fusion_mesh_vertices",
           "endo_fusion_mesh_faces")
TABLE_SHA256 = "27817b34b28060477a68a54130f5d8a23dd75e83cdad006a01bfaf8ceaffc61a"          # of the (256, 16) int8 array: a sanity check


def read_mesh_ply(path):
    """What utils.write_mesh wrote: (vertices (P, 6) float32 of x, y, z, r, g, b, normals (P, 3) float32, faces (T, 3) int32)."""
    with open(str(path), "rb") as f:
        data = f.read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] in ("format ascii 1.0", "format binary_little_endian 1.0")
    assert lines[2].startswith("element vertex ") and lines[12].startswith("element face ") and lines[14] == ""
    assert tuple(lines[3:12]) == ("property float x", "property float y", "property float z", "property float nx", "property float ny",
                                  "property float nz", "property uchar red", "property uchar green", "property uchar blue")
    assert lines[13] == "property list uchar int vertex_indices"
    n, t = int(lines[2].split()[2]), int(lines[12].split()[2])
    if lines[1] == "format ascii 1.0":
        rows = [line.split() for line in body.decode("ascii").split("\n")[:-1]] if body else []
        assert len(rows) == n + t and all(len(r) == 9 for r in rows[:n]) and all(len(r) == 4 and r[0] == "3" for r in rows[n:])
        vertex = np.array(rows[:n], np.float64).astype(np.float32).reshape(n, 9)
        faces = np.array([r[1:] for r in rows[n:]], np.int64).astype(np.int32).reshape(t, 3)
        return np.concatenate([vertex[:, :3], vertex[:, 6:]], axis=1), vertex[:, 3:6], faces
    vdt = np.dtype([("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("rgb", "u1", (3,))])
    fdt = np.dtype([("count", "u1"), ("index", "<i4", (3,))])
    assert len(body) == n * vdt.itemsize + t * fdt.itemsize
    vertex = np.frombuffer(body, vdt, n)
    tri = np.frombuffer(body, fdt, t, offset=n * vdt.itemsize)
    assert (tri["count"] == 3).all()
    return np.concatenate([vertex["xyz"], vertex["rgb"].astype(np.float32)], axis=1), vertex["n"].copy(), tri["index"].copy()


def directed_edge_counts(faces, points):
    """{a * points + b: the number of triangles that use a -> b}, as two sorted arrays."""
    a = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]]).astype(np.int64)
    b = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]]).astype(np.int64)
    return np.unique(a * points + b, return_counts=True), np.unique(b * points + a, return_counts=True)


def library_case(lib, case):
    edges = (ctypes.c_int32 * 15)()
    count = lib.endo_fusion_mesh_case(case, edges)
    return count, list(edges)


def test_entries_are_declared_exported_and_built_with_the_flag():
    import __graft_entry__ as entry
    assert "fusion_mesh.hip" in entry.SOURCES and entry.EXTRA_FLAGS["fusion_mesh.hip"] == ["-ffp-contract=off"]
    if not os.path.exists(ea._lib.LIB_PATH):
        entry.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "endo_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(ea._lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared" % name
        assert hasattr(raw, name), "libendo_hip.so does not export %s" % name
        assert name in ea._lib.SIGNATURES
    lib = ea._lib.load()
    # argument validation happens before any device work
    assert lib.endo_fusion_mesh_workspace_bytes(40, 24, 20) >= 2 * 24 * 20 * 8
    assert lib.endo_fusion_mesh_workspace_bytes(42, 24, 20) == -1 and lib.endo_fusion_mesh_workspace_bytes(40, 0, 20) == -1
    assert lib.endo_fusion_mesh_workspace_bytes(40, 70000, 20) == -1 and lib.endo_fusion_mesh_workspace_bytes(2 ** 30, 2 ** 10, 2 ** 10) == -1
    assert lib.endo_fusion_mesh_workspace_bytes(512, 512, 512) == 2 * 512 * 512 * 8          # O(nz ny), whatever nx
    assert lib.endo_fusion_mesh_count(None, 0.5, 40, 24, 20, None, None, None, 1.0, None, None, 0, None) == -1
    assert lib.endo_fusion_mesh_vertices(None, 0.5, 40, 24, 20, None, None, None, 1.0, None, None, 0, None, None, 0, None) == -1
    assert lib.endo_fusion_mesh_faces(None, 0.5, 40, 24, 20, None, None, None, 1.0, None, 0, None, None, 0, None) == -1
    assert hasattr(ea.fusion.TSDFVolume, "extract_mesh") and hasattr(ea.utils, "write_mesh")


def test_the_compiled_table_is_the_rule():
    lib = ea._lib.load()
    assert lib.endo_fusion_mesh_case(-1, None) == -1 and lib.endo_fusion_mesh_case(256, None) == -1
    counts = []
    table = np.full((256, 16), -1, np.int8)
    for case in range(256):
        count, edges = library_case(lib, case)
        want = mr.case_triangles(case)
        flat = [e for tri in want for e in tri]
        assert count == len(want) == lib.endo_fusion_mesh_case(case, None), "case 0x%02x" % case
        assert edges == flat + [-1] * (15 - len(flat)), "case 0x%02x" % case
        # every triangle's corners are three different crossed edges of the cell
        for tri in want:
            assert len(set(tri)) == 3
            for e in tri:
                axis, start = mr.edge_start(e)
                assert ((case >> start) & 1) != ((case >> (start | (1 << axis))) & 1)
        counts.append(count)
        table[case, :15] = edges
    assert sum(counts) == 820 and max(counts) == 5
    assert np.bincount(counts).tolist() == [2, 16, 50, 80, 76, 32]
    assert np.array_equal(table, mr.case_table())
    assert [mr.case_triangles(c) for c in (0x01, 0x03, 0xfe)] == [[(0, 4, 8)], [(4, 8, 9), (4, 9, 5)], [(0, 8, 4)]]
    assert mr.case_triangles(0x69) == [(0, 4, 8), (1, 5, 11), (2, 7, 9), (3, 6, 10)]
    assert hashlib.sha256(table.tobytes()).hexdigest() == TABLE_SHA256


def test_the_generator_writes_the_committed_header():
    spec = importlib.util.spec_from_file_location("gen_fusion_mesh_table", os.path.join(ROOT, "tools", "gen_fusion_mesh_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ROOT, "endoscopydepthestimation-pytorch_amd", "csrc", "fusion_mesh_table.h")) as f:
        assert f.read() == gen.header_text()


def ambiguous(case):
    """A face of the cell has two diagonal negative corners."""
    return any([(case >> c) & 1 for c in walk] in ([1, 0, 1, 0], [0, 1, 0, 1]) for walk in mr.face_walks())


def test_a_case_and_its_complement():
    """The complement crosses the same edges.  Where no face is ambiguous the complement's surface is the same one seen from the other
    side: the same number of triangles, every loop reversed.  A face with two diagonal negative corners is cut so that each negative
    corner is cut off, and its complement cuts off the other two: the 120 such cases pair with another surface through the same
    edges (88 of them with another number of triangles), which is what keeps neighbouring cells consistent."""
    plain = 0
    for case in range(256):
        other = 255 - case
        loops, other_loops = mr.case_loops(case), mr.case_loops(other)
        assert sorted(e for loop in loops for e in loop) == sorted(e for loop in other_loops for e in loop)
        if ambiguous(case):
            continue
        plain += 1
        assert len(mr.case_triangles(case)) == len(mr.case_triangles(other))
        assert sorted([loop[0]] + loop[:0:-1] for loop in loops) == sorted(other_loops), "case 0x%02x" % case
    assert plain == 136


@pytest.mark.parametrize("dims, seed, every_case", [((12, 10, 9), 0, False), ((20, 14, 12), 0, True)])
def test_every_case_closes(dims, seed, every_case):
    """Noise inside a shell of +1, all weights 1: every cell takes part and no surface reaches the grid's border, so the mesh is
    closed and consistently oriented: as many triangles use a -> b as use b -> a (noise can put four triangles on one edge, so not
    exactly one each).  The 792 cells of 12 x 10 x 9 hold about 210 of the 256 cases whatever the seed (229 at most over 200 seeds:
    the 378 cells away from the shell are 1.5 per case); 20 x 14 x 12 holds them all, asserted on the input."""
    volume = mr.noise_volume(dims, seed, shell=True)
    part, case = mr.cell_cases(volume)
    assert part.all()
    found = np.unique(case).shape[0]
    print("%s: %d cells, %d cases" % (dims, case.size, found))
    assert found == 256 if every_case else found >= 200
    vertices, normals, faces = mr.mesh(volume)
    assert vertices.tobytes() == fr.extract(volume).tobytes()
    assert faces.dtype == np.int32 and faces.shape[0] == mr.case_table_counts()[case].sum()
    forward, backward = directed_edge_counts(faces, vertices.shape[0])
    assert np.array_equal(forward[0], backward[0]) and np.array_equal(forward[1], backward[1])
    assert np.unique(faces).shape[0] == vertices.shape[0]          # every row is referenced
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()


def test_a_sphere():
    volume = mr.sphere_volume()
    vertices, normals, faces = mr.mesh(volume)
    points = vertices.shape[0]
    forward, backward = directed_edge_counts(faces, points)
    assert (forward[1] == 1).all() and np.array_equal(forward[0], backward[0])          # every edge in two triangles, once each way
    edges = forward[0].shape[0] // 2
    assert np.unique(faces).shape[0] == points and points - edges + faces.shape[0] == 2
    p = vertices[:, :3].astype(np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    volume_in = float((a * np.cross(b, c)).sum() / 6.0)
    cross = np.cross(b - a, c - a)
    area = np.linalg.norm(cross, axis=1) / 2.0
    exact_volume, exact_area = 4.0 / 3.0 * np.pi * mr.SPHERE_RADIUS ** 3, 4.0 * np.pi * mr.SPHERE_RADIUS ** 2
    n = normals.astype(np.float64)
    big = area > 1e-6
    facing = ((cross[big] / (2.0 * area[big, None])) * n[faces[big, 0]]).sum(axis=1)
    radial = p - mr.SPHERE_CENTRE
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    along = (n * radial).sum(axis=1)
    print("sphere: %d vertices, %d faces, volume %.1f (%.1f), area %.1f (%.2f), face . vertex normal >= %.3f, normal . radial >= %.5f" % (
        points, faces.shape[0], volume_in, exact_volume, area.sum(), exact_area, facing.min(), along.min()))
    assert abs(exact_volume - 333.0) < 0.1 and abs(exact_area - 232.35) < 0.01
    assert volume_in > 0 and abs(volume_in - 333.0) <= 0.05 * 333.0
    assert abs(area.sum() - 232.35) <= 0.03 * 232.35
    assert facing.min() > 0.9 and along.min() > 0.99
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6


def test_holes():
    volume = mr.noise_volume((12, 10, 9), 0, shell=True, holes=0.15)
    vertices, normals, faces = mr.mesh(volume)
    assert vertices.tobytes() == fr.extract(volume).tobytes() and normals.shape == (vertices.shape[0], 3)
    points = vertices.shape[0]
    assert faces.shape[0] > 100 and faces.min() >= 0 and faces.max() < points
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    assert np.unique(faces).shape[0] < points          # rows on the rim of a hole
    # no face from a cell with an unobserved corner: every triangle's corners lie on the edges of one cell whose voxels all count
    p = vertices[:, :3].astype(np.float64)
    grid = (p - volume.origin.astype(np.float64)) / float(volume.vs) - 0.5          # in voxels: two whole coordinates, one inside an edge
    ok = volume.weight >= 1.0
    low = np.floor(np.minimum(np.minimum(grid[faces[:, 0]], grid[faces[:, 1]]), grid[faces[:, 2]]) + 1e-4).astype(int)
    high = np.ceil(np.maximum(np.maximum(grid[faces[:, 0]], grid[faces[:, 1]]), grid[faces[:, 2]]) - 1e-4).astype(int)
    assert ((high - low) <= 1).all()
    flat = high == low          # a triangle inside a face of its cell: the cell on either side
    cells = np.array([volume.nx, volume.ny, volume.nz]) - 1
    found = np.zeros(faces.shape[0], bool)
    for side in np.ndindex(2, 2, 2):
        cell = low - np.array(side) * flat
        inside = ((cell >= 0) & (cell < cells)).all(axis=1)
        cell = np.clip(cell, 0, cells - 1)
        whole = inside.copy()
        for dx, dy, dz in np.ndindex(2, 2, 2):
            whole &= ok[cell[:, 2] + dz, cell[:, 1] + dy, cell[:, 0] + dx]
        found |= whole
    assert found.all()
    part, case = mr.cell_cases(volume)
    assert not part.all() and faces.shape[0] == mr.case_table_counts()[case[part]].sum()


@pytest.mark.parametrize("text", [False, True])
def test_write_mesh_round_trips(tmp_path, text):
    volume = mr.noise_volume((12, 10, 9), 3, shell=True, holes=0.15)
    vertices, normals, faces = mr.mesh(volume)
    path = tmp_path / "mesh.ply"
    ea.utils.write_mesh(path, vertices, normals, faces, text=text)
    got = read_mesh_ply(path)
    for a, b in zip(got, (vertices, normals, faces)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    # no faces, and nothing at all
    ea.utils.write_mesh(path, vertices, normals, faces[:0], text=text)
    got = read_mesh_ply(path)
    assert got[0].tobytes() == vertices.tobytes() and got[1].tobytes() == normals.tobytes() and got[2].shape == (0, 3)
    ea.utils.write_mesh(path, vertices[:0], normals[:0], faces[:0], text=text)
    got = read_mesh_ply(path)
    assert got[0].shape == (0, 6) and got[1].shape == (0, 3) and got[2].shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        ea.utils.write_mesh(path, vertices[:5], normals[:5], faces, text=text)
    with pytest.raises(ValueError, match="one normal per vertex"):
        ea.utils.write_mesh(path, vertices, normals[:5], faces, text=text)
