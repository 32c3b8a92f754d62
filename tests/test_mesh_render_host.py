"""CPU-only checks of the triangle-mesh rasteriser: properties of tests/mesh_render_restate.py itself, the statement the device is held
to byte for byte in tests/test_gpu_mesh_render.py -- that a closed mesh has no cracks, how ties fall, how far fp32 leaves the depth from
the fp64 ray-plane intersection, what culling keeps, that degenerate and hostile data never hit -- and reader.read_mesh, the queries
and the argument validation of endo_mesh_render and mesh.TriangleMesh (every call here is refused before any device work)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mesh_render_restate as mr

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
mesh, reader, utils = ea.mesh, ea.reader, ea.utils
BADARG = -1
H, W = 37, 53
K = mr.intrinsics(30.0, H, W)
OUTPUTS = ("depth", "mask", "triangle", "barycentric", "normals")


def frames(k, n):
    return np.stack([k] * n)


def test_a_closed_mesh_has_no_cracks():
    """Six random poses inside the closed 320-face icosphere: every pixel is hit.  An exact condition: two triangles on an edge see
    the same sheared vertices and edge functions of equal magnitude and opposite sign, and zero is inclusive."""
    vertices, faces = mr.icosphere(2)
    assert faces.shape == (320, 3)
    rng = np.random.default_rng(0)
    rotations = np.stack([mr.random_rotation(rng) for _ in range(6)])
    translations = rng.uniform(-0.4, 0.4, (6, 3))
    out = mr.render(vertices, faces, frames(K, 6), rotations, translations, H, W)
    assert out["mask"].all() and (out["triangle"] >= 0).all()
    assert np.isfinite(out["depth"]).all() and out["depth"].min() > 0.3 and out["depth"].max() < 1.5
    lengths = np.linalg.norm(out["normals"].astype(np.float64), axis=-1)
    assert np.abs(lengths - 1.0).max() < 1e-6
    assert np.abs(out["barycentric"].astype(np.float64).sum(axis=-1) - 1.0).max() < 1e-5
    # seen from inside, every face is a back face: the normals are turned to the camera, and culling the back leaves nothing
    assert mr.render(vertices, faces, frames(K, 6), rotations, translations, H, W, cull=mr.CULL_BACK)["mask"].sum() == 0
    front = mr.render(vertices, faces, frames(K, 6), rotations, translations, H, W, cull=mr.CULL_FRONT)
    assert all(front[key].tobytes() == out[key].tobytes() for key in OUTPUTS)


def test_ties_go_to_the_lower_face():
    """A planar grid of quads at z = 2 with its vertices exactly on pixel-centre rays, camera at the origin: every pixel is hit, every
    depth is exactly 2.0, and where a ray meets an edge or a vertex the lowest of the faces that share it wins."""
    vertices, faces = mr.pixel_grid(K, H, W)
    out = mr.render(vertices, faces, K[None], np.eye(3)[None], np.zeros((1, 3)), H, W)
    assert out["mask"].all() and (out["depth"] == 2.0).all()
    shared = 0
    for face in range(faces.shape[0]):          # each face alone: the pixels it accepts
        alone = mr.render(vertices, faces[face:face + 1], K[None], np.eye(3)[None], np.zeros((1, 3)), H, W)["mask"][0, 0] > 0
        assert (out["triangle"][0][alone] <= face).all()
        shared += int((out["triangle"][0][alone] < face).sum())
    assert shared > 200          # the vertex rays alone are shared by up to six faces


def oblique_frames():
    poses = []
    for eye, target in (((0.0, 0.0, -3.0), (0.0, 0.0, 0.0)), ((2.0, 1.0, -2.5), (0.5, 0.0, 0.0)), ((-2.0, 1.0, -3.5), (0.0, -1.0, 0.0)),
                        ((1.0, -3.0, -4.5), (0.0, 0.0, 0.0)), ((0.3, 0.2, -11.0), (2.0, 1.0, 0.0))):
        poses.append((mr.look_at(eye, target), np.asarray(eye)))
    return np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses]), np.array([1.0, 0.37, 2.5, 14.0, 0.05], np.float32)


MEASURED_DEPTH_ERROR = 2.58e-5          # the largest relative error of test_depth_accuracy_on_a_plane's five frames, measured on the CPU


def test_depth_accuracy_on_a_plane():
    """One large quad in the plane z = 0 under five oblique poses and scales, against the fp64 intersection of each pixel's ray with
    the plane.  Measured here, on the CPU: the largest relative error of the restatement is MEASURED_DEPTH_ERROR = 2.572e-05 (frame 1; the
    others 7.9e-08, 6.9e-06, 7.9e-06, 1.2e-06).  That is not a few ulp: the quad's corners lie 500 units from rays that meet it 3 to
    11 units away, the edge functions are differences of products of the order 500^2, and what survives their cancellation carries
    2^-24 of that -- the price of one triangle this much larger than its distance; the frame that looks straight down the quad's
    centre, where the products pair off, keeps 8e-08.  The bound is four times the measurement, the margin for other libm and numpy
    builds."""
    vertices = np.array([[-500.0, -500.0, 0.0], [500.0, -500.0, 0.0], [500.0, 500.0, 0.0], [-500.0, 500.0, 0.0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    rotations, translations, scales = oblique_frames()
    k32 = mr.intrinsics(45.0, H, W)
    out = mr.render(vertices, faces, frames(k32, 5), rotations, translations, H, W, scales=scales)
    assert out["mask"].all()
    k = k32.astype(np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    worst = 0.0
    for f in range(5):
        ray = np.stack([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], np.ones_like(u)], axis=-1) @ rotations[f].T
        truth = -translations[f][2] / ray[..., 2] / float(scales[f])
        error = np.abs(out["depth"][f, 0].astype(np.float64) - truth) / truth
        print("frame %d: largest relative depth error %.3e" % (f, error.max()))
        worst = max(worst, float(error.max()))
    print("largest relative depth error %.3e" % worst)
    assert worst <= 4.0 * MEASURED_DEPTH_ERROR


def test_culling_by_the_sign_of_det():
    """The outward-oriented sphere from outside: culling the back changes no byte (the front is what is seen), culling the front
    shows the far side."""
    vertices, faces = mr.icosphere(2)
    rotation, translation = mr.look_at((0.5, 0.3, -3.0), (0.0, 0.0, 0.0))[None], np.array([[0.5, 0.3, -3.0]])
    plain = mr.render(vertices, faces, K[None], rotation, translation, H, W)
    back = mr.render(vertices, faces, K[None], rotation, translation, H, W, cull=mr.CULL_BACK)
    front = mr.render(vertices, faces, K[None], rotation, translation, H, W, cull=mr.CULL_FRONT)
    assert all(plain[key].tobytes() == back[key].tobytes() for key in OUTPUTS)
    hit = plain["mask"] > 0
    assert 300 < hit.sum() < H * W and (front["mask"] > 0)[hit].all()
    assert (front["depth"][hit] > plain["depth"][hit]).all()
    centre = (0, 0, H // 2, W // 2)
    assert abs(plain["depth"][centre] - 2.06) < 0.1 and abs(front["depth"][centre] - 4.06) < 0.1
    # the front's normal points at the camera: against the viewing direction
    toward = rotation[0][:, 2]
    assert plain["normals"][0, H // 2, W // 2] @ toward < -0.9 and front["normals"][0, H // 2, W // 2] @ toward < -0.9


def test_degenerate_and_hostile_data_never_hit():
    """Triangles with a repeated vertex (U, V, W are f(P, P) = 0 and a pair f(P, Q), f(Q, P): one sign only when all are 0, and then
    det = 0), faces with an index of -1 or V, a triangle wholly behind the camera and a NaN scale: nothing is hit, nothing raises.
    One honest triangle among them is seen as it is alone."""
    honest = np.array([[-1.0, -1.0, 3.0], [1.0, -1.0, 3.0], [0.0, 1.0, 3.0]], np.float32)
    extra = np.array([[0.2, 0.1, 2.0], [-0.3, 0.2, 2.5], [0.0, 0.0, -2.0], [1.0, 0.0, -3.0], [0.0, 1.0, -2.5], [np.nan, 0.0, 2.0]], np.float32)
    vertices = np.concatenate([honest, extra])
    count = vertices.shape[0]
    faces = np.array([[3, 3, 3], [3, 3, 4], [3, 4, 3], [4, 3, 3], [0, 1, -1], [0, count, 2], [-5, 1, 2], [5, 6, 7], [8, 3, 4], [0, 1, 2]], np.int32)
    rotations, translations = np.stack([np.eye(3)] * 2), np.zeros((2, 3))
    out = mr.render(vertices, faces, frames(K, 2), rotations, translations, H, W, scales=np.array([1.0, np.nan], np.float32))
    alone = mr.render(honest, faces[-1:], K[None], rotations[:1], translations[:1], H, W)
    assert set(np.unique(out["triangle"][0])) == {-1, 9} and (out["triangle"][0] == 9).sum() > 100
    assert out["depth"][0].tobytes() == alone["depth"][0].tobytes() and out["mask"][0].tobytes() == alone["mask"][0].tobytes()
    assert out["flags"].tolist() == [mr.FRAME_OK, mr.FRAME_BAD_SCALE]
    assert not out["mask"][1].any() and not out["depth"][1].any() and (out["triangle"][1] == -1).all() and not out["normals"][1].any()
    assert mr.render(vertices, faces[:-1], frames(K, 2), rotations, translations, H, W)["mask"].sum() == 0
    empty = mr.render(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), K[None], rotations[:1], translations[:1], H, W)
    assert empty["mask"].sum() == 0 and empty["colors"] is None


def test_colours_are_mixed_by_the_barycentric_weights():
    vertices = np.array([[-2.0, -2.0, 3.0, 255.0, 0.0, 10.0], [2.0, -2.0, 3.0, 0.0, 255.0, 20.0], [0.0, 2.5, 3.0, 0.0, 0.0, 30.0]], np.float32)
    out = mr.render(vertices, np.array([[0, 1, 2]], np.int32), K[None], np.eye(3)[None], np.zeros((1, 3)), H, W)
    hit = out["mask"][0, 0] > 0
    beta = out["barycentric"][0][hit].astype(np.float64)
    want = beta @ vertices[:, [5, 4, 3]].astype(np.float64)          # byte c is column 5 - c: b, g, r = planes 0, 1, 2
    assert hit.sum() > 500 and np.abs(out["colors"][0][hit].astype(np.float64) - want).max() <= 0.5 + 1e-3
    assert not out["colors"][0][~hit].any()


def test_read_mesh_reads_what_write_mesh_writes(tmp_path):
    rng = np.random.default_rng(1)
    vertices = np.concatenate([rng.normal(size=(40, 3)), rng.integers(0, 256, (40, 3))], axis=1).astype(np.float32)
    normals = rng.normal(size=(40, 3)).astype(np.float32)
    faces = rng.integers(0, 40, (70, 3)).astype(np.int32)
    for text in (False, True):
        path = tmp_path / ("mesh_%d.ply" % text)
        utils.write_mesh(path, vertices, normals, faces, text=text)
        got_vertices, got_faces = reader.read_mesh(path)
        assert got_vertices.dtype == np.float32 and got_faces.dtype == np.int32
        assert got_vertices.tobytes() == vertices.tobytes() and got_faces.tobytes() == faces.tobytes()
        utils.write_mesh(path, vertices[:0], normals[:0], faces[:0], text=text)
        got_vertices, got_faces = reader.read_mesh(path)
        assert got_vertices.shape == (0, 6) and got_faces.shape == (0, 3)
    assert len(reader.read_point_cloud(path)) == 0          # the vertex reader is what it was


def test_read_mesh_takes_polygons_any_property_order_and_no_faces(tmp_path):
    path = tmp_path / "quad.ply"
    path.write_text("\n".join([
        "ply", "format ascii 1.0", "comment by hand", "element vertex 5", "property float nz", "property double y", "property float x",
        "property float nx", "property float z", "property float ny", "element face 4", "property uchar flag",
        "property list uchar uint vertex_indices", "end_header",
        "0 1.5 0.25 0 -3 1", "0 2.5 1.25 0 -4 1", "1 3.5 2.25 0 -5 0", "1 4.5 3.25 0 -6 0", "1 5.5 4.25 0 -7 0",
        "7 4 0 1 2 3", "9 2 0 1", "1 3 4 3 2", "0 5 0 1 2 3 4"]) + "\n")
    vertices, faces = reader.read_mesh(path)
    assert vertices.tolist() == [[0.25, 1.5, -3.0], [1.25, 2.5, -4.0], [2.25, 3.5, -5.0], [3.25, 4.5, -6.0], [4.25, 5.5, -7.0]]
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [4, 3, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    cloud = tmp_path / "cloud.ply"
    utils.write_point_cloud(cloud, np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]], np.float32), text=False)
    vertices, faces = reader.read_mesh(cloud)
    assert vertices.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]] and faces.shape == (0, 3) and faces.dtype == np.int32
    with pytest.raises(ValueError, match="not a PLY file"):
        bad = tmp_path / "bad.ply"
        bad.write_text("plain text\n")
        reader.read_mesh(bad)


def test_queries():
    lib = ea._lib.load()
    assert [lib.endo_mesh_render_tile(which) for which in range(5)] == [8, 8, 16, 256, BADARG] and lib.endo_mesh_render_tile(-1) == BADARG
    assert mesh.RENDER_TILE == (8, 8, 16, 256)
    assert (mesh.CULL_BACK, mesh.CULL_FRONT, mesh.BRUTE) == (mr.CULL_BACK, mr.CULL_FRONT, mr.BRUTE) == (1, 2, 4)

    def up(v):
        return (v + 255) // 256 * 256

    for n, h, w, t in ((1, 1, 1, 0), (8, 37, 53, 320), (3, 17, 25, 1), (8, 256, 320, 1000000)):
        assert lib.endo_mesh_render_workspace_bytes(n, h, w, t) == up(n * h * w * 8) + 256 + up(n * t * 8), (n, h, w, t)
    for bad in ((0, 16, 24, 5), (1, 0, 24, 5), (1, 16, -1, 5), (65536, 16, 24, 5), (8, 1 << 15, 1 << 15, 5), (1, 16, 24, -1), (1, 16, 24, 1 << 31)):
        assert lib.endo_mesh_render_workspace_bytes(*bad) == -1, bad


def test_endo_mesh_render_refuses_bad_arguments_before_any_device_work():
    """No call here is valid, so none launches: the pointers are host addresses that are never followed."""
    lib = ea._lib.load()
    block = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(block) + 255) // 256 * 256

    def p(offset=0):
        return ctypes.c_void_p(base + offset)

    need = lib.endo_mesh_render_workspace_bytes(2, 16, 24, 10)
    good = dict(vertices=p(), vertex_stride=6, vertex_count=12, faces=p(), triangles=10, intrinsics=p(), rotations=p(), translations=p(),
                scales=None, boundaries=None, frames=2, height=16, width=24, options=0, depth=p(), mask=None, triangle=None,
                barycentric=None, normals=None, colors=None, flags=None, workspace=p(), workspace_bytes=need, stream=None)
    bad = [dict(vertices=None), dict(faces=None), dict(intrinsics=None), dict(rotations=None), dict(translations=None), dict(depth=None),
           dict(workspace=None), dict(vertices=p(2)), dict(faces=p(1)), dict(intrinsics=p(3)), dict(rotations=p(4)), dict(translations=p(4)),
           dict(scales=p(2)), dict(boundaries=p(1)), dict(depth=p(2)), dict(mask=p(2)), dict(triangle=p(3)), dict(barycentric=p(1)),
           dict(normals=p(2)), dict(flags=p(2)), dict(workspace=p(4)), dict(vertex_stride=2), dict(vertex_stride=3, colors=p()),
           dict(vertex_stride=5, colors=p()), dict(vertex_count=-1), dict(vertex_count=1 << 31), dict(triangles=-1), dict(triangles=1 << 31),
           dict(frames=0), dict(height=0), dict(width=-3), dict(frames=65536), dict(options=3), dict(options=8), dict(options=-1),
           dict(workspace_bytes=need - 1), dict(workspace_bytes=0)]
    for change in bad:
        args = dict(good, **change)
        assert lib.endo_mesh_render(*args.values()) == BADARG, change
    assert list(good) == ["vertices", "vertex_stride", "vertex_count", "faces", "triangles", "intrinsics", "rotations", "translations",
                          "scales", "boundaries", "frames", "height", "width", "options", "depth", "mask", "triangle", "barycentric",
                          "normals", "colors", "flags", "workspace", "workspace_bytes", "stream"]
    assert len(ea._lib.SIGNATURES["endo_mesh_render"][1]) == len(good)
    with pytest.raises(TypeError):
        lib.endo_mesh_render(*list(good.values())[:-1])


def test_triangle_mesh_checks_its_arguments():
    with pytest.raises(RuntimeError, match="vertices must live on the GPU: the MI355X path has no CPU fallback"):
        mesh.TriangleMesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="vertices must be"):
        mesh.TriangleMesh(torch.zeros(4, 4), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="vertices must be"):
        mesh.TriangleMesh(np.zeros(12, np.float32), np.zeros((2, 3), np.int32))
    shell = mesh.TriangleMesh.__new__(mesh.TriangleMesh)          # (no device here: the checks below come before any device work)
    shell.vertices, shell.faces = torch.zeros(4, 6), torch.zeros((2, 3), dtype=torch.int32)
    shell.device, shell.has_colors = torch.device("cuda:0"), True
    k = torch.from_numpy(frames(K, 2))
    pose = (np.stack([np.eye(3)] * 2), np.zeros((2, 3)))
    with pytest.raises(RuntimeError, match="intrinsics must live on the GPU: the MI355X path has no CPU fallback"):
        shell.render(k, *pose, H, W)
    with pytest.raises(ValueError, match="intrinsics must be an"):
        shell.render(k[0], *pose, H, W)
    with pytest.raises(ValueError, match="cull is None, 'back' or 'front'"):
        shell.render(k, *pose, H, W, cull="both")
    with pytest.raises(ValueError, match="mesh must be a mesh.TriangleMesh"):
        ea.evaluate.model_depth_errors(torch.zeros(2, 1, H, W), torch.zeros(2, 1, H, W), k, *pose, object())
