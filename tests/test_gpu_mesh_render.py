"""mesh.TriangleMesh.render / endo_mesh_render on the device against tests/mesh_render_restate.py, byte for byte, for every output, with
the pixel box and with every pixel against every triangle (brute=True).  Run with ``pytest -m gpu`` on an MI355X."""
import importlib

import numpy as np
import pytest
import torch

import mesh_render_restate as mr
from test_gpu_fusion_render import cameras, centre_of, integrated, on_device

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
mesh = ea.mesh
OUTPUTS = ("depth", "mask", "triangle", "barycentric", "normals", "colors", "flags")
SCALES = np.array([0.7, np.nan, 2.0], np.float32)          # three frames; the middle one renders nothing
FOCAL = 30.0


def over_tile():
    tx, ty = mesh.RENDER_TILE[:2]
    return 2 * ty + 1, 3 * tx + 1


def shapes():
    return [(37, 53), over_tile()]


def look(eyes, targets):
    return np.stack([mr.look_at(e, t) for e, t in zip(eyes, targets)]), np.asarray(eyes, np.float64)


def case(name, h, w):
    """(vertices, faces, intrinsics (3, 3, 3), rotations, translations) of a named case."""
    k = np.stack([mr.intrinsics(FOCAL * w / 53.0, h, w)] * 3)
    if name == "sphere inside":
        rng = np.random.default_rng(2)
        return mr.icosphere(2) + (k, np.stack([mr.random_rotation(rng) for _ in range(3)]), rng.uniform(-0.4, 0.4, (3, 3)))
    if name == "sphere outside":
        return mr.icosphere(2) + (k,) + look([(0.5, 0.3, -3.0), (2.0, -1.0, 1.5), (0.0, 2.2, 0.1)], [(0.0, 0.0, 0.0)] * 3)
    if name == "tube":          # inside: ring 0 crosses the second camera's plane, rings behind the others lie behind them
        return mr.tube() + (k,) + look([(0.0, 0.0, 1.0), (0.3, -0.2, 0.25), (0.0, 0.1, 2.0)], [(0.2, 0.0, 4.0), (0.0, 0.3, 3.0), (0.6, 0.0, 4.0)])
    if name == "pixel grid":          # the first frame sees the vertices on its pixel centres; the others see the grid askew
        vertices, faces = mr.pixel_grid(k[0], h, w)
        return (vertices, faces, k) + look([(0.0, 0.0, 0.0), (0.4, 0.1, -0.5), (-0.2, 0.3, 0.3)], [(0.0, 0.0, 2.0), (0.0, 0.0, 2.0), (0.3, 0.0, 2.0)])
    if name == "mixed":
        return mr.mixed_mesh() + (k,) + look([(0.0, 0.0, 0.0), (0.1, 0.0, -0.3), (0.0, -0.1, 0.2)], [(0.0, 0.0, 3.0), (0.0, 0.1, 3.0), (0.2, 0.0, 3.0)])
    raise KeyError(name)


CASES = ("sphere inside", "sphere outside", "tube", "pixel grid", "mixed")
_wanted = {}


def boundaries_of(h, w):
    mask = np.ones((3, h, w), np.float32)
    mask[:, 0, :] = mask[:, :, -1] = 0.0
    mask[:, h // 3:h // 2, w // 4:w // 2] = 0.25
    return mask


def restated(key, vertices, faces, k, rotations, translations, h, w, masked, cull=0):
    """The restatement's outputs: made once per key and left unchanged."""
    key = (key, h, w, masked, cull)
    if key not in _wanted:
        _wanted[key] = mr.render(vertices, faces, k, rotations, translations, h, w, scales=SCALES,
                                 boundaries=boundaries_of(h, w) if masked else None, cull=cull)
    return _wanted[key]


def device_render(model, k, rotations, translations, h, w, masked, cull=None, brute=False):
    d = model.device
    return model.render(torch.from_numpy(k).to(d), rotations, translations, h, w, scales=SCALES,
                        boundaries=torch.from_numpy(boundaries_of(h, w)).to(d) if masked else None, cull=cull, brute=brute)


def assert_same(got, want, what):
    for name in OUTPUTS:
        if want[name] is None:
            assert got[name] is None, (what, name)
            continue
        a = got[name].cpu().numpy()
        assert a.dtype == want[name].dtype and a.shape == want[name].shape, (what, name)
        if a.tobytes() != want[name].tobytes():
            differ = np.argwhere(a.view(np.uint8 if a.dtype == np.uint8 else np.int32) != want[name].view(np.uint8 if a.dtype == np.uint8 else np.int32))
            raise AssertionError("%s: %s differs in %d places, first at %s: %r against %r" % (
                what, name, len(differ), tuple(differ[0]), a[tuple(differ[0])], want[name][tuple(differ[0])]))


def check(key, vertices, faces, k, rotations, translations, h, w, model=None):
    model = model or mesh.TriangleMesh(vertices, faces)
    for masked in (False, True):
        want = restated(key, vertices, faces, k, rotations, translations, h, w, masked)
        assert want["flags"].tolist() == [0, 3, 0] and not want["mask"][1].any()
        first = device_render(model, k, rotations, translations, h, w, masked)
        assert_same(first, want, "%s %dx%d masked=%s" % (key, h, w, masked))
        assert_same(device_render(model, k, rotations, translations, h, w, masked, brute=True), want, "%s %dx%d masked=%s brute" % (key, h, w, masked))
        again = device_render(model, k, rotations, translations, h, w, masked)          # the same call: the same bytes
        for name in OUTPUTS:
            assert (first[name] is None and again[name] is None) or torch.equal(first[name], again[name]), name
    return model


@pytest.mark.parametrize("h,w", shapes())
@pytest.mark.parametrize("name", CASES)
def test_render_matches_the_restatement(name, h, w):
    vertices, faces, k, rotations, translations = case(name, h, w)
    check(name, vertices, faces, k, rotations, translations, h, w)
    plain = restated(name, vertices, faces, k, rotations, translations, h, w, False)
    hit = plain["mask"][[0, 2]].mean()
    if name == "sphere inside":
        assert hit == 1.0
    else:
        assert hit > 0.2, hit          # a condition on the input: the case is seen
    if name == "pixel grid":
        assert plain["mask"][0].all() and (plain["depth"][0] == np.float32(2.0) / SCALES[0]).all()


@pytest.mark.parametrize("name", ("sphere outside", "tube"))
def test_culling_matches_the_restatement(name):
    h, w = 37, 53
    vertices, faces, k, rotations, translations = case(name, h, w)
    model = mesh.TriangleMesh(vertices, faces)
    seen = {}
    for cull, option in (("back", mr.CULL_BACK), ("front", mr.CULL_FRONT)):
        want = restated(name, vertices, faces, k, rotations, translations, h, w, False, option)
        for brute in (False, True):
            assert_same(device_render(model, k, rotations, translations, h, w, False, cull, brute), want, "%s cull %s brute %s" % (name, cull, brute))
        seen[cull] = want["mask"].sum()
    if name == "tube":          # its faces look at the axis: the camera inside sees fronts only
        assert seen["back"] > 0 and seen["front"] < seen["back"]
    else:
        assert seen["back"] > 0 and seen["front"] > 0


def raw_render(model, k, rotations, translations, h, w, options=0, only_depth=True):
    """endo_mesh_render itself with a workspace of the test's own: (depth, the number of queued triangles)."""
    lib = ea._lib.load()
    d = model.device
    n = k.shape[0]
    kd = torch.from_numpy(k).to(d)
    rot, tr = torch.from_numpy(np.ascontiguousarray(rotations, np.float64)).to(d), torch.from_numpy(np.ascontiguousarray(translations, np.float64)).to(d)
    scales = torch.from_numpy(SCALES).to(d)
    triangles = int(model.faces.shape[0])
    need = int(lib.endo_mesh_render_workspace_bytes(n, h, w, triangles))
    workspace = torch.empty(need, dtype=torch.uint8, device=d)
    depth = torch.empty((n, 1, h, w), dtype=torch.float32, device=d)
    extra = None if only_depth else torch.empty((n, h, w), dtype=torch.int32, device=d)
    ea._lib.check(lib.endo_mesh_render(ea._lib.ptr(model.vertices), int(model.vertices.shape[1]), int(model.vertices.shape[0]),
                                       ea._lib.ptr(model.faces), triangles, ea._lib.ptr(kd), ea._lib.ptr(rot), ea._lib.ptr(tr),
                                       ea._lib.ptr(scales), None, n, h, w, options, ea._lib.ptr(depth), None, ea._lib.ptr(extra), None, None, None,
                                       None, ea._lib.ptr(workspace), need, ea._lib.stream()), "endo_mesh_render")
    at = (n * h * w * 8 + 255) // 256 * 256
    queued = int(workspace[at:at + 8].view(torch.int64).cpu()[0])
    return depth, extra, queued


def test_optional_outputs_may_be_null_and_both_passes_run():
    h, w = 37, 53
    vertices, faces, k, rotations, translations = case("mixed", h, w)
    model = mesh.TriangleMesh(vertices, faces)
    want = restated("mixed", vertices, faces, k, rotations, translations, h, w, False)
    depth, _, queued = raw_render(model, k, rotations, translations, h, w)
    assert depth.cpu().numpy().tobytes() == want["depth"].tobytes()
    # the two frames with a scale: the one large triangle is queued; the small ones, under a pixel across, have boxes of at most 3 x 3
    # pixels and are tested in place or lie outside the image
    assert queued == 2, queued
    assert (want["triangle"][[0, 2]] == faces.shape[0] - 1).any() and ((want["triangle"][[0, 2]] >= 0) & (want["triangle"][[0, 2]] < faces.shape[0] - 1)).any()
    depth, triangle, brute_queued = raw_render(model, k, rotations, translations, h, w, options=mr.BRUTE, only_depth=False)
    assert depth.cpu().numpy().tobytes() == want["depth"].tobytes() and triangle.cpu().numpy().tobytes() == want["triangle"].tobytes()
    assert brute_queued == 2 * faces.shape[0]          # every pixel against every triangle


def test_a_fused_surface_with_colours():
    """TriangleMesh(*volume.extract_mesh()[::2]): (P, 6) rows and int32 faces where they are, seen by the volume's own cameras."""
    n, h, w = 3, 37, 53
    volume = integrated("40x24x20", 8, h, w)
    device = on_device(volume)
    rows, _, faces = device.extract_mesh(1.0)
    assert rows.shape[1] == 6 and faces.dtype == torch.int32 and faces.shape[0] > 100
    model = mesh.TriangleMesh(*device.extract_mesh(1.0)[::2])
    assert model.has_colors and model.vertices.data_ptr() != 0
    k, rotations, translations = cameras(n, h, w, centre_of(volume))
    check("fused", rows.cpu().numpy(), faces.cpu().numpy(), k, rotations, translations, h, w, model=model)
    want = restated("fused", None, None, None, None, None, h, w, False)
    hit = want["mask"][0, 0] > 0
    assert hit.sum() > 100 and want["colors"][0][hit].any()
    # the mesh is the volume's zero crossing: its depth agrees with the ray-cast of the same volume to a fraction of a voxel
    cast = device.render(torch.from_numpy(k).cuda(), rotations, translations, h, w, scales=SCALES)
    both = hit & (cast["mask"][0, 0].cpu().numpy() > 0)
    gap = np.abs(cast["depth"][0, 0].cpu().numpy()[both] - want["depth"][0, 0][both]) * SCALES[0]
    print("mesh against ray-cast depth on %d pixels: median %.3g max %.3g (voxel %.3g)" % (both.sum(), np.median(gap), gap.max(), volume.vs))
    assert both.sum() > 100 and np.median(gap) < float(volume.vs)


def test_an_empty_mesh_and_bad_arguments():
    h, w = 16, 24
    k = np.stack([mr.intrinsics(20.0, h, w)] * 3)
    pose = (np.stack([np.eye(3)] * 3), np.zeros((3, 3)))
    for vertices, faces in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)),
                            (np.zeros((0, 6), np.float32), np.array([[0, 1, 2]], np.int32))):
        out = device_render(mesh.TriangleMesh(vertices, faces), k, *pose, h, w, False)
        assert_same(out, mr.render(vertices, faces, k, *pose, h, w, scales=SCALES), "empty")
        assert not out["mask"].any() and (out["triangle"] == -1).all()
    model = mesh.TriangleMesh(*mr.icosphere(1))
    assert mesh.flag_names(device_render(model, k, *pose, h, w, False)["flags"]) == ["ok", "bad_scale", "ok"]
    with pytest.raises(ValueError, match="scales must hold one value per frame: 3, not 2"):
        model.render(torch.from_numpy(k).cuda(), *pose, h, w, scales=[1.0, 1.0])
    with pytest.raises(ValueError, match="boundaries must be"):
        model.render(torch.from_numpy(k).cuda(), *pose, h, w, boundaries=torch.ones(3, h, w + 1, device="cuda"))
    target = model.target()
    assert isinstance(target, ea.registration.TargetModel) and target.count == 42
