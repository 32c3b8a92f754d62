"""fusion.TSDFVolume.extract_mesh on the device against tests/fusion_mesh_restate.py: vertices, normals and faces are compared by
``tobytes()``.  Seeded noise goes straight into the volume's planes, so every marching-cubes case is met; the long volumes cross the
face kernel's 256-cell chunk and every 64-lane wave boundary.  Run with ``pytest -m gpu`` on an MI355X."""
import importlib
import os

import numpy as np
import pytest
import torch

import fusion_mesh_restate as mr
import fusion_restate as fr
from test_fusion_mesh_host import read_mesh_ply
from test_gpu_evaluate import sequence, trained  # noqa: F401  (the two fixtures of the example sequence)
from test_gpu_evaluate_posed import read_ply
from test_gpu_fusion import NORMAL, TRUNC, VS, origin_of

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate, fusion = ea.evaluate, ea.fusion

LONG, SMALL, FLAT = (260, 5, 4), (4, 2, 2), (4, 1, 3)          # two chunks of cells; the smallest grid with cells; one without


CASES = {
    "A": lambda: (mr.noise_volume(LONG, 11), 1.0),
    "B": lambda: (mr.noise_volume(LONG, 12, holes=0.15, low_weight=0.15), 2.0),
    "C-4x2x2": lambda: (mr.noise_volume(SMALL, 13), 1.0),
    "C-4x1x3": lambda: (mr.noise_volume(FLAT, 14), 1.0),
    "D-260x5x4": lambda: (mr.noise_volume(LONG, 15, positive=True), 1.0),
    "D-4x2x2": lambda: (mr.noise_volume(SMALL, 16, positive=True), 1.0),
    "D-4x1x3": lambda: (mr.noise_volume(FLAT, 17, positive=True), 1.0),
    "sphere": lambda: (mr.sphere_volume(), 1.0),
}
_wanted = {}


def wanted(name):
    """(the restatement's volume, min_weight, its mesh): made once per case and left unchanged."""
    if name not in _wanted:
        volume, min_weight = CASES[name]()
        _wanted[name] = (volume, min_weight, mr.mesh(volume, min_weight))
    return _wanted[name]


def on_device(volume):
    out = fusion.TSDFVolume(volume.origin, float(volume.vs), (volume.nx, volume.ny, volume.nz), truncation=float(volume.trunc),
                            device="cuda:0")
    out.tsdf.copy_(torch.from_numpy(volume.tsdf))
    out.weight.copy_(torch.from_numpy(volume.weight))
    out.color.copy_(torch.from_numpy(volume.color))
    return out


def assert_same_mesh(got, want, what):
    names = ("vertices", "normals", "faces")
    for name, a, b in zip(names, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s is %s %s, not %s %s" % (what, name, a.dtype, a.shape, b.dtype, b.shape)
        assert a.tobytes() == b.tobytes(), "%s: %s differs in %d rows of %d" % (what, name, int((a != b).any(axis=1).sum()), a.shape[0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_extract_mesh_matches_the_restatement(name):
    volume, min_weight, want = wanted(name)
    part, case = mr.cell_cases(volume, min_weight)
    if name == "A":          # on the input: 3108 cells, about 12 per case
        assert part.all() and case.size == 3108 and np.unique(case).shape[0] == 256
    if name == "B":
        assert 100 < part.sum() < part.size // 4 and (volume.weight == 0).any() and (volume.weight == 1).any() and (volume.weight == 2).any()
        assert np.unique(want[2]).shape[0] < want[0].shape[0]          # rows that no cell taking part touches
    if name.startswith("C"):
        assert want[0].shape[0] > 0 and (want[2].shape[0] > 0) == (name == "C-4x2x2") and case.size == (3 if name == "C-4x2x2" else 0)
    if name.startswith("D"):
        assert want[0].shape == (0, 6) and want[2].shape == (0, 3)
    if name == "sphere":
        assert want[0].shape[0] - 3 * want[2].shape[0] // 2 + want[2].shape[0] == 2          # closed, genus 0 (test_fusion_mesh_host.py)
    device = on_device(volume)
    before = device.extract(min_weight).cpu().numpy()
    got = device.extract_mesh(min_weight)
    assert all(t.is_cuda for t in got)
    assert_same_mesh(got, want, name)
    after = device.extract(min_weight).cpu().numpy()
    assert before.tobytes() == after.tobytes() == want[0].tobytes()
    assert device.tsdf.cpu().numpy().tobytes() == volume.tsdf.tobytes() and device.weight.cpu().numpy().tobytes() == volume.weight.tobytes()
    if name in ("A", "B"):          # another threshold on the same planes
        other = 1.0 if name == "B" else 2.0
        assert_same_mesh(device.extract_mesh(other), mr.mesh(volume, other), "%s at min_weight %g" % (name, other))


def test_an_integrated_volume():
    """Two frames of a plane into 40 x 24 x 20 voxels: the planes are the restatement's, and so is the mesh at both thresholds."""
    h, w, dims = 16, 24, (40, 24, 20)
    k = fr.intrinsics(20.0, h, w)
    rotations = np.stack([np.eye(3), fr.rotation_about((1, 1, 0), 8.0)])
    translations = np.array([[0.0, 0.0, 0.0], [-2.0, 0.5, -3.0]])
    depth = fr.render_plane(NORMAL, 30.0 * NORMAL[2], rotations, translations, k, h, w)
    rng = np.random.default_rng(2)
    depth += rng.uniform(-0.2, 0.2, depth.shape).astype(np.float32) * (depth > 0)
    mask = np.ones_like(depth)
    colors = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    want = fr.Volume(origin_of(dims), VS, dims, truncation=TRUNC)
    assert fr.integrate(want, depth, mask, colors, np.stack([k] * 2), rotations, translations, scales=np.ones(2, np.float32)) == ["ok", "ok"]
    d = torch.device("cuda:0")
    volume = fusion.TSDFVolume(origin_of(dims), VS, dims, truncation=TRUNC, device=d)
    flags = volume.integrate(torch.from_numpy(depth).to(d), torch.from_numpy(mask).to(d), torch.from_numpy(colors).to(d),
                             torch.from_numpy(np.stack([k] * 2)).to(d), rotations, translations, scales=np.ones(2, np.float32))
    assert flags == ["ok", "ok"] and volume.tsdf.cpu().numpy().tobytes() == want.tsdf.tobytes()
    for min_weight in (1.0, 2.0):
        got = volume.extract_mesh(min_weight)
        assert got[0].cpu().numpy().tobytes() == volume.extract(min_weight).cpu().numpy().tobytes()
        mesh = mr.mesh(want, min_weight)
        assert_same_mesh(got, mesh, "integrated, min_weight %g" % min_weight)
        assert mesh[2].shape[0] > 100
        # the normals look at the cameras: against the plane's normal, which points away from them
        facing = mesh[1].astype(np.float64) @ NORMAL
        assert np.median(facing) < -0.9


def test_capacities_below_the_counts_write_nothing_past_them():
    volume, min_weight, want = wanted("A")
    points, triangles = want[0].shape[0], want[2].shape[0]
    device = on_device(volume)
    lib = ea._lib.load()
    nx, ny, nz = device.dims
    need = int(lib.endo_fusion_mesh_workspace_bytes(nx, ny, nz))
    workspace = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    totals = torch.empty(4, dtype=torch.int64, device="cuda:0")
    vol = (fusion._host_doubles(device.origin), device.voxel_size, nx, ny, nz, ea._lib.ptr(device.tsdf), ea._lib.ptr(device.weight),
           ea._lib.ptr(device.color), min_weight)
    state = (ea._lib.ptr(totals), ea._lib.ptr(workspace), need, ea._lib.stream())
    ea._lib.check(lib.endo_fusion_mesh_count(*(vol + state)), "endo_fusion_mesh_count")
    assert totals.cpu().tolist() == [0, points, 0, triangles]
    for rows_kept, faces_kept in ((points // 2 + 1, triangles // 3 + 1), (1, 1), (0, 0)):
        rows = torch.full((points, 6), -7.0, device="cuda:0")
        normals = torch.full((points, 3), -7.0, device="cuda:0")
        faces = torch.full((triangles, 3), -7, dtype=torch.int32, device="cuda:0")
        ea._lib.check(lib.endo_fusion_mesh_vertices(*(vol + (ea._lib.ptr(rows), ea._lib.ptr(normals), rows_kept) + state)), "vertices")
        ea._lib.check(lib.endo_fusion_mesh_faces(*(vol + (ea._lib.ptr(faces), faces_kept) + state)), "faces")
        rows, normals, faces = rows.cpu().numpy(), normals.cpu().numpy(), faces.cpu().numpy()
        assert rows[:rows_kept].tobytes() == want[0][:rows_kept].tobytes() and (rows[rows_kept:] == -7.0).all()
        assert normals[:rows_kept].tobytes() == want[1][:rows_kept].tobytes() and (normals[rows_kept:] == -7.0).all()
        assert faces[:faces_kept].tobytes() == want[2][:faces_kept].tobytes() and (faces[faces_kept:] == -7).all()
    # faces are int32: a capacity they cannot index is refused before any launch
    one = torch.empty((1, 6), dtype=torch.int32, device="cuda:0")
    assert lib.endo_fusion_mesh_faces(*(vol + (ea._lib.ptr(one), 2 ** 31) + state)) == -1
    assert lib.endo_fusion_mesh_vertices(*(vol + (ea._lib.ptr(one), ea._lib.ptr(one), 2 ** 31) + state)) == -1
    assert lib.endo_fusion_mesh_count(*(vol + (ea._lib.ptr(totals), ea._lib.ptr(workspace), need - 1, ea._lib.stream()))) == -1
    with pytest.raises(ValueError, match="NaN"):
        device.extract_mesh(float("nan"))


def test_run_fusion_phase_writes_the_mesh(sequence, trained, tmp_path):
    model, _ = trained
    model.eval()
    names = [str(p) for p in ea.utils.get_filenames_from_frame_indexes(os.path.dirname(sequence), ea.reader.read_visible_view_indexes(sequence))]
    frames = ea.dataset.TestFrames(names, batch_size=2, suggested_h=256, suggested_w=320)
    pose_file = tmp_path / "initial_poses"
    pose_file.write_text("4594, 10.5, -3.25, 7.0, 0.5, 0.5, -0.5, 0.5\n4584, -1.5, 2.0, 30.0, 0.9, 0.1, 0.3, -0.2\n")
    _, translations, rotations = ea.reader.read_initial_pose_file(pose_file)
    plain = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "plain", resolution=64, min_weight=1.0, ply_text=True)
    meshed = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "meshed", resolution=64, min_weight=1.0,
                                       ply_text=True, mesh=True)
    assert "triangles" not in plain and sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["fused_surface.ply"]
    assert sorted(p.name for p in (tmp_path / "meshed").iterdir()) == ["fused_mesh.ply", "fused_surface.ply"]
    assert (tmp_path / "plain" / "fused_surface.ply").read_bytes() == (tmp_path / "meshed" / "fused_surface.ply").read_bytes()
    assert {k: v for k, v in meshed.items() if k not in ("triangles", "origin")} == {k: v for k, v in plain.items() if k != "origin"}
    assert np.array_equal(meshed["origin"], plain["origin"])

    # the same volume by hand, downloaded: the file is the restatement's mesh of it
    (batch,) = list(frames)
    rots, trans = [rotations[n] for n in batch["names"]], [translations[n] for n in batch["names"]]
    out = evaluate.posed_test_outputs(model, batch, rots, trans)
    volume = fusion.TSDFVolume.around(out["points"][:out["offsets"][-1]], resolution=64, truncation_voxels=4)
    volume.integrate(out["depth"], batch["boundaries"].cuda(), out["color_images"], batch["intrinsics"].cuda(), rots, trans)
    assert meshed["dims"] == volume.dims
    want = fr.Volume(volume.origin, volume.voxel_size, volume.dims, volume.truncation, volume.max_weight)
    want.tsdf, want.weight, want.color = volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy(), volume.color.cpu().numpy()
    mesh = mr.mesh(want, 1.0)
    written = read_mesh_ply(tmp_path / "meshed" / "fused_mesh.ply")
    assert_same_mesh(written, mesh, "fused_mesh.ply")
    assert meshed["triangles"] == mesh[2].shape[0] > 100 and meshed["points"] == mesh[0].shape[0]
    assert read_ply(tmp_path / "meshed" / "fused_surface.ply").tobytes() == mesh[0].tobytes()
    # binary, with a registration beside it: the three files of the phase and the mesh
    target = mesh[0][:, :3].copy()
    both = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "both", resolution=64, min_weight=1.0, mesh=True,
                                     target=target, initial=np.eye(4))
    assert sorted(p.name for p in (tmp_path / "both").iterdir()) == ["fused_mesh.ply", "fused_registered.ply", "fused_registration.csv",
                                                                     "fused_surface.ply"]
    assert_same_mesh(read_mesh_ply(tmp_path / "both" / "fused_mesh.ply"), mesh, "binary fused_mesh.ply")
    assert both["triangles"] == meshed["triangles"] and both["registration"] is not None
