"""evaluate.run_fusion_phase end to end on the committed example sequence: the posed outputs per batch fused into one volume around the
posed clouds, fused_surface.ply, and with a target the one registration of the fused rows.  Run with ``pytest -m gpu`` on an MI355X."""
import csv
import importlib
import os

import numpy as np
import pytest

import fusion_restate as fr
import registration_restate as rr
from test_gpu_evaluate import sequence, trained  # noqa: F401  (the two fixtures of the example sequence)
from test_gpu_evaluate_posed import read_ply

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate, fusion, registration = ea.evaluate, ea.fusion, ea.registration


def test_run_fusion_phase_on_the_example_sequence(sequence, trained, tmp_path):
    model, _ = trained
    model.eval()
    names = [str(p) for p in ea.utils.get_filenames_from_frame_indexes(os.path.dirname(sequence), ea.reader.read_visible_view_indexes(sequence))]
    frames = ea.dataset.TestFrames(names, batch_size=2, suggested_h=256, suggested_w=320)
    pose_file = tmp_path / "initial_poses"
    pose_file.write_text("4594, 10.5, -3.25, 7.0, 0.5, 0.5, -0.5, 0.5\n4584, -1.5, 2.0, 30.0, 0.9, 0.1, 0.3, -0.2\n")
    _, translations, rotations = ea.reader.read_initial_pose_file(pose_file)
    missing = dict(rotations)
    del missing["00004594"]
    with pytest.raises(KeyError):
        evaluate.run_fusion_phase(model, frames, translations, missing, tmp_path / "never", resolution=64)
    assert not (tmp_path / "never").exists()          # raised before anything was written

    out_dir = tmp_path / "out"
    result = evaluate.run_fusion_phase(model, frames, translations, rotations, out_dir, resolution=64, min_weight=1.0, ply_text=True)
    assert result["frames"] == 2 and result["empty"] == [] and result["zero_range"] == [] and result["registration"] is None
    assert sorted(p.name for p in out_dir.iterdir()) == ["fused_surface.ply"]
    written = read_ply(out_dir / "fused_surface.ply")

    # the pieces by hand on the same batch
    (batch,) = list(frames)
    rots, trans = [rotations[n] for n in batch["names"]], [translations[n] for n in batch["names"]]
    out = evaluate.posed_test_outputs(model, batch, rots, trans)
    off = out["offsets"]
    volume = fusion.TSDFVolume.around(out["points"][:off[-1]], resolution=64, truncation_voxels=4)
    flags = volume.integrate(out["depth"], batch["boundaries"].cuda(), out["color_images"], batch["intrinsics"].cuda(), rots, trans)
    rows = volume.extract(1.0).cpu().numpy()
    assert flags == ["ok", "ok"]
    assert result["dims"] == volume.dims and result["voxel_size"] == volume.voxel_size and np.array_equal(result["origin"], volume.origin)
    assert result["points"] == rows.shape[0] == written.shape[0] >= 1 and result["observed_voxels"] == volume.observed_voxels() > 0
    assert written.tobytes() == rows.tobytes()
    assert max(volume.dims) <= 64 + 1 + 16 + 3 and abs(volume.truncation - 4.0 * volume.voxel_size) <= 1e-12

    # which are the restatement's rows on the downloaded depth
    want = fr.Volume(volume.origin, volume.voxel_size, volume.dims, volume.truncation, volume.max_weight)
    n, _, h, w = out["depth"].shape
    want_flags = fr.integrate(want, out["depth"].cpu().numpy().reshape(n, h, w), batch["boundaries"].cpu().numpy().reshape(n, h, w),
                              out["color_images"].cpu().numpy(), batch["intrinsics"].cpu().numpy(), np.stack(rots), np.stack(trans))
    assert want_flags == flags
    assert volume.tsdf.cpu().numpy().tobytes() == want.tsdf.tobytes() and volume.weight.cpu().numpy().tobytes() == want.weight.tobytes()
    assert fr.extract(want, 1.0).tobytes() == rows.tobytes()
    lo = volume.origin
    hi = lo + volume.voxel_size * np.asarray(volume.dims)
    assert np.isfinite(rows).all() and (rows[:, :3] >= lo).all() and (rows[:, :3] <= hi).all()
    assert (rows[:, 3:] >= 0).all() and (rows[:, 3:] <= 255).all() and (rows[:, 3:] == np.rint(rows[:, 3:])).all()
    # the pose and scale conventions are the posed writer's: the fused surface lies on the posed clouds.  A posed point is where its
    # pixel's ray has sdf = 0; where neighbouring pixels (and the other frame, where it looks at the same place) agree to within a
    # voxel, a grid edge within one voxel diagonal of it changes sign.  That holds for most points, not at depth edges: the median.
    posed = out["points"][:off[-1]]
    near = registration.nearest_points(posed[::97].contiguous(), volume.extract(1.0))
    median = float(near["distance"].median())
    print("%d surface rows, %d observed voxels of %s; posed points to the surface: median %.3g mean %.3g max %.3g (voxel %.3g)" % (
        rows.shape[0], result["observed_voxels"], volume.dims, median, near["mean"], near["max"], volume.voxel_size))
    assert median <= np.sqrt(3.0) * volume.voxel_size

    # a target: the fused rows under a known similarity, the start beside it
    truth = (0.93, rr.rotation_about((1.0, -0.4, 0.2), 14.0), np.array([-20.0, 5.0, 11.0]))
    target = rows.copy()
    target[:, :3] = rr.apply(rows, *truth).astype(np.float32)
    middle = rows[:, :3].astype(np.float64).mean(axis=0)
    start_scale, start_rot = truth[0] * 1.0005, truth[1] @ rr.rotation_about((0.0, 1.0, 0.0), 0.02)
    start = np.eye(4)
    start[:3, :3] = start_scale * start_rot
    start[:3, 3] = truth[0] * (truth[1] @ middle) + truth[2] - start_scale * (start_rot @ middle) + 0.005
    reg_dir = tmp_path / "registered"
    fitted = evaluate.run_fusion_phase(model, frames, translations, rotations, reg_dir, resolution=64, min_weight=1.0, ply_text=True,
                                       target=target[:, :3].copy(), initial=start)
    assert sorted(p.name for p in reg_dir.iterdir()) == ["fused_registered.ply", "fused_registration.csv", "fused_surface.ply"]
    assert read_ply(reg_dir / "fused_surface.ply").tobytes() == rows.tobytes()
    with open(str(reg_dir / "fused_registration.csv")) as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == evaluate.REGISTRATION_COLUMNS and len(table) == 2
    row = table[1]
    print("fused registration: scale %s rms %s max %s after %s iterations" % (row[3], row[5], row[6], row[7]))
    assert int(row[1]) == rows.shape[0] and 3 <= int(row[2]) <= rows.shape[0] and row[8] == "1"          # (inliers: within 3 x rms of rounding noise)
    assert abs(float(row[3]) - truth[0]) <= 1e-6 and abs(fitted["registration"].scale - truth[0]) <= 1e-6
    moved = read_ply(reg_dir / "fused_registered.ply")
    assert np.array_equal(moved[:, 3:], rows[:, 3:])          # colours kept
    limit = 4.0 * 2.0 ** -23 * max(np.abs(rows[:, :3]).max(), np.abs(target[:, :3]).max())
    assert np.sqrt(((moved[:, :3].astype(np.float64) - target[:, :3]) ** 2).sum(axis=1).mean()) <= limit
