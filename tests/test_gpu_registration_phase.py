"""evaluate.run_registration_phase end to end on the committed example sequence: the posed test outputs per batch, every frame's cloud
registered to a model read from a PLY file (the sequence's own clouds moved by a known similarity), registration_errors.csv and the
registered clouds.  Run with ``pytest -m gpu`` on an MI355X."""
import csv
import importlib
import os

import numpy as np
import pytest

import registration_restate as rr
from test_gpu_evaluate import sequence, trained  # noqa: F401  (the two fixtures of the example sequence)
from test_gpu_evaluate_posed import read_ply

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate, registration = ea.evaluate, ea.registration


def test_run_registration_phase_on_the_example_sequence(sequence, trained, tmp_path):
    model, _ = trained
    model.eval()
    names = [str(p) for p in ea.utils.get_filenames_from_frame_indexes(os.path.dirname(sequence), ea.reader.read_visible_view_indexes(sequence))]
    frames = ea.dataset.TestFrames(names, batch_size=2, suggested_h=256, suggested_w=320)
    pose_file = tmp_path / "initial_poses"
    pose_file.write_text("4594, 10.5, -3.25, 7.0, 0.5, 0.5, -0.5, 0.5\n4584, -1.5, 2.0, 30.0, 0.9, 0.1, 0.3, -0.2\n")
    _, translations, rotations = ea.reader.read_initial_pose_file(pose_file)
    (batch,) = list(frames)
    out = evaluate.posed_test_outputs(model, batch, [rotations[n] for n in batch["names"]], [translations[n] for n in batch["names"]])
    off = out["offsets"]
    points = out["points"][:off[-1]].cpu().numpy()
    assert off[1] > 1000 and np.isfinite(points).all()
    # the "CT model": the sequence's clouds under a known similarity, through a PLY file
    truth = (0.93, rr.rotation_about((1.0, -0.4, 0.2), 14.0), np.array([-20.0, 5.0, 11.0]))
    target = points.copy()
    target[:, :3] = rr.apply(points, *truth).astype(np.float32)
    ea.utils.write_point_cloud(tmp_path / "model.ply", target, text=False)
    model_cloud = registration.TargetModel.from_ply(tmp_path / "model.ply")
    assert model_cloud.count == off[-1] and np.array_equal(model_cloud.points.cpu().numpy(), target[:, :3])
    middle = points[:, :3].astype(np.float64).mean(axis=0)
    start_scale, start_rot = truth[0] * 1.0005, truth[1] @ rr.rotation_about((0.0, 1.0, 0.0), 0.02)
    start = np.eye(4)          # beside the truth, as a tracker-to-model calibration would be
    start[:3, :3] = start_scale * start_rot
    start[:3, 3] = truth[0] * (truth[1] @ middle) + truth[2] - start_scale * (start_rot @ middle) + 0.005
    missing = dict(rotations)
    del missing["00004594"]
    with pytest.raises(KeyError):
        evaluate.run_registration_phase(model, frames, translations, missing, model_cloud, tmp_path / "never", initial=start)
    assert not (tmp_path / "never").exists()          # raised before anything ran
    out_dir = tmp_path / "out"
    result = evaluate.run_registration_phase(model, frames, translations, rotations, model_cloud, out_dir, initial=start)
    assert result["frames"] == 2 and result["registered"] == 2 and result["failed"] == []
    limit = 4.0 * 2.0 ** -23 * max(np.abs(points[:, :3]).max(), np.abs(target[:, :3]).max())
    with open(str(out_dir / "registration_errors.csv")) as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == evaluate.REGISTRATION_COLUMNS == ("name", "points", "inliers", "scale", "mean", "rms", "max", "iterations",
                                                                 "converged")
    assert [row[0] for row in table[1:]] == batch["names"]
    squares, inliers = 0.0, 0
    for f, row in enumerate(table[1:]):
        rows = points[off[f]:off[f + 1]]
        assert int(row[1]) == rows.shape[0] and int(row[2]) == rows.shape[0] and row[8] == "1" and int(row[7]) <= 30
        print("frame %s: scale %s rms %s max %s after %s iterations (limit %.3g)" % (row[0], row[3], row[5], row[6], row[7], limit))
        assert abs(float(row[3]) - truth[0]) <= 1e-6 and 0.0 <= float(row[4]) <= float(row[5]) <= limit and float(row[5]) <= float(row[6]) <= 2.0 * limit
        moved = read_ply(out_dir / ("registered_%s.ply" % row[0]))
        assert np.array_equal(moved[:, 3:], rows[:, 3:])          # colours kept
        assert np.sqrt(((moved[:, :3].astype(np.float64) - target[off[f]:off[f + 1], :3]) ** 2).sum(axis=1).mean()) <= limit
        squares += float(row[5]) ** 2 * int(row[2])
        inliers += int(row[2])
    assert abs(result["rms"] - np.sqrt(squares / inliers)) <= 1e-12
    assert sorted(p.name for p in out_dir.iterdir()) == ["registered_00004584.ply", "registered_00004594.ply", "registration_errors.csv"]
    # without clouds: the table only; a cap below every distance leaves nothing to fit, and the frame is reported, not raised
    none = evaluate.run_registration_phase(model, frames, translations, rotations, model_cloud, tmp_path / "none", initial=start,
                                           write_ply=False, max_distance=1e-12)
    assert none["registered"] == 0 and none["failed"] == batch["names"] and np.isnan(none["rms"])
    assert [p.name for p in (tmp_path / "none").iterdir()] == ["registration_errors.csv"]
