"""evaluate.run_fusion_phase(refine=K): on the sequence tests/test_gpu_fusion_phase.py builds, fused_tracking.csv with one row per frame
that took part while refine=0 is what it was; and on a synthetic sequence of tests/fusion_track_restate.py's curved scene with a
tracker's errors, the refined poses against the truth.  Run with ``pytest -m gpu`` on an MI355X."""
import csv
import importlib
import os

import numpy as np
import pytest
import torch

import fusion_track_restate as tr
from test_gpu_evaluate import sequence, trained  # noqa: F401  (the two fixtures of the example sequence)

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate, fusion = ea.evaluate, ea.fusion

BEFORE = ["dims", "empty", "frames", "observed_voxels", "origin", "points", "registration", "voxel_size", "zero_range"]


def read_table(path):
    with open(str(path)) as f:
        return list(csv.reader(f))


def test_run_fusion_phase_tracks_every_frame_that_took_part(sequence, trained, tmp_path):
    model, _ = trained
    model.eval()
    names = [str(p) for p in ea.utils.get_filenames_from_frame_indexes(os.path.dirname(sequence), ea.reader.read_visible_view_indexes(sequence))]
    frames = ea.dataset.TestFrames(names, batch_size=2, suggested_h=256, suggested_w=320)
    pose_file = tmp_path / "initial_poses"
    pose_file.write_text("4594, 10.5, -3.25, 7.0, 0.5, 0.5, -0.5, 0.5\n4584, -1.5, 2.0, 30.0, 0.9, 0.1, 0.3, -0.2\n")
    _, translations, rotations = ea.reader.read_initial_pose_file(pose_file)
    kw = dict(resolution=64, min_weight=1.0, ply_text=True)
    plain = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "plain", **kw)
    off = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "off", refine=0, **kw)
    refined = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "refined", refine=1, **kw)

    # refine=0: the files and the keys of before
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted(p.name for p in (tmp_path / "off").iterdir()) == ["fused_surface.ply"]
    assert (tmp_path / "plain" / "fused_surface.ply").read_bytes() == (tmp_path / "off" / "fused_surface.ply").read_bytes()
    assert sorted(off) == sorted(plain) == BEFORE
    assert {k: v for k, v in off.items() if k != "origin"} == {k: v for k, v in plain.items() if k != "origin"}
    # refine=1: the surface still, and the table
    took_part = ["00004584", "00004594"]
    assert sorted(p.name for p in (tmp_path / "refined").iterdir()) == ["fused_surface.ply", "fused_tracking.csv"]
    assert sorted(refined) == sorted(BEFORE + ["tracking", "poses"]) and refined["frames"] == 2
    assert refined["dims"] == plain["dims"] and refined["voxel_size"] == plain["voxel_size"] and refined["points"] >= 1
    table = read_table(tmp_path / "refined" / "fused_tracking.csv")
    assert tuple(table[0]) == evaluate.TRACKING_COLUMNS == ("name", "status", "iterations", "count", "rms_before", "rms_after",
                                                            "rotation_degrees", "translation", "scale_ratio")
    assert sorted(row[0] for row in table[1:]) == took_part == sorted(refined["poses"]) and len(refined["tracking"]) == 2
    for row, kept in zip(table[1:], refined["tracking"]):
        print("tracking of %s" % ", ".join(row))
        assert (row[0], row[1], int(row[2]), int(row[3])) == tuple(kept[:4]) and row[1] in ("ok", "too_few", "singular")
        for text, value in zip(row[4:], kept[4:]):
            assert float(text) == value or (np.isnan(float(text)) and np.isnan(value))
        rotation, translation, scale = refined["poses"][row[0]]
        if row[1] != "ok":          # it keeps the tracker's pose
            assert rotation.tobytes() == np.asarray(rotations[row[0]], np.float64).tobytes() and float(row[6]) < 1e-5 and float(row[8]) == 1.0
        assert abs(np.linalg.det(rotation) - 1.0) < 1e-9 and scale > 0
    with pytest.raises(ValueError, match="refine"):
        evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "never", refine=-1, **kw)


class Predictions(object):
    """A stand-in for the network in eval mode: the sequence's depth maps, batch after batch."""
    training = False

    def __init__(self, batches):
        self.batches, self.calls = batches, 0

    def __call__(self, masked):
        self.calls += 1
        return self.batches[self.calls - 1]


def test_refining_a_jittered_sequence_brings_its_frames_closer_to_the_truth(tmp_path):
    """The fixture of test_the_restated_refinement_brings_a_jittered_sequence_closer_to_the_truth (tests/test_fusion_track_host.py),
    where the restated pipeline lowers the mean mapped-point error 3.8 x (0.664 -> 0.173 units): on the device the mean decreases, and
    the frames' statuses are the restatement's."""
    seq = tr.jittered_sequence()
    d = torch.device("cuda:0")
    n, h, w = seq["depth"].shape
    names = ["%08d" % (100 + f) for f in range(n)]
    rng = np.random.default_rng(5)
    batches, predictions = [], []
    for b in range(0, n, 4):          # a batch of four and one of two
        pick = slice(b, min(b + 4, n))
        count = len(names[pick])
        batches.append({"names": names[pick], "colors": torch.from_numpy(rng.uniform(-1, 1, (count, 3, h, w)).astype(np.float32)).to(d),
                        "boundaries": torch.from_numpy(seq["boundaries"][pick]).to(d).unsqueeze(1),
                        "intrinsics": torch.from_numpy(seq["intrinsics"][pick]).to(d)})
        predictions.append(torch.from_numpy(seq["depth"][pick]).to(d).unsqueeze(1))
    model = Predictions(predictions)
    rotations = {name: seq["rotations"][f] for f, name in enumerate(names)}
    translations = {name: seq["translations"][f] for f, name in enumerate(names)}
    result = evaluate.run_fusion_phase(model, batches, translations, rotations, tmp_path / "out", resolution=64, refine=1)
    assert model.calls == 2 and result["frames"] == n and result["empty"] == [] and result["zero_range"] == []
    want_before, want_after, _, _, _, want_fits = tr.refine(seq, 1)
    table = read_table(tmp_path / "out" / "fused_tracking.csv")
    assert [row[0] for row in table[1:]] == names and [row[1] for row in table[1:]] == [fit["status"] for fit in want_fits] == ["ok"] * n
    own, _ = tr.fr.frame_scales(seq["depth"], seq["boundaries"])
    before = tr.errors_to_truth(seq, seq["rotations"], seq["translations"], own.astype(np.float64))
    poses = [result["poses"][name] for name in names]
    after = tr.errors_to_truth(seq, [p[0] for p in poses], [p[1] for p in poses], [p[2] for p in poses])
    print("mean mapped-point error %.4f -> %.4f units (the restatement: %.4f -> %.4f); per frame %s" % (
        before.mean(), after.mean(), want_before.mean(), want_after.mean(), after.round(4)))
    assert np.abs(before - want_before).max() < 1e-12
    assert after.mean() < before.mean()
    for f, (row, pose) in enumerate(zip(table[1:], poses)):          # the table's changes are those from the tracker's pose and the own scale
        assert abs(float(row[8]) - pose[2] / float(own[f])) <= 1e-12 and abs(float(row[7]) - np.linalg.norm(pose[1] - seq["translations"][f])) <= 1e-12
        assert 0.0 < float(row[6]) < 3.0 and float(row[5]) < float(row[4])
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["fused_surface.ply", "fused_tracking.csv"] and result["points"] > 100
