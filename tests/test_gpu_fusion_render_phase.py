"""evaluate.run_fusion_phase(render=True) on the sequence tests/test_gpu_fusion_phase.py builds: fused_consistency.csv, one row per frame
that took part, and fused_color_<name>.png, the fused model as each frame sees it; render=False is what it was.  Run with
``pytest -m gpu`` on an MI355X."""
import csv
import importlib
import os

import numpy as np
import pytest

from test_gpu_evaluate import sequence, trained  # noqa: F401  (the two fixtures of the example sequence)
from test_gpu_evaluate_posed import read_png

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate, fusion = ea.evaluate, ea.fusion


def test_run_fusion_phase_renders_every_frame_that_took_part(sequence, trained, tmp_path):
    model, _ = trained
    model.eval()
    names = [str(p) for p in ea.utils.get_filenames_from_frame_indexes(os.path.dirname(sequence), ea.reader.read_visible_view_indexes(sequence))]
    frames = ea.dataset.TestFrames(names, batch_size=2, suggested_h=256, suggested_w=320)
    pose_file = tmp_path / "initial_poses"
    pose_file.write_text("4594, 10.5, -3.25, 7.0, 0.5, 0.5, -0.5, 0.5\n4584, -1.5, 2.0, 30.0, 0.9, 0.1, 0.3, -0.2\n")
    _, translations, rotations = ea.reader.read_initial_pose_file(pose_file)
    kw = dict(resolution=64, min_weight=1.0, ply_text=True)
    plain = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "plain", **kw)
    off = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "off", render=False, **kw)
    shown = evaluate.run_fusion_phase(model, frames, translations, rotations, tmp_path / "shown", render=True, **kw)

    # render=False: the files and the keys of before
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted(p.name for p in (tmp_path / "off").iterdir()) == ["fused_surface.ply"]
    assert (tmp_path / "plain" / "fused_surface.ply").read_bytes() == (tmp_path / "off" / "fused_surface.ply").read_bytes()
    assert sorted(off) == sorted(plain) == ["dims", "empty", "frames", "observed_voxels", "origin", "points", "registration", "voxel_size",
                                            "zero_range"]
    # render=True: the same surface, one image per frame and the table
    assert shown["frames"] == 2 and shown["empty"] == [] and shown["zero_range"] == []
    took_part = ["00004584", "00004594"]
    assert sorted(p.name for p in (tmp_path / "shown").iterdir()) == sorted(
        ["fused_surface.ply", "fused_consistency.csv"] + ["fused_color_%s.png" % name for name in took_part])
    assert (tmp_path / "shown" / "fused_surface.ply").read_bytes() == (tmp_path / "plain" / "fused_surface.ply").read_bytes()
    assert {k: v for k, v in shown.items() if k not in ("consistency", "origin")} == {k: v for k, v in plain.items() if k != "origin"}
    with open(str(tmp_path / "shown" / "fused_consistency.csv")) as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == evaluate.CONSISTENCY_COLUMNS == ("name", "pixels", "abs_rel", "sigma_1", "sigma_2", "sigma_3")
    assert sorted(row[0] for row in table[1:]) == took_part and len(shown["consistency"]) == 2
    for row, kept in zip(table[1:], shown["consistency"]):
        pixels, abs_rel, s1, s2, s3 = int(row[1]), float(row[2]), float(row[3]), float(row[4]), float(row[5])
        print("fused consistency of %s: %d pixels, abs rel %.4g, sigma %.4g %.4g %.4g" % (row[0], pixels, abs_rel, s1, s2, s3))
        assert (row[0], pixels, abs_rel, s1, s2, s3) == tuple(kept)
        assert 0 < pixels <= 256 * 320
        assert np.isfinite(abs_rel) and abs_rel >= 0.0
        assert 0.0 <= s1 <= s2 <= s3 <= 1.0
        image = read_png(tmp_path / "shown" / ("fused_color_%s.png" % row[0]))
        assert image.shape == (256, 320, 3) and image.dtype == np.uint8 and int((image.reshape(-1, 3).max(axis=1) > 0).sum()) <= pixels
