"""Timing prints of the posed test output (utils.write_test_output_with_initial_pose's counterpart): run by hand with ``pytest -m bench`` on
an MI355X; nothing is asserted about speed."""

import os
import shutil
import time

import numpy as np
import pytest
import torch

from test_gpu_evaluate import SEQ_NAME, dev, ea, evaluate, random_batch, sequence, trained  # noqa: F401 -- the last two are fixtures
from test_gpu_evaluate_posed import random_poses

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]


def per_call_us(launch, reps=500):
    for _ in range(10):
        assert launch() == 0
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        launch()
    stop.record()
    stop.synchronize()
    return 1000.0 * start.elapsed_time(stop) / reps


def test_bench_posed_test_phase(sequence, trained, tmp_path):
    """Device time of endo_evaluate_posed per batch (N = 8, 256 x 320; 500 back-to-back calls between two events) beside endo_evaluate's in
    the same job, and run_posed_test_phase frames/s at batch size 8 with and without writing the files beside run_test_phase's (64
    frames: copies of the example sequence's two).  Prints only; nothing is asserted about speed."""
    n, h, w = 8, 256, 320
    d = dev()
    t = [torch.from_numpy(a).to(d) for a in random_batch(n, h, w, seed=1)]
    rot, tr = (torch.from_numpy(a).to(d) for a in random_poses(n, 2))
    lib = ea._lib.load()
    p = ea._lib.ptr
    need = int(lib.endo_evaluate_workspace_bytes(n, h, w))
    need_posed = int(lib.endo_evaluate_posed_workspace_bytes(n, h, w))
    ws = torch.empty(max(need, need_posed), dtype=torch.uint8, device=d)
    depth = torch.empty((n, 1, h, w), device=d)
    panels = torch.empty((n, h, 2 * w, 3), dtype=torch.uint8, device=d)          # also the two (N, H, W, 3) images
    points = torch.empty((n * h * w, 6), device=d)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=d)
    ranges = torch.empty((n, 2), device=d)
    color_images, depth_images = panels.view(2, n, h, w, 3)[0], panels.view(2, n, h, w, 3)[1]

    def plain():
        return lib.endo_evaluate(p(t[0]), p(t[1]), p(t[2]), p(t[3]), n, h, w, 0, 1, p(depth), p(panels), p(points), p(offsets), p(ws), need,
                                 ea._lib.stream())

    def posed(thr=0):
        return lib.endo_evaluate_posed(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(rot), p(tr), n, h, w, 0, 1, thr, 100.0, 150.0, p(depth),
                                       p(color_images), p(depth_images), p(points), p(offsets), p(ranges), p(ws), need_posed,
                                       ea._lib.stream())
    print()
    for label, fn in (("endo_evaluate", plain), ("endo_evaluate_posed", posed), ("endo_evaluate_posed, thresholds", lambda: posed(1)),
                      ("endo_evaluate", plain), ("endo_evaluate_posed", posed)):
        print("%s N=%d %dx%d: %.1f us per batch (500 back-to-back calls)" % (label, n, h, w, per_call_us(fn)))
    model, _ = trained
    folder = os.path.join(str(tmp_path), "bag_1", SEQ_NAME)
    shutil.copytree(sequence, folder)
    frames_src = [os.path.join(folder, f) for f in ("00004584.jpg", "00004594.jpg")]
    names = []
    for i in range(64):
        names.append(os.path.join(folder, "%08d.jpg" % (20000 + i)))
        shutil.copyfile(frames_src[i % 2], names[-1])
    rots, trs = random_poses(64, 3)
    rotations = {os.path.basename(name)[:8]: rots[i] for i, name in enumerate(names)}
    translations = {os.path.basename(name)[:8]: trs[i] for i, name in enumerate(names)}
    frames = ea.dataset.TestFrames(names, batch_size=8, suggested_h=256, suggested_w=320)
    evaluate.run_test_phase(model, frames, tmp_path / "warm")
    evaluate.run_posed_test_phase(model, frames, translations, rotations, tmp_path / "warm_posed")
    for label, posed_kw, plain_kw in (("no files", dict(write_images=False, write_ply=False), dict(write_png=False, write_ply=False)),
                                      ("png + text ply (+ merged)", {}, {}),
                                      ("png + binary ply (+ merged)", dict(ply_text=False), dict(ply_text=False)),
                                      ("no files", dict(write_images=False, write_ply=False), dict(write_png=False, write_ply=False))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = evaluate.run_test_phase(model, frames, tmp_path / "run", **plain_kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        result = evaluate.run_posed_test_phase(model, frames, translations, rotations, tmp_path / "run_posed", **posed_kw)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert result["frames"] == count == 64 and not result["zero_range"] and not result["empty"]
        print("batch 8, 256x320, %s: run_test_phase %.1f frames/s, run_posed_test_phase %.1f frames/s" % (
            label, count / (t1 - t0), count / (t2 - t1)))
    assert np.isfinite(ranges.cpu().numpy()).all()
