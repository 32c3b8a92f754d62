"""Timing prints of the test phase (evaluate.py's counterpart): run by hand with ``pytest -m bench`` on an MI355X; nothing is asserted about
speed."""

import os
import shutil
import time

import pytest
import torch

from test_gpu_evaluate import SEQ_NAME, dev, ea, evaluate, random_batch, sequence, trained  # noqa: F401 -- the last two are fixtures

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]


def test_bench_test_phase(sequence, trained, tmp_path):
    """GPU time of endo_evaluate per batch (N = 8, 256 x 320), and run_test_phase frames/s at batch size 8 with and without writing the
    files (64 frames: copies of the example sequence's two).  Prints only; nothing is asserted about speed."""
    n, h, w = 8, 256, 320
    t = [torch.from_numpy(a).to(dev()) for a in random_batch(n, h, w, seed=1)]
    lib = ea._lib.load()
    need = int(lib.endo_evaluate_workspace_bytes(n, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    depth = torch.empty((n, 1, h, w), device=dev())
    panels = torch.empty((n, h, 2 * w, 3), dtype=torch.uint8, device=dev())
    points = torch.empty((n * h * w, 6), device=dev())
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev())
    p = ea._lib.ptr

    def launch():
        return lib.endo_evaluate(p(t[0]), p(t[1]), p(t[2]), p(t[3]), n, h, w, 0, 1, p(depth), p(panels), p(points), p(offsets), p(ws), need,
                                 ea._lib.stream())
    for _ in range(10):
        assert launch() == 0
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 500
    start.record()
    for _ in range(reps):
        launch()
    stop.record()
    stop.synchronize()
    print("\nendo_evaluate N=%d %dx%d: %.1f us per batch (%d back-to-back launches)" % (n, h, w, 1000.0 * start.elapsed_time(stop) / reps, reps))
    model, _ = trained
    folder = os.path.join(str(tmp_path), "bag_1", SEQ_NAME)
    shutil.copytree(sequence, folder)
    frames_src = [os.path.join(folder, f) for f in ("00004584.jpg", "00004594.jpg")]
    names = []
    for i in range(64):
        names.append(os.path.join(folder, "%08d.jpg" % (20000 + i)))
        shutil.copyfile(frames_src[i % 2], names[-1])
    frames = ea.dataset.TestFrames(names, batch_size=8, suggested_h=256, suggested_w=320)
    evaluate.run_test_phase(model, frames, tmp_path / "warm")
    for label, kw in (("no files", dict(write_png=False, write_ply=False)), ("png + text ply", {}), ("png + binary ply", dict(ply_text=False)),
                      ("no files", dict(write_png=False, write_ply=False))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = evaluate.run_test_phase(model, frames, tmp_path / "run", **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("run_test_phase, batch 8, 256x320, %s: %d frames in %.3f s = %.1f frames/s" % (label, count, dt, count / dt))
