"""Timing prints of evaluate.py's validation phase (evaluate.py:119-277): run by hand with ``pytest -m bench`` on an MI355X; nothing is
asserted about speed."""

import time

import pytest
import torch

from oracle import network as onet
from test_gpu_evaluate_validation import PANEL_KEYS, dev, ea, validation_inputs

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]


def _events(launch, reps=500):
    for _ in range(10):
        assert launch() == 0
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        launch()
    stop.record()
    stop.synchronize()
    return 1000.0 * start.elapsed_time(stop) / reps


def test_bench_evaluate_validation():
    """GPU time of endo_evaluate_validation per batch (N = 8, 256 x 320) over 500 back-to-back calls, timed by events, with endo_display
    in the same job for scale."""
    n, h, w = 8, 256, 320
    x = validation_inputs(n, h, w, seed=1)
    t = [torch.from_numpy(x[k]).to(dev()) for k in PANEL_KEYS]
    lib = ea._lib.load()
    p = ea._lib.ptr
    need = int(lib.endo_evaluate_validation_workspace_bytes(n, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    panel = torch.empty(ea.display.validation_panel_shape(n, h, w), dtype=torch.uint8, device=dev())
    metrics = torch.empty((n, 2, 4), dtype=torch.float32, device=dev())
    points = torch.empty((n * h * w, 6), dtype=torch.float32, device=dev())
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev())
    us = _events(lambda: lib.endo_evaluate_validation(*[p(a) for a in t], n, h, w, 1e-8, 0, 1, p(panel), p(metrics), p(points), p(offsets),
                                                      p(ws), need, ea._lib.stream()))
    rows = int(offsets[-1])
    # floats read per pixel: reduce 4 + 3 per half; write 12 per half and 5 for the point rows; written: the panel and the point rows
    moved = n * h * w * 4 * (2 * 7 + 2 * 12 + 5) + panel.numel() + rows * 24
    print("\nendo_evaluate_validation N=%d %dx%d: %.1f us per batch (500 back-to-back calls), %.1f MB algorithmic -> %.0f GB/s" % (
        n, h, w, us, moved / 1e6, moved / us / 1e3))
    d = [t[i] for i in (0, 1, 3, 4, 2, 11, 12, 13, 14)]
    need_d = int(lib.endo_display_workspace_bytes(n, h, w))
    ws_d = torch.empty(need_d, dtype=torch.uint8, device=dev())
    out_d = torch.empty(ea.display.panel_shape(n, h, w), dtype=torch.uint8, device=dev())
    us_d = _events(lambda: lib.endo_display(*[p(a) for a in d], n, h, w, p(out_d), p(ws_d), need_d, ea._lib.stream()))
    moved_d = 2 * n * h * w * 4 * 13 + out_d.numel()
    print("endo_display (for scale): %.1f us per batch, %.1f MB algorithmic -> %.0f GB/s" % (us_d, moved_d / 1e6, moved_d / us_d / 1e3))
    m = [t[3], t[5], t[7]]
    out_m = torch.empty((n, 4), dtype=torch.float32, device=dev())
    us_m = _events(lambda: lib.endo_depth_metrics(*[p(a) for a in m], n, h, w, 1e-8, p(out_m), ea._lib.stream()))
    print("endo_depth_metrics: %.1f us per batch, %.1f MB -> %.0f GB/s" % (us_m, n * h * w * 12 / 1e6, n * h * w * 12 / us_m / 1e3))


def test_bench_run_validation_phase(tmp_path):
    """Pairs/s of run_validation_phase over 16 synthetic batches at 8 x 256 x 320, with and without file writing."""
    n, h, w = 8, 256, 320
    batches = [{k: v.to(dev()) for k, v in ea.synthetic.make_batch(n, h, w, seed=60 + i, sparse_points=2000).items()} for i in range(16)]
    state = onet.keep_depth_positive(onet.perturb_affine(onet.synthetic_state(7), 8))
    model = ea.FCDenseNet57(1)
    model.load_state_dict(state)
    model = model.to(dev()).eval()
    for label, kw in (("no files", {"write_png": False, "write_ply": False}), ("PNG + text PLY of sample 0", {}),
                      ("PNG + binary PLY of every sample", {"ply_text": False, "all_samples": True})):
        ea.evaluate.run_validation_phase(model, batches[:2], tmp_path / "warm", **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ea.evaluate.run_validation_phase(model, batches, tmp_path / label.replace(" ", "_"), **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("\nrun_validation_phase, %s: %d pairs in %.1f ms = %.1f pairs/s" % (label, res["pairs"], 1000 * dt, res["pairs"] / dt))
