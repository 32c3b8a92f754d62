"""Timing prints of the validation pass and the display panels (train.py:353-371, 375-492): run by hand with ``pytest -m bench`` on an
MI355X; nothing is asserted about speed."""

import time

import pytest
import torch

from oracle import network as onet
from test_gpu_validation import dev, display_inputs, ea, synthetic

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]


def test_bench_display():
    """GPU time of endo_display per batch (N = 8, 256 x 320) over 500 back-to-back calls, timed by events."""
    n, h, w = 8, 256, 320
    cols, depths, b, sparse, dense = display_inputs(n, h, w, seed=1)
    t = [torch.from_numpy(a).to(dev()) for a in (cols[0], cols[1], depths[0], depths[1], b, sparse[0], sparse[1], dense[0], dense[1])]
    lib = ea._lib.load()
    need = int(lib.endo_display_workspace_bytes(n, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    out = torch.empty(ea.display.panel_shape(n, h, w), dtype=torch.uint8, device=dev())
    p = ea._lib.ptr

    def launch():
        return lib.endo_display(*[p(a) for a in t], n, h, w, p(out), p(ws), need, ea._lib.stream())
    for _ in range(10):
        assert launch() == 0
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 500
    start.record()
    for _ in range(reps):
        launch()
    stop.record()
    stop.synchronize()
    us = 1000.0 * start.elapsed_time(stop) / reps
    moved = 2 * n * h * w * 4 * 13 + out.numel()
    print("\nendo_display N=%d %dx%d: %.1f us per batch (%d back-to-back launches), %.1f MB algorithmic -> %.0f GB/s" % (
        n, h, w, us, reps, moved / 1e6, moved / us / 1e3))


def _model(seed=7):
    state = onet.keep_depth_positive(onet.perturb_affine(onet.synthetic_state(seed), seed + 1))
    model = ea.FCDenseNet57(1)
    model.load_state_dict(state)
    return model.to(dev()).train()


def test_bench_validation_pass():
    """Validation pairs/s over 16 synthetic batches at 8 x 256 x 320: train_step.validate (fused pass, device means) against the module path
    (fused_head=False: losses() under no_grad) with the reference's per-batch loss.item() reads."""
    n, h, w = 8, 256, 320
    batches = [{k: v.to(dev()) for k, v in synthetic.make_batch(n, h, w, seed=60 + i, sparse_points=2000).items()} for i in range(16)]
    model = _model()
    fused = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1e-4), h, w)
    modular = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1e-4), h, w, fused_head=False)

    def fused_pass():
        return ea.train_step.validate(fused, batches)

    def module_pass():
        means = [0.0, 0.0, 0.0]
        for i, batch in enumerate(batches):
            vals = modular.validation_losses(batch)[:3].tolist()          # the reference's loss.item() per batch
            means = vals if i == 0 else [(m * i + v) / (i + 1.0) for m, v in zip(means, vals)]
        return means
    for label, fn in (("fused", fused_pass), ("module path", module_pass)):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 3
        print("\nvalidation, %s: 16 batches of %d pairs at %dx%d in %.1f ms = %.1f pairs/s" % (label, n, h, w, 1000 * dt, 16 * n / dt))


def test_bench_display_in_training():
    """What display_panels() at display_each = 10 costs inside a training loop (8 x 256 x 320): 40 steps with and without it."""
    n, h, w = 8, 256, 320
    batches = [{k: v.to(dev()) for k, v in synthetic.make_batch(n, h, w, seed=80 + i, sparse_points=2000).items()} for i in range(4)]
    model = _model(9)
    step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1e-5), h, w)
    kept = []
    for display_each in (None, 10, None, 10):
        kept.clear()
        step(batches[0])["loss"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prev = None
        for i in range(40):
            out = step(batches[i % 4])
            if display_each is not None and i % display_each == 0:
                kept.append(step.display_panels())
            if prev is not None:
                prev["loss"]
            prev = out
        prev["loss"]
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 40
        print("\ntraining 8x256x320, display_each=%s: %.3f ms per step (%d panels)" % (display_each, 1000 * dt, len(kept)))
