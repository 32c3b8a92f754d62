"""Timing prints of the six loss modules that finish the reference's losses.py, next to NormalizedDistanceLoss from the same job: run by
hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""

import importlib

import pytest
import torch

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")


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


def test_bench_losses_extra():
    """Device time per call (N = 8, 256 x 320; 500 back-to-back calls between two events) of each new entry point, forward (memset, reduce,
    finalize) and backward (one elementwise kernel, both gradients), with the bytes the algorithm moves."""
    n, h, w = 8, 256, 320
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    lib, p, s = ea._lib.load(), ea._lib.ptr, ea._lib.stream()
    mask = (rand(n, 1, h, w) < 0.6).float()
    depth = 0.3 + 0.6 * rand(n, 1, h, w)
    warped = depth * (0.8 + 0.45 * rand(n, 1, h, w))
    smask = (rand(n, 1, h, w) < 0.05).float()
    sparse = (0.6 + 7.4 * rand(n, 1, h, w)) * smask
    est = 0.5 + 7.5 * rand(n, 1, h, w)
    images, images_hat = rand(n, 3, h, w), rand(n, 3, h, w)
    flows, flows_hat = rand(n, 2, h, w), rand(n, 2, h, w)
    trans = torch.randn(n, 3, device=dev, generator=gen)
    k = ea.synthetic.make_batch(n, h, w, seed=1, sparse_points=100)["intrinsics"].to(dev).reshape(n, 9).contiguous()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    stats = torch.empty((n, 4), dtype=torch.float64, device=dev)
    gone, gvec = torch.ones((), device=dev), torch.ones(n, device=dev)
    g1, g3a, g3b, g2a, g2b = (torch.empty_like(t) for t in (depth, images, images_hat, flows, flows_hat))
    g1b = torch.empty_like(depth)
    hw, eps = h * w, 1.0e-3
    triple = [p(depth), p(warped), p(mask)]
    # name -> (forward launch, floats read per pixel forward, backward launch, floats moved per pixel backward)
    rows = [
        ("NormalizedDistanceLoss (for scale)",
         lambda: lib.endo_norm_dist_fwd(*triple, p(k), p(loss), p(stats), n, h, w, 1e-5, s), 3,
         lambda: lib.endo_norm_dist_bwd(p(gone), *triple, p(k), p(stats), p(g1), p(g1b), n, h, w, 1e-5, s), 5),
        ("NormalizedL2Loss",
         lambda: lib.endo_norm_l2_fwd(*triple, p(loss), p(stats), n, hw, eps, s), 3,
         lambda: lib.endo_norm_l2_bwd(p(gone), *triple, p(stats), p(g1), p(g1b), n, hw, eps, s), 5),
        ("NormalizedL1Loss",
         lambda: lib.endo_norm_l1_fwd(*triple, p(loss), p(stats), n, hw, eps, s), 3,
         lambda: lib.endo_norm_l1_bwd(p(gone), *triple, p(stats), p(g1), p(g1b), n, hw, eps, s), 5),
        ("NormalizedWeightedMaskedL2Loss",
         lambda: lib.endo_weighted_l2_fwd(*triple, p(trans), p(loss), p(stats), n, hw, 1.0, s), 3,
         lambda: lib.endo_weighted_l2_bwd(p(gone), *triple, p(stats), p(g1), p(g1b), n, hw, 1.0, s), 5),
        ("MaskedScaleInvariantLoss",
         lambda: lib.endo_masked_scale_inv_fwd(p(est), p(sparse), p(smask), p(loss), p(stats), n, hw, 1e-8, s), 3,
         lambda: lib.endo_masked_scale_inv_bwd(p(gone), p(est), p(sparse), p(smask), p(stats), p(g1), n, hw, 1e-8, s), 4),
        ("MaskedL1Loss (endo_sparse_l1_*, C = 3)",
         lambda: lib.endo_sparse_l1_fwd(p(images), p(images_hat), p(mask), p(loss), p(stats), n, 3, hw, 1.0, s), 7,
         lambda: lib.endo_sparse_l1_bwd(p(gone), p(images), p(images_hat), p(mask), p(stats), p(g3a), p(g3b), n, 3, hw, 1.0, s), 13),
        ("SparseMaskedL1LossDisplay (C = 2)",
         lambda: lib.endo_sparse_l1_display_fwd(p(flows), p(flows_hat), p(smask), p(out), p(stats), n, 2, hw, 1.0, s), 5,
         lambda: lib.endo_sparse_l1_display_bwd(p(gvec), p(flows), p(flows_hat), p(smask), p(stats), p(g2a), p(g2b), n, 2, hw, 1.0, s), 9),
    ]
    print("\nloss entry points, N=%d %dx%d, device us per call over 500 back-to-back calls (MB moved -> GB/s)" % (n, h, w))
    for name, fwd, fwd_floats, bwd, bwd_floats in rows:
        us_f = _events(fwd)          # the forward leaves `stats` as the backward reads it
        us_b = _events(bwd)
        mb_f, mb_b = 4e-6 * fwd_floats * n * hw, 4e-6 * bwd_floats * n * hw
        print("%-40s forward %6.1f us (%5.1f MB -> %5.0f GB/s)   backward %6.1f us (%5.1f MB -> %5.0f GB/s)" % (
            name, us_f, mb_f, 1e3 * mb_f / us_f, us_b, mb_b, 1e3 * mb_b / us_b))
