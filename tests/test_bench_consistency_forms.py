"""Timing prints of the consistency-loss choice: endo_warp_consistency_forms per form next to the module chain it replaces
(DepthWarpingLayer -> loss module under autograd, both directions), and one TrainingStep per form, from the same job: run by hand
with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""

import importlib
import time

import pytest
import torch

import consistency_forms_restate as cr

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")


def _events(launch, reps):
    for _ in range(10):
        launch()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        launch()
    stop.record()
    stop.synchronize()
    return 1000.0 * start.elapsed_time(stop) / reps


def test_bench_warp_consistency_forms():
    """Device time per call at N = 8, 256 x 320 between two events: 500 back-to-back fused calls; 100 of the module chain (its time
    includes the gaps between its ~10 autograd nodes' launches, which is what a caller of the modules pays)."""
    n, h, w = 8, 256, 320
    dev = torch.device("cuda:0")
    db = {k: v.to(dev).contiguous() for k, v in ea.synthetic.make_batch(n, h, w, seed=1, sparse_points=500).items()}
    d1 = ea.synthetic.smooth_depth(n, h, w, seed=2).to(dev).contiguous()
    d2 = ea.synthetic.smooth_depth(n, h, w, seed=3).to(dev).contiguous()
    p12 = [db["translations_1_wrt_2"], db["rotations_1_wrt_2"], db["intrinsics"]]
    p21 = [db["translations_2_wrt_1"], db["rotations_2_wrt_1"], db["intrinsics"]]
    warp = ea.DepthWarpingLayer()
    print("\ndepth warp both ways + consistency loss, forward and backward, N=%d %dx%d, device us per call" % (n, h, w))
    for form in cr.FORMS:
        module = ea.train_step.consistency_loss_spec(form, h, w)[1]
        fourth = {"distance": ([db["intrinsics"]], [db["intrinsics"]]), "weighted_l2": ([p12[0]], [p21[0]])}.get(form, ([], []))

        def fused():
            ea.losses.warp_consistency(d1, d2, db["boundaries"], p12[0], p12[1], p21[0], p21[1], db["intrinsics"], form=form)

        def chain():
            g1, g2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
            w21, i1 = warp([g1, g2, db["boundaries"]] + p12)
            w12, i2 = warp([g2, g1, db["boundaries"]] + p21)
            (0.5 * (module([g1, w21, i1] + fourth[0]) + module([g2, w12, i2] + fourth[1]))).backward()

        t_fused, t_chain = _events(fused, 500), _events(chain, 100)
        print("%-12s fused %6.1f us (%.4f ms per pair)   module chain %7.1f us" % (form, t_fused, 1e-3 * t_fused / n, t_chain))


def test_bench_training_step_per_form():
    """Wall time of TrainingStep per form at the benchmark batch (8 x 256 x 320, fp32): 10 steps after 3, ended by a synchronise."""
    n, h, w = 8, 256, 320
    dev = torch.device("cuda:0")
    batch = {k: v.to(dev) for k, v in ea.synthetic.make_batch(n, h, w, seed=1, sparse_points=500).items()}
    print("\nTrainingStep, N=%d %dx%d, fp32, ms per step" % (n, h, w))
    for form in cr.FORMS:
        model = ea.FCDenseNet57(n_classes=1).to(dev).train()
        step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-4), h, w, consistency_loss=form)
        for _ in range(3):
            step(batch, lr=1.0e-4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            out = step(batch, lr=1.0e-4)
        torch.cuda.synchronize()
        print("%-12s %7.3f ms per step (loss %.5f)" % (form, 100.0 * (time.perf_counter() - t0), out["loss"]))
