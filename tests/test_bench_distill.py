"""Timing prints of the distillation head and step: endo_distill_head in both modes next to the chain of the four endo_scale_inv_*
calls it replaces, and one DistillationStep call (pure mode) next to one TrainingStep call, from the same job: run by hand with
``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""

import importlib

import pytest
import torch

from oracle import network as onet

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


def _network(seed, dev, train):
    model = ea.FCDenseNet57(1)
    model.load_state_dict(onet.keep_depth_positive(onet.perturb_affine(onet.synthetic_state(seed), seed + 1)))
    model = model.to(dev)
    return model.train() if train else model.eval()


def test_bench_distill_head():
    """Device time per call (N = 8, 256 x 320; 500 back-to-back calls between two events).  The chain is what a caller without the entry
    runs after the two torch.abs: endo_scale_inv_fwd and endo_scale_inv_bwd per frame (two memsets and six launches); the fused entry is
    one memset and two launches for both frames."""
    n, h, w = 8, 256, 320
    dev = torch.device("cuda:0")
    lib, p, s = ea._lib.load(), ea._lib.ptr, ea._lib.stream()
    mask = ea.synthetic.make_batch(n, h, w, seed=1, sparse_points=10)["boundaries"].to(dev).contiguous()
    pred = [ea.synthetic.smooth_depth(n, h, w, seed=2 + i).to(dev).contiguous() for i in range(2)]
    goal = [ea.synthetic.smooth_depth(n, h, w, seed=4 + i, lo=0.2, hi=1.4).to(dev).contiguous() for i in range(2)]
    grad = [torch.zeros_like(t) for t in pred]
    loss, up = torch.empty(2, device=dev), torch.full((1,), 0.5, device=dev)
    stats = torch.empty(2, 3 * n, dtype=torch.float64, device=dev)
    losses = torch.zeros(5, device=dev)

    def chain():
        rc = 0
        for i in range(2):
            rc |= lib.endo_scale_inv_fwd(p(pred[i]), p(goal[i]), p(mask), p(loss[i:]), p(stats[i]), n, h * w, 1.0e-8, s)
            rc |= lib.endo_scale_inv_bwd(p(up), p(pred[i]), p(goal[i]), p(mask), p(stats[i]), p(grad[i]), None, n, h * w, 1.0e-8, s)
        return rc

    head = lambda acc: lib.endo_distill_head(p(pred[0]), p(pred[1]), p(goal[0]), p(goal[1]), p(mask), 1.0, 1.0e-8, acc, p(losses),
                                             p(grad[0]), p(grad[1]), p(stats), n, h * w, s)
    mb = 4e-6 * n * h * w
    print("\ndistillation head, both frames, N=%d %dx%d, device us per call over 500 back-to-back calls (MB moved -> GB/s)" % (n, h, w))
    rows = (("endo_scale_inv_fwd + _bwd, twice (the chain)", chain, 2 * (3 + 4)),
            ("endo_distill_head, accumulate = 0", lambda: head(0), 2 * (3 + 4) - 2),          # the boundary is shared by both frames' rows in L2, not in HBM traffic counted here
            ("endo_distill_head, accumulate = 1", lambda: head(1), 2 * (3 + 5) - 2))
    for name, launch, planes in rows:
        us = _events(launch)
        print("%-46s %6.1f us (%5.1f MB -> %5.0f GB/s)" % (name, us, planes * mb, 1e3 * planes * mb / us))
        if name.endswith("= 1"):
            grad[0].zero_()
            grad[1].zero_()


def test_bench_distillation_step():
    """Wall time per iteration, N = 8, 256 x 320: DistillationStep in pure mode (teacher forward + student forward + head + student backward
    + optimizer) next to TrainingStep (one forward + loss head + backward + optimizer); 3 warm-up and 10 timed calls each, one sync."""
    import time
    n, h, w = 8, 256, 320
    dev = torch.device("cuda:0")
    batch = {k: v.to(dev).contiguous() for k, v in ea.synthetic.make_batch(n, h, w, seed=1, sparse_points=500).items()}
    student, teacher, plain = _network(4, dev, True), _network(24, dev, False), _network(4, dev, True)
    steps = (("DistillationStep, pure mode", ea.train_step.DistillationStep(student, teacher, ea.optim.FusedClipSGD(student, lr=1.0e-4), h, w)),
             ("TrainingStep", ea.train_step.TrainingStep(plain, ea.optim.FusedClipSGD(plain, lr=1.0e-4), h, w)))
    print("\none training iteration, N=%d %dx%d, wall ms per call over 10 calls" % (n, h, w))
    for name, step in steps:
        for _ in range(3):
            out = step(batch)
        assert out["skipped"] is False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            out = step(batch)
        torch.cuda.synchronize()
        print("%-30s %7.2f ms   (loss %.5f)" % (name, 100.0 * (time.perf_counter() - t0), out["loss"]))
