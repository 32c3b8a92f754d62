"""Timing prints of the image-warping entry points (endo_warp_coordinates_*, endo_image_warp_*), next to the depth warp and the flow
layer from the same job: run by hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""

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


def test_bench_image_warp():
    """Device time per call (N = 8, C = 3, 256 x 320; 500 back-to-back calls between two events) with the bytes the algorithm moves:
    planes read or written once, a 4-tap gather counted as one read of the plane (the taps of neighbouring pixels share lines), the
    image gradient's memset and scatter as one write and one read-modify-write of the planes.  The coordinates are the coordinate
    call's for a synthetic pair, so every masked-out pixel samples at (0, 0): with the cotangent of a loss under the mask those pixels
    scatter nothing; the "unmasked" row gives them a cotangent, and their atomics then meet on one pixel per plane."""
    n, c, h, w = 8, 3, 256, 320
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    lib, p, s = ea._lib.load(), ea._lib.ptr, ea._lib.stream()
    batch = ea.synthetic.make_batch(n, h, w, seed=1, sparse_points=100)
    mask = batch["boundaries"].to(dev).contiguous()
    t = batch["translations_1_wrt_2"].to(dev).reshape(n, 3).contiguous()
    r = batch["rotations_1_wrt_2"].to(dev).reshape(n, 9).contiguous()
    k = batch["intrinsics"].to(dev).reshape(n, 9).contiguous()
    d1 = ea.synthetic.smooth_depth(n, h, w, seed=2).to(dev).contiguous()
    d2 = ea.synthetic.smooth_depth(n, h, w, seed=3).to(dev).contiguous()
    images, cot = rand(n, c, h, w), rand(n, c, h, w)
    u, v, gd, gplane = (torch.empty(n, h, w, device=dev) for _ in range(4))
    gu, gv = torch.empty_like(u), torch.empty_like(v)
    warped, gimg = torch.empty_like(images), torch.empty_like(images)
    flow = torch.empty(n, 2, h, w, device=dev)
    wd, inter, g1, g2 = (torch.empty_like(d1) for _ in range(4))
    gplane.copy_(rand(n, h, w))
    gwd = cot[:, :1].contiguous()
    mcot = (cot * mask).contiguous()          # the cotangent of a loss under the boundary mask, as MaskedL1Loss hands it back
    pose = [p(t), p(r), p(k)]
    assert lib.endo_warp_coordinates_fwd(p(d1), p(mask), *pose, p(u), p(v), n, h, w, s) == 0          # the sampler's coordinates: a real warp
    # name -> (launch, planes of n * h * w floats moved)
    rows = [
        ("endo_warp_coordinates_fwd", lambda: lib.endo_warp_coordinates_fwd(p(d1), p(mask), *pose, p(u), p(v), n, h, w, s), 4),
        ("endo_warp_coordinates_bwd", lambda: lib.endo_warp_coordinates_bwd(p(gplane), p(gplane), p(d1), p(mask), *pose, p(gd), n, h, w, s), 5),
        ("endo_flow_from_depth_fwd (for scale)", lambda: lib.endo_flow_from_depth_fwd(p(d1), p(mask), *pose, p(flow), n, h, w, s), 4),
    ]
    for mode, name in enumerate(("zeros", "border", "reflection")):
        rows.append(("endo_image_warp_fwd %s" % name,
                     lambda mode=mode: lib.endo_image_warp_fwd(p(images), p(u), p(v), p(warped), n, c, h, w, mode, s), 2 + 2 * c))
    rows += [
        ("endo_image_warp_bwd zeros, all gradients",
         lambda: lib.endo_image_warp_bwd(p(mcot), p(images), p(u), p(v), p(gimg), p(gu), p(gv), n, c, h, w, 0, s), 4 + 5 * c),
        ("endo_image_warp_bwd zeros, images only",
         lambda: lib.endo_image_warp_bwd(p(mcot), p(images), p(u), p(v), p(gimg), None, None, n, c, h, w, 0, s), 2 + 4 * c),
        ("endo_image_warp_bwd zeros, all, unmasked cot.",
         lambda: lib.endo_image_warp_bwd(p(cot), p(images), p(u), p(v), p(gimg), p(gu), p(gv), n, c, h, w, 0, s), 4 + 5 * c),
        ("endo_image_warp_bwd zeros, coordinates only",
         lambda: lib.endo_image_warp_bwd(p(cot), p(images), p(u), p(v), None, p(gu), p(gv), n, c, h, w, 0, s), 4 + 2 * c),
        ("endo_depth_warp_fwd (for scale)",
         lambda: lib.endo_depth_warp_fwd(p(d1), p(d2), p(mask), *pose, p(wd), p(inter), n, h, w, 1e-8, s), 5),
        ("endo_depth_warp_bwd (for scale)",
         lambda: lib.endo_depth_warp_bwd(p(gwd), p(d1), p(d2), p(mask), *pose, p(g1), p(g2), n, h, w, 1e-8, s), 7),
        ("endo_depth_warp_fwd_tiled 0 x 0: its gather form",
         lambda: lib.endo_depth_warp_fwd_tiled(p(d1), p(d2), p(mask), *pose, p(wd), p(inter), n, h, w, 1e-8, 0, 0, s), 5),
        ("endo_depth_warp_bwd_tiled 0 x 0: its gather form",
         lambda: lib.endo_depth_warp_bwd_tiled(p(gwd), p(d1), p(d2), p(mask), *pose, p(g1), p(g2), n, h, w, 1e-8, 0, 0, s), 7),
    ]
    print("\nimage warping entry points, N=%d C=%d %dx%d, device us per call over 500 back-to-back calls (MB moved -> GB/s)" % (n, c, h, w))
    for name, launch, planes in rows:
        us = _events(launch)
        mb = 4e-6 * planes * n * h * w
        print("%-46s %6.1f us (%5.1f MB -> %5.0f GB/s)" % (name, us, mb, 1e3 * mb / us))
