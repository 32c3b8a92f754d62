"""Timing prints of the volume renderer: run by hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""
import importlib

import numpy as np
import pytest
import torch

from test_bench_fusion import H, N, RES, VS, W, frames
from test_bench_registration import device_ms

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion = ea.fusion


def test_bench_render():
    """Device time per render of 8 frames of 256 x 320 from 256^3 voxels integrated from the posed arc, from the frames' own poses, with
    and without the empty-space marks; the share of the in-grid samples that lie in unmarked bricks (counted in torch on the same rays'
    sample grid, every 16th pixel); integrate in the same job for scale.  Prints only."""
    inputs = frames("arc")
    volume = fusion.TSDFVolume((-0.5 * RES * VS,) * 3, VS, (RES, RES, RES), device="cuda:0")
    scales = torch.ones(N, device="cuda:0")
    assert volume.integrate(*inputs, scales=scales) == ["ok"] * N
    ms_integrate = device_ms(lambda: volume.integrate(*inputs, scales=scales), window_ms=100.0)
    volume.clear()
    volume.integrate(*inputs, scales=scales)
    k, rotations, translations = inputs[3], inputs[4], inputs[5]
    out = {}
    ms = {}
    for skip in (True, False):
        out[skip] = volume.render(k, rotations, translations, H, W, scales=scales, skip=skip)
        ms[skip] = device_ms(lambda: volume.render(k, rotations, translations, H, W, scales=scales, skip=skip), window_ms=200.0)
    for name in out[True]:
        assert torch.equal(out[True][name], out[False][name]), name
    hits = int(out[True]["mask"].sum())

    # the share of in-grid samples in unmarked bricks, on the sample grid of every 16th pixel (fp32 in torch: a count, not a contract)
    b = fusion.RENDER_BRICK[0]
    pad = torch.nn.functional.pad(((volume.weight >= 1.0) & (volume.tsdf <= 0)).float()[None, None], (0, 1, 0, 1, 0, 1))
    marks = torch.nn.functional.max_pool3d(pad, kernel_size=b + 1, stride=b)[0, 0] > 0
    inside_total, skipped_total = 0, 0
    kk = np.asarray(k.cpu())
    for f in range(N):
        v, u = torch.meshgrid(torch.arange(0, H, 4, device="cuda:0", dtype=torch.float32),
                              torch.arange(0, W, 4, device="cuda:0", dtype=torch.float32), indexing="ij")
        d = torch.stack([(u - float(kk[f, 0, 2])) / float(kk[f, 0, 0]), (v - float(kk[f, 1, 2])) / float(kk[f, 1, 1]), torch.ones_like(u)], dim=-1)
        step = 0.5 * VS / d.norm(dim=-1, keepdim=True)
        w = d @ torch.from_numpy(rotations[f].T).float().cuda()
        t0 = torch.from_numpy(translations[f]).float().cuda()
        for chunk in range(0, 1200, 100):
            ks = torch.arange(chunk + 1, chunk + 101, device="cuda:0", dtype=torch.float32)
            x = t0 + (ks[:, None, None, None] * step[None]) * w[None]
            g = torch.floor((x + 0.5 * RES * VS) / VS - 0.5).long()
            inside = ((g >= 0) & (g <= RES - 2)).all(dim=-1)
            gi = g.clamp(0, RES - 2) // b
            marked = marks[gi[..., 2], gi[..., 1], gi[..., 0]]
            inside_total += int(inside.sum())
            skipped_total += int((inside & ~marked).sum())
    share = skipped_total / max(1, inside_total)
    rays = N * H * W
    print()
    print("endo_fusion_render arc: 8 x %d x %d rays through %d^3 at step 0.5: %.3f ms per call with the marks (2 launches), %.3f ms without "
          "(%.2fx); %d of %d rays hit; %.1f %% of the in-grid samples lie in unmarked bricks (%.0f in-grid samples per ray); "
          "integrate of the same 8 frames: %.3f ms" % (H, W, RES, ms[True], ms[False], ms[False] / ms[True], hits, rays, 100.0 * share,
                                                        16.0 * inside_total / rays, ms_integrate))
    assert torch.isfinite(out[True]["depth"]).all()
