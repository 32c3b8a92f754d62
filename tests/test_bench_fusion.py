"""Timing prints of the TSDF fusion: run by hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""
import importlib

import numpy as np
import pytest
import torch

import fusion_restate as fr
from test_bench_registration import device_ms

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion = ea.fusion

HBM_BYTES_PER_S = 6.3e12          # achievable on an MI355X (float4 copy)
N, H, W, RES = 8, 256, 320, 256
VS = 0.25


def frames(kind):
    """Eight 256 x 320 frames of a sphere-like wall around a 64-unit volume: ``all``: every camera sees the whole volume from far
    away; ``arc``: cameras inside the volume on a circle, each looking through the centre at about a tenth of it."""
    k = fr.intrinsics(260.0, H, W)
    rng = np.random.default_rng(5)
    if kind == "all":
        rotations = [fr.rotation_about((0, 1, 0), 2.0 * i - 7.0) for i in range(N)]
        translations = [np.array([0.5 * i - 2.0, 0.0, -120.0]) for i in range(N)]
        depth = np.full((N, H, W), 120.0, np.float32) + rng.uniform(-20.0, 20.0, (N, H, W)).astype(np.float32)
    else:
        rotations = [fr.rotation_about((0, 1, 0), 40.0 * i) for i in range(N)]
        translations = [rot @ np.array([0.0, 0.0, -12.0]) for rot in rotations]
        depth = np.full((N, H, W), 40.0, np.float32) + rng.uniform(-2.0, 2.0, (N, H, W)).astype(np.float32)
    d = torch.device("cuda:0")
    colors = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(d)
    return (torch.from_numpy(depth).to(d), torch.ones((N, H, W), device=d), colors, torch.from_numpy(np.stack([k] * N)).to(d),
            np.stack(rotations), np.stack(translations))


def torch_integrate(tsdf, weight, color, centres, depth, mask, colors, k, rotations, translations, trunc, max_weight):
    """The same update in plain torch, frame by frame over the whole volume."""
    n, h, w = depth.shape
    for f in range(n):
        p = (centres - translations[f]) @ rotations[f]
        u = torch.round(k[f, 0, 0] * (p[..., 0] / p[..., 2]) + k[f, 0, 2])
        v = torch.round(k[f, 1, 1] * (p[..., 1] / p[..., 2]) + k[f, 1, 2])
        valid = (p[..., 2] > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
        pix = torch.where(valid, v * w + u, torch.zeros_like(u)).long()
        z = depth[f].reshape(-1)[pix]
        sdf = z - p[..., 2]
        valid &= (mask[f].reshape(-1)[pix] > 0.5) & torch.isfinite(z) & (z > 0) & (sdf >= -trunc)
        val = torch.clamp(sdf / trunc, max=1.0)
        w1 = weight + 1.0
        tsdf.copy_(torch.where(valid, (tsdf * weight + val) / w1, tsdf))
        for c in range(3):
            sample = colors[f].reshape(-1, 3)[pix, c].float()
            color[c].copy_(torch.where(valid, (color[c] * weight + sample) / w1, color[c]))
        weight.copy_(torch.where(valid, torch.clamp(w1, max=max_weight), weight))


@pytest.mark.parametrize("kind", ["all", "arc"])
def test_bench_integrate(kind):
    """Device time per integrate of 8 frames of 256 x 320 into 256^3 voxels, the bytes the launch moves by its own arithmetic (40 per
    voxel of every wave box that is loaded and stored, the frames once) and the fraction of achievable HBM bandwidth that is; extract;
    and the same update in plain torch in the same job.  Prints only."""
    inputs = frames(kind)
    volume = fusion.TSDFVolume((-0.5 * RES * VS,) * 3, VS, (RES, RES, RES), device="cuda:0")
    scales = torch.ones(N, device="cuda:0")
    flags = volume.integrate(*inputs, scales=scales)
    assert flags == ["ok"] * N
    bx, by, bz = fusion.WAVE_BOX
    boxes = volume.weight.reshape(RES // bz, bz, RES // by, by, RES // bx, bx).amax(dim=(1, 3, 5))
    touched = int((boxes > 0).sum())
    fraction = touched / float(boxes.numel())
    moved = touched * bx * by * bz * 40.0 + N * H * W * 11.0
    lib = ea._lib.load()
    need = int(lib.endo_fusion_workspace_bytes(N, H, W))
    workspace = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    flags_dev = torch.empty(N, dtype=torch.int32, device="cuda:0")
    rot, tr = ea.evaluate._poses_f64(inputs[4], inputs[5], N, volume.device)
    origin = fusion._host_doubles(volume.origin)

    def launch(options):
        ea._lib.check(lib.endo_fusion_integrate(ea._lib.ptr(inputs[0]), ea._lib.ptr(inputs[1]), ea._lib.ptr(inputs[2]), ea._lib.ptr(inputs[3]),
                                                ea._lib.ptr(rot), ea._lib.ptr(tr), ea._lib.ptr(scales), N, H, W, origin, volume.voxel_size,
                                                volume.truncation, volume.max_weight, RES, RES, RES, ea._lib.ptr(volume.tsdf),
                                                ea._lib.ptr(volume.weight), ea._lib.ptr(volume.color), ea._lib.ptr(flags_dev), options,
                                                ea._lib.ptr(workspace), need, ea._lib.stream()), "endo_fusion_integrate")

    ms = device_ms(lambda: launch(0))
    ms_all = device_ms(lambda: launch(fusion.NO_CULL))
    ms_extract = device_ms(lambda: volume.extract(1.0), window_ms=100.0)
    rows = volume.extract(1.0).shape[0]
    # plain torch on the same data
    axis = (torch.arange(RES, device="cuda:0", dtype=torch.float32) + 0.5) * VS - 0.5 * RES * VS
    centres = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij")[::-1], dim=-1)
    k = inputs[3]
    rots = torch.from_numpy(inputs[4]).float().cuda()
    trs = torch.from_numpy(inputs[5]).float().cuda()
    plain = [torch.ones((RES,) * 3, device="cuda:0"), torch.zeros((RES,) * 3, device="cuda:0"), torch.zeros((3,) + (RES,) * 3, device="cuda:0")]
    ms_torch = device_ms(lambda: torch_integrate(plain[0], plain[1], plain[2], centres, inputs[0], inputs[1], inputs[2], k, rots, trs,
                                                 volume.truncation, volume.max_weight), window_ms=100.0)
    print()
    print("endo_fusion_integrate %s: 8 x %d x %d into %d^3: %.3f ms per call (%.3f ms without culling); %.0f %% of the wave boxes hold "
          "an observed voxel: %.1f MB by the kernel's arithmetic, %.0f %% of %.1f TB/s; extract (3 launches, one read, %d rows): %.3f ms; "
          "plain torch, same update: %.1f ms (%.0fx)" % (kind, H, W, RES, ms, ms_all, 100.0 * fraction, moved / 1e6,
                                                         100.0 * moved / (ms * 1e-3) / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12, rows,
                                                         ms_extract, ms_torch, ms_torch / ms))
    assert torch.isfinite(volume.tsdf).all()
