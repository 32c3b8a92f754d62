"""Timing prints of the frame-to-model tracker: run by hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""
import importlib
import time

import numpy as np
import pytest
import torch

import fusion_restate as fr
from test_bench_fusion import H, N, RES, VS, W, frames
from test_bench_registration import device_ms

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion = ea.fusion


def torch_sums(volume, depth, mask, k, rotations, translations, scales, min_weight):
    """The same 40 sums per frame with plain torch ops: fp32 per pixel (torch's own order of operations), fp64 products and sums."""
    nx, ny, nz = volume.dims
    origin = torch.tensor(volume.origin, dtype=torch.float32, device=depth.device)
    tsdf, weight = volume.tsdf.reshape(-1), volume.weight.reshape(-1)
    v, u = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float32), torch.arange(W, device=depth.device, dtype=torch.float32),
                          indexing="ij")
    upper = torch.triu_indices(7, 7, device=depth.device)
    out = []
    for f in range(depth.shape[0]):
        ray = torch.stack([(u - k[f, 0, 2]) / k[f, 0, 0], (v - k[f, 1, 2]) / k[f, 1, 1], torch.ones_like(u)], dim=-1).reshape(-1, 3)
        y = (scales[f] * depth[f].reshape(-1, 1)) * (ray @ rotations[f].T)
        g = (translations[f] + y - origin) / volume.voxel_size - 0.5
        base = torch.floor(g)
        r = g - base
        limit = torch.tensor([nx - 2, ny - 2, nz - 2], device=depth.device, dtype=torch.float32)
        ok = (mask[f].reshape(-1) > 0.5) & torch.isfinite(depth[f].reshape(-1)) & (depth[f].reshape(-1) > 0) & ((base >= 0) & (base <= limit)).all(dim=1)
        b = torch.where(ok[:, None], base, torch.zeros_like(base)).long()
        idx = (b[:, 2] * ny + b[:, 1]) * nx + b[:, 0]
        corner = [[[idx + (z * ny + yy) * nx + x for x in (0, 1)] for yy in (0, 1)] for z in (0, 1)]
        for z in (0, 1):
            for yy in (0, 1):
                for x in (0, 1):
                    ok &= weight[corner[z][yy][x]] >= min_weight
        t = [[[tsdf[corner[z][yy][x]] for x in (0, 1)] for yy in (0, 1)] for z in (0, 1)]
        d = [[t[z][yy][1] - t[z][yy][0] for yy in (0, 1)] for z in (0, 1)]
        a = [[t[z][yy][0] + r[:, 0] * d[z][yy] for yy in (0, 1)] for z in (0, 1)]
        e = [a[z][1] - a[z][0] for z in (0, 1)]
        bb = [a[z][0] + r[:, 1] * e[z] for z in (0, 1)]
        lerp = lambda p, q, w: p + w * (q - p)          # noqa: E731
        grad = torch.stack([lerp(lerp(d[0][0], d[0][1], r[:, 1]), lerp(d[1][0], d[1][1], r[:, 1]), r[:, 2]), lerp(e[0], e[1], r[:, 2]), bb[1] - bb[0]], dim=1)
        res = (bb[0] + r[:, 2] * grad[:, 2]) * volume.truncation
        nrm = grad * (volume.truncation / volume.voxel_size)
        j = torch.cat([torch.linalg.cross(y, nrm), nrm, (nrm * y).sum(dim=1, keepdim=True)], dim=1)[ok].double()
        rd = res[ok].double()
        jtj = j.T @ j
        out.append(torch.cat([torch.stack([ok.sum().double(), (rd * rd).sum(), rd.abs().sum(), rd.abs().max() if rd.numel() else rd.sum(),
                                           (y[ok].double() ** 2).sum()]), j.T @ rd, jtj[upper[0], upper[1]]]))
    return torch.stack(out)


def test_bench_track():
    """Device time per endo_fusion_track call on 8 frames of 256 x 320 against 256^3 voxels integrated from the posed arc, poses half a
    degree and a tenth of a unit off, with and without the per-pixel outputs; one residuals() with its read; a 5-iteration track();
    and the same sums with plain torch ops in the same job.  Prints only."""
    inputs = frames("arc")
    volume = fusion.TSDFVolume((-0.5 * RES * VS,) * 3, VS, (RES, RES, RES), device="cuda:0")
    scales = np.ones(N)
    assert volume.integrate(*inputs, scales=torch.ones(N, device="cuda:0")) == ["ok"] * N
    depth, mask, _, k, rotations, translations = inputs
    rng = np.random.default_rng(11)
    rotations = np.stack([fr.rotation_about(rng.normal(size=3), 0.5) @ r for r in rotations])
    translations = translations + rng.normal(size=(N, 3)) * 0.1
    lib = ea._lib.load()
    need = int(lib.endo_fusion_track_workspace_bytes(N, H, W))
    d = torch.device("cuda:0")
    rot_d, tr_d = torch.from_numpy(rotations).to(d), torch.from_numpy(translations).to(d)
    scales_d = torch.ones(N, device=d)
    workspace = torch.empty(need, dtype=torch.uint8, device=d)
    sums, flags = torch.empty((N, 40), dtype=torch.float64, device=d), torch.empty(N, dtype=torch.int32, device=d)
    maps = [torch.empty((N, H, W), device=d), torch.empty((N, H, W), device=d), torch.empty((N, H, W, 3), device=d)]
    origin = fusion._host_doubles(volume.origin)

    def launch(per_pixel):
        outs = [ea._lib.ptr(m) for m in maps] if per_pixel else [None, None, None]
        ea._lib.check(lib.endo_fusion_track(origin, volume.voxel_size, volume.truncation, RES, RES, RES, ea._lib.ptr(volume.tsdf),
                                            ea._lib.ptr(volume.weight), ea._lib.ptr(depth), ea._lib.ptr(mask), ea._lib.ptr(k), ea._lib.ptr(rot_d),
                                            ea._lib.ptr(tr_d), ea._lib.ptr(scales_d), N, H, W, 1.0, ea._lib.ptr(sums), ea._lib.ptr(flags), *outs,
                                            ea._lib.ptr(workspace), need, ea._lib.stream()), "endo_fusion_track")

    ms_bare = device_ms(lambda: launch(False), window_ms=100.0)
    ms_maps = device_ms(lambda: launch(True), window_ms=100.0)
    got = sums.cpu().numpy()
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(20):
        out = volume.residuals(depth, mask, k, rotations, translations, scales=scales, per_pixel=False)
    ms_read = (time.perf_counter() - start) * 1000.0 / 20
    assert out["sums"].tobytes() == got.tobytes()
    start = time.perf_counter()
    fits = volume.track(depth, mask, k, rotations, translations, scales=scales, iterations=5, tolerance=0.0)
    ms_track = (time.perf_counter() - start) * 1000.0
    args = (volume, depth, mask, k, rot_d.float(), tr_d.float(), scales_d, 1.0)
    want = torch_sums(*args).cpu().numpy()
    ms_torch = device_ms(lambda: torch_sums(*args), window_ms=200.0)
    pixels = N * H * W
    print()
    print("endo_fusion_track arc: 8 x %d x %d pixels against %d^3: %.3f ms per call of device time without the per-pixel outputs, %.3f ms with "
          "them (2 launches); %d of %d pixels are samples; residuals() with its one read: %.3f ms of wall time; track() of 5 iterations "
          "(6 calls and reads, 5 x 8 solves of 7 x 7): %.2f ms of wall time, %s; the same sums in plain torch ops: %.3f ms (%.0fx)" % (
              H, W, RES, ms_bare, ms_maps, int(got[:, 0].sum()), pixels, ms_read, ms_track, sorted(set(fit.status for fit in fits)), ms_torch,
              ms_torch / ms_bare))
    # the torch sums are another order of fp32 operations: a sanity check of the numbers timed, not a contract
    assert np.abs(got[:, 0] - want[:, 0]).max() <= 1.0e-3 * pixels / N and np.isfinite(got).all()
    assert np.abs(got[:, 1] - want[:, 1]).max() <= 1.0e-2 * np.abs(want[:, 1]).max()
