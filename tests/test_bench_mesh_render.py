"""Timing prints of the triangle-mesh rasteriser: run by hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""
import importlib

import numpy as np
import pytest
import torch

import mesh_render_restate as mr
from test_bench_fusion import H, N, RES, VS, W, frames
from test_bench_registration import device_ms

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion, mesh = ea.fusion, ea.mesh
PASSES = ("mesh_clear_kernel", "mesh_setup_kernel", "mesh_queue_kernel", "mesh_resolve_kernel")


def big_tube(rings, sectors, radius=1.0, length=6.0):
    """mesh_render_restate.tube's shape without its loops: 2 * rings * sectors triangles."""
    z = length * np.arange(rings + 1) / rings
    angle = 2.0 * np.pi * np.arange(sectors) / sectors
    rad = radius * (1.0 + 0.15 * np.sin(3.0 * angle[None, :] + z[:, None]))
    points = np.stack([rad * np.cos(angle)[None, :] + 0.3 * np.sin(z)[:, None], rad * np.sin(angle)[None, :], np.broadcast_to(z[:, None], rad.shape)], axis=-1)
    a = (np.arange(rings)[:, None] * sectors + np.arange(sectors)[None, :]).reshape(-1)
    b = (np.arange(rings)[:, None] * sectors + (np.arange(sectors)[None, :] + 1) % sectors).reshape(-1)
    faces = np.stack([np.stack([a, a + sectors, b], axis=1), np.stack([b, a + sectors, b + sectors], axis=1)], axis=1).reshape(-1, 3)
    return points.reshape(-1, 3).astype(np.float32), faces.astype(np.int32)


def cameras():
    eyes = [(0.05 * i, 0.03 * i - 0.1, 0.4 + 0.5 * i) for i in range(N)]
    targets = [(0.3 * np.sin(e[2] + 1.5), 0.1, e[2] + 1.5) for e in eyes]
    return np.stack([mr.look_at(e, t) for e, t in zip(eyes, targets)]), np.asarray(eyes, np.float64)


def pass_shares(call):
    """Device time per kernel of one call, by name, from torch's profiler; None where it cannot tell."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                call()
            torch.cuda.synchronize()
        times = {}
        for event in prof.key_averages():
            for name in PASSES:
                if name in event.key:
                    total = getattr(event, "device_time_total", None)
                    times[name] = (total if total is not None else event.cuda_time_total) / 5.0 / 1000.0
        return times if len(times) == len(PASSES) else None
    except Exception:          # a profiler that is not there: the totals stand without their shares
        return None


def queued_triangles(model, k, rotations, translations):
    """The queue's count after one call with a workspace of the bench's own (the layout of include/endo_hip.h)."""
    lib = ea._lib.load()
    d = model.device
    rot, tr = torch.from_numpy(rotations).to(d), torch.from_numpy(translations).to(d)
    triangles = int(model.faces.shape[0])
    need = int(lib.endo_mesh_render_workspace_bytes(N, H, W, triangles))
    workspace = torch.empty(need, dtype=torch.uint8, device=d)
    depth = torch.empty((N, 1, H, W), dtype=torch.float32, device=d)
    ea._lib.check(lib.endo_mesh_render(ea._lib.ptr(model.vertices), 3, int(model.vertices.shape[0]), ea._lib.ptr(model.faces), triangles,
                                       ea._lib.ptr(k), ea._lib.ptr(rot), ea._lib.ptr(tr), None, None, N, H, W, 0, ea._lib.ptr(depth), None, None,
                                       None, None, None, None, ea._lib.ptr(workspace), need, ea._lib.stream()), "endo_mesh_render")
    at = (N * H * W * 8 + 255) // 256 * 256
    return int(workspace[at:at + 8].view(torch.int64).cpu()[0])


def test_bench_mesh_render():
    """Device time per render of 8 frames of 256 x 320 from inside a synthetic tube of about 10^6 triangles and of 10^4, the share of
    each of the four launches, the number of queued (frame, triangle) pairs, and TSDFVolume.render of 8 such frames from 256^3 voxels in
    the same job for orientation.  Prints only."""
    k = torch.from_numpy(np.stack([mr.intrinsics(260.0, H, W)] * N)).cuda()
    rotations, translations = cameras()
    print()
    for rings, sectors in ((500, 1000), (50, 100)):
        model = mesh.TriangleMesh(*big_tube(rings, sectors))
        out = model.render(k, rotations, translations, H, W)
        hits = int(out["mask"].sum())
        ms = device_ms(lambda: model.render(k, rotations, translations, H, W), window_ms=200.0)
        shares = pass_shares(lambda: model.render(k, rotations, translations, H, W))
        queued = queued_triangles(model, k, rotations, translations)
        text = "unavailable" if shares is None else ", ".join("%s %.3f ms" % (name.replace("mesh_", "").replace("_kernel", ""), shares[name]) for name in PASSES)
        print("endo_mesh_render tube of %d triangles: 8 x %d x %d pixels: %.3f ms per call (4 launches); per launch: %s; %d of %d (frame, "
              "triangle) pairs queued; %d of %d pixels hit" % (model.faces.shape[0], H, W, ms, text, queued, N * model.faces.shape[0], hits, N * H * W))
        assert torch.isfinite(out["depth"]).all()
    inputs = frames("arc")
    volume = fusion.TSDFVolume((-0.5 * RES * VS,) * 3, VS, (RES, RES, RES), device="cuda:0")
    scales = torch.ones(N, device="cuda:0")
    volume.integrate(*inputs, scales=scales)
    ms = device_ms(lambda: volume.render(inputs[3], inputs[4], inputs[5], H, W, scales=scales), window_ms=200.0)
    print("for orientation, TSDFVolume.render of 8 x %d x %d rays through %d^3 voxels: %.3f ms per call" % (H, W, RES, ms))
