"""Timing prints of the mesh extraction: run by hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""
import importlib

import pytest
import torch

from test_bench_fusion import HBM_BYTES_PER_S, N, RES, VS, frames
from test_bench_registration import device_ms

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion = ea.fusion


@pytest.mark.parametrize("kind", ["all", "arc"])
def test_bench_extract_mesh(kind):
    """Device time of extract_mesh's count (two launches), vertex and face launches on test_bench_fusion.py's two 256^3 volumes, of the
    whole call with its one read, and of extract in the same job; the bytes each launch moves by its own arithmetic (the tsdf and
    weight planes once per launch, 36 bytes per row, 12 per triangle) and the fraction of achievable HBM bandwidth that is.  Prints
    only."""
    inputs = frames(kind)
    volume = fusion.TSDFVolume((-0.5 * RES * VS,) * 3, VS, (RES, RES, RES), device="cuda:0")
    assert volume.integrate(*inputs, scales=torch.ones(N, device="cuda:0")) == ["ok"] * N
    vertices, normals, faces = volume.extract_mesh(1.0)
    points, triangles = int(vertices.shape[0]), int(faces.shape[0])
    assert torch.equal(vertices, volume.extract(1.0)) and points > 0 and triangles > 0
    assert int(faces.min()) >= 0 and int(faces.max()) < points
    lib = ea._lib.load()
    need = int(lib.endo_fusion_mesh_workspace_bytes(RES, RES, RES))
    workspace = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    totals = torch.empty(4, dtype=torch.int64, device="cuda:0")
    vol = (fusion._host_doubles(volume.origin), volume.voxel_size, RES, RES, RES, ea._lib.ptr(volume.tsdf), ea._lib.ptr(volume.weight),
           ea._lib.ptr(volume.color), 1.0)
    state = (ea._lib.ptr(totals), ea._lib.ptr(workspace), need, ea._lib.stream())
    ms_count = device_ms(lambda: ea._lib.check(lib.endo_fusion_mesh_count(*(vol + state)), "count"))
    ms_vertices = device_ms(lambda: ea._lib.check(lib.endo_fusion_mesh_vertices(
        *(vol + (ea._lib.ptr(vertices), ea._lib.ptr(normals), points) + state)), "vertices"))
    ms_faces = device_ms(lambda: ea._lib.check(lib.endo_fusion_mesh_faces(*(vol + (ea._lib.ptr(faces), triangles) + state)), "faces"))
    ms_mesh = device_ms(lambda: volume.extract_mesh(1.0), window_ms=100.0)
    ms_extract = device_ms(lambda: volume.extract(1.0), window_ms=100.0)
    planes = 8.0 * RES ** 3
    moved = {"count": planes, "vertices": planes + 36.0 * points, "faces": planes + 12.0 * triangles}
    print()
    print("extract_mesh %s: %d^3, %d rows, %d triangles: count %.3f ms (%.0f MB, %.0f %% of %.1f TB/s); vertices %.3f ms (%.0f MB, %.0f %%); "
          "faces %.3f ms (%.0f MB, %.0f %%); the call with its read: %.3f ms; extract in the same job: %.3f ms" % (
              kind, RES, points, triangles, ms_count, moved["count"] / 1e6, 100.0 * moved["count"] / (ms_count * 1e-3) / HBM_BYTES_PER_S,
              HBM_BYTES_PER_S / 1e12, ms_vertices, moved["vertices"] / 1e6, 100.0 * moved["vertices"] / (ms_vertices * 1e-3) / HBM_BYTES_PER_S,
              ms_faces, moved["faces"] / 1e6, 100.0 * moved["faces"] / (ms_faces * 1e-3) / HBM_BYTES_PER_S, ms_mesh, ms_extract))
