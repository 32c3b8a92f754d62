"""The workspace contract of the C ABI (include/endo_hip.h) for the mesh entries: endo_fusion_mesh_count, endo_fusion_mesh_vertices and
endo_fusion_mesh_faces inside tests/guarded_alloc.py's context, as tests/test_gpu_fusion_contract.py uses it.  Every buffer the Python
side allocates -- the planes, the row and cell-row offsets, the totals, the vertices, the normals, the faces -- gets 64 KiB of guard
bytes on either side; no write may fall outside, and a run on NaN-poisoned buffers must give the bytes of a run on zero-filled ones.
Nothing here writes out of bounds or provokes a fault: a violated guard is an assertion failure that names the allocation."""
import importlib

import numpy as np
import pytest
import torch

from guarded_alloc import guarded
from test_gpu_fusion_mesh import assert_same_mesh, wanted

pytestmark = pytest.mark.gpu

fusion = importlib.import_module("endoscopydepthestimation-pytorch_amd.fusion")


def run(fill, name):
    want, min_weight, _ = wanted(name)
    planes = [torch.from_numpy(a).cuda() for a in (want.tsdf, want.weight, want.color)]          # inputs: made outside the context
    with guarded(device="cuda", fill=fill) as g:
        volume = fusion.TSDFVolume(want.origin, float(want.vs), (want.nx, want.ny, want.nz), device="cuda:0")
        volume.tsdf.copy_(planes[0])
        volume.weight.copy_(planes[1])
        volume.color.copy_(planes[2])
        mesh = volume.extract_mesh(min_weight)
        other = volume.extract_mesh(2.0)          # (above every weight of volume A and of the smallest one: nothing at all)
        rows = volume.extract(min_weight)
        torch.cuda.synchronize()
        assert g.block_of(volume._planes) is not None and len(g.blocks) >= 8
        assert all(g.block_of(t) is not None for t in mesh if t.shape[0])
        assert any("fusion.py" in b.site for b in g.blocks)
    # leaving the block has compared every guard byte
    out = {"vertices": mesh[0], "normals": mesh[1], "faces": mesh[2], "other_vertices": other[0], "other_normals": other[1],
           "other_faces": other[2], "rows": rows, "planes": volume._planes}
    return {key: value.cpu().numpy() for key, value in out.items()}


@pytest.mark.parametrize("name", ["A", "C-4x2x2"])
def test_mesh_entries_on_guarded_buffers(name):
    poisoned = run("poison", name)
    zeroed = run("zeros", name)
    for key in poisoned:
        assert poisoned[key].tobytes() == zeroed[key].tobytes(), key
        assert np.isfinite(poisoned[key]).all(), key
    assert_same_mesh((poisoned["vertices"], poisoned["normals"], poisoned["faces"]), wanted(name)[2], name)
    assert poisoned["rows"].tobytes() == poisoned["vertices"].tobytes() and poisoned["faces"].shape[0] > 0
    assert poisoned["other_vertices"].shape == (0, 6) and poisoned["other_faces"].shape == (0, 3)
