"""The workspace contract of the C ABI (include/endo_hip.h) for endo_fusion_render inside tests/guarded_alloc.py's context, as
tests/test_gpu_fusion_mesh_contract.py uses it.  Every buffer the Python side allocates -- the planes, the brick marks, depth, mask,
colours, normals -- gets 64 KiB of guard bytes on either side; no write may fall outside, and a run on NaN-poisoned buffers must give
the bytes of a run on zero-filled ones.  Nothing here writes out of bounds or provokes a fault: a violated guard is an assertion
failure that names the allocation."""
import importlib

import numpy as np
import pytest
import torch

from guarded_alloc import guarded
from test_gpu_fusion_render import MASKED, OUTPUTS, PLAIN, arguments, assert_same_render, device_render, integrated, restated
from test_gpu_fusion_mesh import wanted

pytestmark = pytest.mark.gpu

fusion = importlib.import_module("endoscopydepthestimation-pytorch_amd.fusion")

CASES = {"40x24x20": lambda: integrated("40x24x20", 8, 37, 53), "brick_over": lambda: integrated("brick_over", 8, 37, 53),
         "A": lambda: wanted("A")[0]}


def run(fill, name):
    want = CASES[name]()
    planes = [torch.from_numpy(a).cuda() for a in (want.tsdf, want.weight, want.color)]          # inputs: made outside the context
    out = {}
    with guarded(device="cuda", fill=fill) as g:
        volume = fusion.TSDFVolume(want.origin, float(want.vs), (want.nx, want.ny, want.nz), truncation=float(want.trunc), device="cuda:0")
        volume.tsdf.copy_(planes[0])
        volume.weight.copy_(planes[1])
        volume.color.copy_(planes[2])
        for params in (PLAIN, MASKED):
            for skip in (True, False):
                got = device_render(volume, arguments(want, 8, 37, 53, params), skip)
                out.update({"%s %s skip=%s" % (key, params, skip): value for key, value in got.items()})
        torch.cuda.synchronize()
        assert g.block_of(volume._planes) is not None and len(g.blocks) >= 1 + 4 * 5
        assert all(g.block_of(t) is not None for t in out.values())
        assert any("fusion.py" in b.site for b in g.blocks)
    # leaving the block has compared every guard byte
    out["planes"] = volume._planes
    return {key: value.cpu().numpy() for key, value in out.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_render_on_guarded_buffers(name):
    poisoned = run("poison", name)
    zeroed = run("zeros", name)
    for key in poisoned:
        assert poisoned[key].tobytes() == zeroed[key].tobytes(), key
        assert np.isfinite(poisoned[key]).all(), key
    for params in (PLAIN, MASKED):
        want, _ = restated(name, CASES[name](), 8, 37, 53, params)
        for skip in (True, False):
            assert_same_render({key: poisoned["%s %s skip=%s" % (key, params, skip)] for key in OUTPUTS}, want, "%s %s" % (name, params))
    assert poisoned["mask %s skip=True" % (PLAIN,)].sum() > 0
