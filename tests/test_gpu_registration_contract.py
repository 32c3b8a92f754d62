"""The workspace contract of the C ABI (include/endo_hip.h) for the registration entries: endo_registration_prepare,
endo_registration_match (with its sums) and endo_similarity_apply inside tests/guarded_alloc.py's context, as
tests/test_gpu_workspace_contract.py uses it.  Every buffer the Python side allocates -- the prepared target, the workspace of per-block
partials, index, distance, the 20 sums, the moved rows -- gets 64 KiB of guard bytes on either side; no write may fall outside, and a
run on NaN-poisoned buffers must give the bytes of a run on zero-filled ones.  Nothing here writes out of bounds or provokes a fault:
a violated guard is an assertion failure that names the allocation."""
import importlib

import numpy as np
import pytest
import torch

import registration_restate as rr
from guarded_alloc import guarded
from test_gpu_registration import MOVE, match_case, rows_on_device

pytestmark = pytest.mark.gpu

registration = importlib.import_module("endoscopydepthestimation-pytorch_amd.registration")


def run(fill, m, k, stride, cap):
    source, target, _, _ = match_case(m, k)
    src, tgt = rows_on_device(source, stride), rows_on_device(target, stride)          # inputs: made outside the context
    scale, rot, tr = MOVE
    with guarded(device="cuda", fill=fill) as g:
        model = registration.TargetModel(tgt)
        out = registration.nearest_points(src, model, scale, rot, tr, max_distance=cap)
        moved = registration.similarity_apply(src, scale, rot, tr)
        result = registration.register(src, model, scale, rot, tr, iterations=3)
        torch.cuda.synchronize()
        sites = [b.site for b in g.blocks]
        assert g.block_of(model.prepared) is not None and g.block_of(out["index"]) is not None and len(g.blocks) >= 10
        assert any("registration.py" in s for s in sites)
    # leaving the block has compared every guard byte
    return {"prepared": model.prepared.cpu().numpy(), "index": out["index"].cpu().numpy(), "distance": out["distance"].cpu().numpy(),
            "sums": out["sums"], "moved": moved.cpu().numpy(), "icp_index": result.index.cpu().numpy(),
            "icp_distance": result.distance.cpu().numpy(), "icp": np.concatenate([[result.scale, result.rms], result.translation])}


def sizes():
    st, tt = registration.SOURCE_TILE, registration.TARGET_TILE
    return {"small": (st - 1, tt - 1), "tiles": (st, tt), "past-tiles": (st + 1, tt + 1), "1000x4099": (1000, 4099)}


@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("size", ["small", "tiles", "past-tiles", "1000x4099"])
def test_registration_entries_on_guarded_buffers(size, stride):
    m, k = sizes()[size]
    poisoned = run("poison", m, k, stride, 0.4)
    zeroed = run("zeros", m, k, stride, 0.4)
    for key in poisoned:
        assert poisoned[key].tobytes() == zeroed[key].tobytes(), key
    assert np.isfinite(poisoned["sums"]).all() and np.isfinite(poisoned["distance"]).all() and np.isfinite(poisoned["moved"]).all()
    assert 0 < poisoned["sums"][0] < m
    source, _, _, _ = match_case(m, k)
    want = rr.apply(source, *MOVE)
    assert (np.abs(poisoned["moved"][:, :3] - want) <= 2.0 ** -24 * np.abs(want) + 1e-12).all()
