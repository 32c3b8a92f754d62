"""The workspace contract of the C ABI (include/endo_hip.h) for endo_mesh_render inside tests/guarded_alloc.py's context, as
tests/test_gpu_fusion_track_contract.py uses it.  Every buffer the Python side allocates -- the keys and the queue, depth, mask,
triangle, barycentric, normals, colours, flags -- gets 64 KiB of guard bytes on either side; no write may fall outside, and a run on
NaN-poisoned buffers must give the bytes of a run on zero-filled ones and of a run outside the context.  Faces whose indices lie outside
the vertices are data here, which the kernel skips: nothing writes out of bounds or provokes a fault, and a violated guard is an
assertion failure that names the allocation."""
import importlib

import numpy as np
import pytest
import torch

import mesh_render_restate as mr
from guarded_alloc import guarded
from test_gpu_mesh_render import OUTPUTS, SCALES, assert_same, boundaries_of, case, device_render, over_tile

pytestmark = pytest.mark.gpu

mesh = importlib.import_module("endoscopydepthestimation-pytorch_amd.mesh")

CASES = {"tube 37x53": ("tube", 37, 53), "mixed over tile": ("mixed",) + over_tile()}


def hostile(vertices, faces):
    """The case's mesh with colour columns and with faces whose indices lie outside 0 .. V - 1 among the honest ones."""
    rng = np.random.default_rng(5)
    rows = np.concatenate([vertices, rng.integers(0, 256, (vertices.shape[0], 3)).astype(np.float32)], axis=1)
    count = vertices.shape[0]
    bad = np.array([[0, 1, -1], [count, 1, 2], [0, 2 ** 31 - 1, 2], [-2 ** 31, 0, 1], [count + 7, count + 8, count + 9]], np.int32)
    return rows, np.concatenate([bad[:2], faces[:faces.shape[0] // 2], bad[2:4], faces[faces.shape[0] // 2:], bad[4:]]).astype(np.int32)


def run(fill, name):
    key, h, w = CASES[name]
    vertices, faces, k, rotations, translations = case(key, h, w)
    rows, faces = hostile(vertices, faces)
    inputs = (torch.from_numpy(rows).cuda(), torch.from_numpy(faces).cuda())          # inputs: made outside the context
    with guarded(device="cuda", fill=fill) as g:
        model = mesh.TriangleMesh(*inputs)
        got = {}
        for masked in (False, True):
            for brute in (False, True):
                got[(masked, brute)] = device_render(model, k, rotations, translations, h, w, masked, brute=brute)
        torch.cuda.synchronize()
        assert all(g.block_of(out[name]) is not None for out in got.values() for name in OUTPUTS)
        assert len(g.blocks) >= 4 * (1 + len(OUTPUTS)) and any("mesh.py" in b.site for b in g.blocks)
    # leaving the block has compared every guard byte
    return {(masked, brute, name): out[name].cpu().numpy() for (masked, brute), out in got.items() for name in OUTPUTS}, got


@pytest.mark.parametrize("name", sorted(CASES))
def test_render_on_guarded_buffers(name):
    key, h, w = CASES[name]
    poisoned, got = run("poison", name)
    zeroed, _ = run("zeros", name)
    for item in poisoned:
        assert poisoned[item].tobytes() == zeroed[item].tobytes(), item
    vertices, faces, k, rotations, translations = case(key, h, w)
    rows, faces = hostile(vertices, faces)
    plain = mesh.TriangleMesh(rows, faces)
    for masked in (False, True):
        want = mr.render(rows, faces, k, rotations, translations, h, w, scales=SCALES, boundaries=boundaries_of(h, w) if masked else None)
        assert want["mask"].sum() > 0 and np.isfinite(want["depth"]).all()
        for brute in (False, True):
            assert_same(got[(masked, brute)], want, "%s masked=%s brute=%s" % (name, masked, brute))
        # the same call outside the context: the same bytes
        assert_same(device_render(plain, k, rotations, translations, h, w, masked), want, "%s masked=%s outside" % (name, masked))
