"""CPU-only checks of the TSDF fusion: the C entries are declared and exported, fusion.hip is built with its flag, the Python side
refuses bad arguments before any device work, and tests/fusion_restate.py -- the numpy statement the device results are compared with
byte for byte -- is itself held to geometry it does not share with the kernel: depth maps of a plane rendered in fp64 give back
points on that plane."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import fusion_restate as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion = ea.fusion

ENTRIES = ("endo_fusion_tile", "endo_fusion_workspace_bytes", "endo_fusion_clear", "endo_fusion_integrate",
           "endo_fusion_extract_workspace_bytes", "endo_fusion_count", "endo_fusion_extract")


def test_entries_are_declared_exported_and_built_with_the_flag():
    import __graft_entry__ as entry
    assert "fusion.hip" in entry.SOURCES and entry.EXTRA_FLAGS["fusion.hip"] == ["-ffp-contract=off"]
    if not os.path.exists(ea._lib.LIB_PATH):
        entry.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "endo_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(ea._lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared" % name
        assert hasattr(raw, name), "libendo_hip.so does not export %s" % name
        assert name in ea._lib.SIGNATURES
    lib = ea._lib.load()
    assert lib.endo_abi_version() == 7          # the entries are additive
    box = fusion.WAVE_BOX
    assert len(box) == 3 and box[0] % 4 == 0 and box[0] * box[1] * box[2] == 256 and lib.endo_fusion_tile(3) == -1
    # argument validation happens before any device work
    assert lib.endo_fusion_workspace_bytes(8, 256, 320) >= 8 * 18 * 4 and lib.endo_fusion_workspace_bytes(0, 256, 320) == -1
    assert lib.endo_fusion_extract_workspace_bytes(40, 24, 20) >= 24 * 20 * 8
    assert lib.endo_fusion_extract_workspace_bytes(42, 24, 20) == -1 and lib.endo_fusion_extract_workspace_bytes(40, 0, 20) == -1
    assert lib.endo_fusion_extract_workspace_bytes(512, 512, 512) > 0          # 2^27 voxels: 64-bit indices
    assert lib.endo_fusion_clear(40, 24, 20, None, None, None, None) == -1
    assert lib.endo_fusion_integrate(*([None] * 7), 1, 16, 24, None, 0.5, 2.0, 64.0, 40, 24, 20, None, None, None, None, 0, None, 0, None) == -1
    assert lib.endo_fusion_count(None, 0.5, 40, 24, 20, None, None, None, 1.0, None, None, 0, None) == -1
    assert lib.endo_fusion_extract(None, 0.5, 40, 24, 20, None, None, None, 1.0, None, 0, None, None, 0, None) == -1
    assert "fusion" in ea.__dict__ and hasattr(ea.evaluate, "run_fusion_phase")


@pytest.mark.parametrize("kwargs, word", [
    (dict(origin=(0, 0, 0), voxel_size=0.5, dims=(42, 24, 20)), "multiple of 4"),
    (dict(origin=(0, 0, 0), voxel_size=0.5, dims=(40, 0, 20)), "positive"),
    (dict(origin=(0, 0, 0), voxel_size=0.5, dims=(-4, 24, 20)), "positive"),
    (dict(origin=(0, 0, 0), voxel_size=0.0, dims=(40, 24, 20)), "voxel_size"),
    (dict(origin=(0, 0, 0), voxel_size=float("nan"), dims=(40, 24, 20)), "voxel_size"),
    (dict(origin=(0, float("inf"), 0), voxel_size=0.5, dims=(40, 24, 20)), "origin"),
    (dict(origin=(0, float("nan"), 0), voxel_size=0.5, dims=(40, 24, 20)), "origin"),
    (dict(origin=(0, 0, 0), voxel_size=0.5, dims=(40, 24, 20), truncation=-1.0), "truncation"),
    (dict(origin=(0, 0, 0), voxel_size=0.5, dims=(40, 24, 20), max_weight=0.0), "max_weight"),
    (dict(origin=(0, 0, 0), voxel_size=0.5, dims=(40, 24, 70000)), "outside"),
    (dict(origin=(0, 0, 0), voxel_size=0.5, dims=(2 ** 30, 2 ** 10, 2 ** 10)), "outside"),
])
def test_volume_arguments_are_refused_without_a_gpu(kwargs, word):
    with pytest.raises(ValueError, match=word):
        fusion.TSDFVolume(**kwargs)


def test_around_refuses_host_rows_and_bad_boxes():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fusion.TSDFVolume.around(torch.zeros((5, 6)))
    with pytest.raises(ValueError, match="rows"):
        fusion.TSDFVolume.around(torch.zeros((5, 2)))
    with pytest.raises(ValueError, match="not finite"):
        fusion.TSDFVolume.around_bounds((0, 0, 0), (1, float("nan"), 1))
    with pytest.raises(ValueError, match="no extent"):
        fusion.TSDFVolume.around_bounds((1, 1, 1), (1, 1, 1))


# ---- the restatement against a plane ----------------------------------------------------------------------------------------------
H, W, FOCAL = 16, 24, 20.0
TRANSLATIONS = np.array([[0.0, 0.0, 0.0], [1.5, -1.0, 2.0], [-2.0, 0.5, -3.0]])
SCENES = {
    "fronto-parallel": (np.array([0.0, 0.0, 1.0]), [np.eye(3)] * 3),
    "tilted": (np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0]),
               [fr.rotation_about((0, 1, 0), 10.0), fr.rotation_about((1, 0, 0), -12.0), fr.rotation_about((1, 1, 0), 8.0)]),
}


def plane_scene(name):
    normal, rotations = SCENES[name]
    k = fr.intrinsics(FOCAL, H, W)
    depth = fr.render_plane(normal, 30.0, rotations, TRANSLATIONS, k, H, W)
    volume = fr.Volume((-10.0, -6.0, 25.0), 0.5, (40, 24, 20), truncation=2.0)
    colors = np.full((3, H, W, 3), 128, np.uint8)
    flags = fr.integrate(volume, depth, np.ones((3, H, W), np.float32), colors, np.stack([k] * 3), np.stack(rotations), TRANSLATIONS,
                         scales=np.ones(3, np.float32))
    assert flags == ["ok"] * 3
    return volume, normal, rotations, depth, k


def frames_that_see(volume, normal, rotations, depth, k):
    """fp64, voxel by voxel: how many cameras have the voxel's centre inside their image, on a pixel with depth, no further than the
    truncation behind the surface; and whether the count is safe from rounding (no test within 1e-4 of its threshold)."""
    cx, cy, cz = (c.astype(np.float64) for c in volume.centres())
    pts = np.stack(np.meshgrid(cz, cy, cx, indexing="ij")[::-1], axis=-1)
    seen = np.zeros(pts.shape[:3], int)
    safe = np.ones(pts.shape[:3], bool)
    for rot, tr, dmap in zip(rotations, TRANSLATIONS, depth):
        p = (pts - tr) @ rot          # Rt (c - t)
        with np.errstate(all="ignore"):
            u = k[0, 0] * p[..., 0] / p[..., 2] + k[0, 2]
            v = k[1, 1] * p[..., 1] / p[..., 2] + k[1, 2]
        inside = (p[..., 2] > 0) & (np.rint(u) >= 0) & (np.rint(u) <= W - 1) & (np.rint(v) >= 0) & (np.rint(v) <= H - 1)
        ui, vi = np.where(inside, np.rint(u), 0).astype(int), np.where(inside, np.rint(v), 0).astype(int)
        z = dmap[vi, ui].astype(np.float64)
        sdf = z - p[..., 2]
        seen += inside & (z > 0) & (sdf >= -2.0)
        for value in (u - np.floor(u) - 0.5, v - np.floor(v) - 0.5, sdf + 2.0):
            safe &= ~(np.abs(value) < 1e-4)
    return seen, safe


@pytest.mark.parametrize("name", ["fronto-parallel", "tilted"])
def test_restatement_recovers_a_plane(name):
    volume, normal, rotations, depth, k = plane_scene(name)
    rows = fr.extract(volume, 1.0)
    distance = np.abs(rows[:, :3].astype(np.float64) @ normal - 30.0)
    print("%s: %d rows, worst distance to the plane %.3g voxel" % (name, rows.shape[0], distance.max() / 0.5))
    assert rows.shape[0] >= 40 * 24 and np.isfinite(rows).all()
    if name == "fronto-parallel":
        assert rows.shape[0] == 40 * 24 and (distance == 0.0).all()          # constant depth, exact interpolation
        assert (rows[:, 2] == 30.0).all()
    else:
        assert distance.max() <= 0.5          # a crossing is bracketed by two adjacent centres: one voxel edge
    assert (rows[:, 3:] == 128.0).all()
    # the weight of a voxel is the number of frames that saw it
    seen, safe = frames_that_see(volume, normal, rotations, depth, k)
    assert safe.mean() > 0.9 and volume.weight.max() == 3.0
    assert np.array_equal(volume.weight[safe], seen[safe].astype(np.float32))
    assert set(np.unique(volume.weight)) <= {0.0, 1.0, 2.0, 3.0}
    assert (volume.tsdf[volume.weight == 0] == 1.0).all() and (volume.color[:, volume.weight == 0] == 0.0).all()
    # every surface edge lies between voxels at least two frames saw
    assert fr.extract(volume, 2.0).tobytes() == rows.tobytes()


def test_restatement_scales_flags_and_weight_cap():
    depth = np.full((4, 5, 6), 7.0, np.float32)
    depth[0, 2, 3] = 3.0
    depth[3, 0, 0] = np.nan
    depth[3, 1, 1] = 2.0
    bnd = np.ones((4, 5, 6), np.float32)
    bnd[1] = 0.0
    scales, flags = fr.frame_scales(depth, bnd)
    assert flags == ["ok", "empty", "zero_range", "ok"] and scales[0] == 5.0 and scales[3] == 4.0          # fmin / fmax skip the NaN
    assert fr.frame_scales(depth, bnd, [1.0, 1.0, np.inf, -1.0])[1] == ["ok", "empty", "bad_scale", "bad_scale"]
    # the same frame five times with max_weight = 3: the weight stops at 3, the value stays the frame's own
    k = fr.intrinsics(FOCAL, H, W)
    one = fr.render_plane((0, 0, 1), 30.0, [np.eye(3)], [np.zeros(3)], k, H, W)
    volume = fr.Volume((-10.0, -6.0, 25.0), 0.5, (40, 24, 20), truncation=2.0, max_weight=3.0)
    for _ in range(5):
        fr.integrate(volume, one, np.ones((1, H, W), np.float32), np.full((1, H, W, 3), 9, np.uint8), k[None], [np.eye(3)], [np.zeros(3)],
                     scales=[1.0])
    assert volume.weight.max() == 3.0 and set(np.unique(volume.weight)) == {0.0, 3.0}
    single = fr.Volume((-10.0, -6.0, 25.0), 0.5, (40, 24, 20), truncation=2.0)
    fr.integrate(single, one, np.ones((1, H, W), np.float32), np.full((1, H, W, 3), 9, np.uint8), k[None], [np.eye(3)], [np.zeros(3)],
                 scales=[1.0])
    assert np.array_equal(volume.tsdf, single.tsdf)
