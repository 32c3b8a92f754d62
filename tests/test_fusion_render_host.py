"""CPU-only checks of the volume renderer: the argument validation of endo_fusion_render and of fusion.TSDFVolume.render (every call
here is refused before any device work), and properties of tests/fusion_render_restate.py itself -- the sample grid, the safety of the
brick rule on the cases of tests/test_gpu_fusion_render.py, and the accuracy of a rendered plane.  The device gets the same properties
through byte equality with the restatement (tests/test_gpu_fusion_render.py)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import fusion_render_restate as rr
import fusion_restate as fr
from test_gpu_fusion import KINDS, NORMAL, TRUNC, VS, origin_of
from test_gpu_fusion_render import HAND_MADE, MASKED, PLAIN, arguments, brick, integrated, render_sizes, wanted

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion = ea.fusion
BADARG = -1
BRICK = brick()          # the library's own brick size: every test here is about the entries that come with it


def test_queries():
    lib = ea._lib.load()
    assert [lib.endo_fusion_render_tile(which) for which in range(6)] == [8, 8, 8, 8, 8, BADARG] and lib.endo_fusion_render_tile(-1) == BADARG
    assert fusion.RENDER_TILE == (8, 8) and fusion.RENDER_BRICK == (8, 8, 8) and fusion.NO_SKIP == 2
    b = BRICK
    want = -(-40 // b) * -(-24 // b) * -(-20 // b)
    assert lib.endo_fusion_render_workspace_bytes(8, 37, 53, 40, 24, 20) == (want + 255) // 256 * 256
    assert lib.endo_fusion_render_workspace_bytes(1, 1, 1, 256, 256, 256) == (256 // b) ** 3
    for bad in ((0, 16, 24, 40, 24, 20), (1, 0, 24, 40, 24, 20), (1, 16, -1, 40, 24, 20), (1, 16, 24, 42, 24, 20), (1, 16, 24, 40, 0, 20),
                (1, 16, 24, 40, 24, 70000), (1, 16, 24, (1 << 24) + 4, 1, 1), (65536, 16, 24, 40, 24, 20), (1, 65535 * 16 + 1, 1, 40, 24, 20)):
        assert lib.endo_fusion_render_workspace_bytes(*bad) == -1, bad


def test_endo_fusion_render_refuses_bad_arguments_before_any_device_work():
    """No call here is valid, so none launches: the pointers are host addresses that are never followed."""
    lib = ea._lib.load()
    block = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(block) + 255) // 256 * 256

    def p(offset=0):
        return ctypes.c_void_p(base + offset)

    origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    good = dict(origin=origin, voxel_size=0.5, truncation=0.75, nx=40, ny=24, nz=20, tsdf=p(), weight=p(16), color=p(32), intrinsics=p(),
                rotations=p(), translations=p(), scales=None, boundaries=None, frames=2, height=16, width=24, min_weight=1.0, step=0.5,
                options=0, depth=p(), mask=p(), colors=p(), normals=p(), workspace=p(), workspace_bytes=256, stream=None)
    bad = [dict(tsdf=None), dict(weight=None), dict(color=None), dict(tsdf=p(4)), dict(weight=p(8)), dict(color=p(12)), dict(origin=None),
           dict(origin=(ctypes.c_double * 3)(0.0, float("nan"), 0.0)), dict(voxel_size=0.0), dict(voxel_size=float("inf")),
           dict(truncation=0.0), dict(truncation=float("nan")), dict(nx=42), dict(ny=0), dict(nz=65536), dict(frames=0), dict(height=0),
           dict(width=-3), dict(intrinsics=None), dict(rotations=None), dict(translations=None), dict(depth=None), dict(mask=None),
           dict(colors=None), dict(normals=None), dict(workspace=None), dict(workspace_bytes=255), dict(min_weight=float("nan")),
           dict(step=0.0), dict(step=-0.5), dict(step=float("nan")), dict(step=float("inf")), dict(step=1.75),          # 1.75 * 0.5 > 0.75
           dict(step=5.0e-5),                                                                                         # 90 / step > 2^20
           dict(options=1), dict(options=4), dict(options=-1)]
    for change in bad:
        args = dict(good, **change)
        assert lib.endo_fusion_render(*args.values()) == BADARG, change
    assert list(good) == ["origin", "voxel_size", "truncation", "nx", "ny", "nz", "tsdf", "weight", "color", "intrinsics", "rotations",
                          "translations", "scales", "boundaries", "frames", "height", "width", "min_weight", "step", "options", "depth",
                          "mask", "colors", "normals", "workspace", "workspace_bytes", "stream"]


def test_render_checks_its_arguments_like_integrate():
    volume = fusion.TSDFVolume.__new__(fusion.TSDFVolume)          # (no device here: the checks below come before any device work)
    volume.origin, volume.voxel_size, volume.dims, volume.truncation = np.zeros(3), VS, (40, 24, 20), TRUNC
    volume.device = torch.device("cuda:0")
    k = torch.from_numpy(np.stack([fr.intrinsics(20.0, 16, 24)] * 2))
    pose = (np.stack([np.eye(3)] * 2), np.zeros((2, 3)), 16, 24)
    with pytest.raises(RuntimeError, match="intrinsics must live on the GPU: the MI355X path has no CPU fallback"):
        volume.render(k, *pose)
    with pytest.raises(ValueError, match="intrinsics"):
        volume.render(k.numpy(), *pose)
    with pytest.raises(ValueError, match="intrinsics"):
        volume.render(k[0], *pose)
    with pytest.raises(ValueError, match="NaN"):
        volume.render(k, *pose, min_weight=float("nan"))
    for step in (0.0, -1.0, float("nan"), 1.75):
        with pytest.raises(ValueError, match="step must be positive and at most"):
            volume.render(k, *pose, step=step)


def test_the_sample_grid_does_not_depend_on_the_path():
    """t_k = float(k) * dt is a product, not a running sum: sample k is the same number whether the samples before it were taken or
    skipped, and the restatement's outputs with and without skipping are the same bytes."""
    h, w = 16, 24
    k = fr.intrinsics(20.0, h, w)
    rot, tr = KINDS["tilted"][0], KINDS["tilted"][1]
    times = rr.sample_times(k, rot, tr, h, w, VS, 0.5, 300)
    assert times.dtype == np.float32 and times.shape == (300, h * w)
    dt = times[0]
    for sample in (2, 3, 7, 150, 299, 300):          # sample k from nothing but k and dt
        assert times[sample - 1].tobytes() == (np.float32(sample) * dt).tobytes()
    running = np.cumsum(np.broadcast_to(dt, times.shape), axis=0, dtype=np.float32)
    assert (running != times).any()          # which a sum over the path taken would not give
    assert (np.diff(times.astype(np.float64), axis=0) > 0).all()
    # step voxels of distance per sample, for every pixel
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    norm = np.sqrt(((u - k[0, 2]) / k[0, 0]) ** 2 + ((v - k[1, 2]) / k[1, 1]) ** 2 + 1.0).reshape(-1)
    assert np.abs(dt.astype(np.float64) * norm - 0.5 * VS).max() < 1e-6 * VS


@pytest.mark.parametrize("n, h, w", [(1, 16, 24), (3, 16, 24), (8, 16, 24), (8, 37, 53)])
def test_the_brick_rule_is_safe_on_the_integrated_cases(n, h, w):
    for size in render_sizes():
        volume = integrated(size, n, h, w)
        for params in (PLAIN, MASKED):
            kw = arguments(volume, n, h, w, params)
            with_marks, without = {}, {}
            a = rr.render(volume, brick=BRICK, stats=with_marks, skip=True, **kw)
            b = rr.render(volume, brick=BRICK, stats=without, skip=False, **kw)
            assert without["unsafe"] == 0          # every sample that ends a ray lies in a marked brick
            assert all(a[name].tobytes() == b[name].tobytes() for name in a), (size, params)
            assert np.array_equal(with_marks["end"], without["end"]) and np.array_equal(with_marks["outcome"], without["outcome"])
            assert with_marks["evaluated"] + with_marks["skipped"] <= without["evaluated"] and without["skipped"] == 0


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_the_brick_rule_is_safe_on_the_hand_made_cases(name):
    volume, n, h, w = wanted(name)[0], 3, 16, 24
    kw = arguments(volume, n, h, w, PLAIN)
    without = {}
    a = rr.render(volume, brick=BRICK, skip=True, **kw)
    b = rr.render(volume, brick=BRICK, stats=without, skip=False, **kw)
    assert without["unsafe"] == 0 and all(a[key].tobytes() == b[key].tobytes() for key in a)
    assert np.isfinite(a["depth"]).all() and np.isfinite(a["normals"]).all()
    hit = a["mask"] > 0
    assert set(np.unique(a["mask"]).tolist()) <= {0.0, 1.0} and (a["depth"][hit] > 0).all() and (a["depth"][~hit] == 0).all()
    length = np.linalg.norm(a["normals"].astype(np.float64), axis=-1)[hit[:, 0]]
    assert ((np.abs(length - 1.0) < 1e-6) | (length == 0)).all()


def test_a_rendered_plane_lies_on_the_plane():
    """One noise-free front_near frame of the plane (tests/test_gpu_fusion.py) integrated at scale 1 into 40 x 24 x 20 voxels of 0.5
    with truncation 0.75, rendered from the same pose at 37 x 53: the depth at the hit pixels against the fp64 map.  Measured here, on
    the CPU: 394 hits of 1961 rays, maximum error 0.022705 units = 0.04541 voxel at step 0.5 (0.021133 at step 1.0, 332 hits); the bound
    is twice the measured value -- another order of operations moves single crossings -- and stays under the cap of a quarter voxel,
    above which a wrongly chosen bracketing sample would pass."""
    h, w, dims = 37, 53, (40, 24, 20)
    k = fr.intrinsics(40.0, h, w)
    rot, tr = np.eye(3)[None], np.zeros((1, 3))
    truth = fr.render_plane(NORMAL, 30.0 * NORMAL[2] + KINDS["front_near"][2], rot, tr, k, h, w)
    colors = np.random.default_rng(1).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    volume = fr.Volume(origin_of(dims), VS, dims, truncation=TRUNC)
    assert fr.integrate(volume, truth, np.ones_like(truth), colors, k[None], rot, tr, scales=np.ones(1, np.float32)) == ["ok"]
    for step, measured in ((0.5, 0.022705078125), (1.0, 0.0211334228515625)):
        bound = 2.0 * measured
        assert bound <= 0.25 * VS
        out = rr.render(volume, k[None], rot, tr, h, w, step=step, brick=BRICK)
        hit = out["mask"][0, 0] > 0
        error = np.abs(out["depth"][0, 0].astype(np.float64) - truth[0].astype(np.float64))[hit]
        print("step %g: %d hits of %d rays, maximum error %.6f units = %.5f voxel" % (step, hit.sum(), h * w, error.max(), error.max() / VS))
        assert hit.sum() >= 300 and error.max() <= bound
        # the normals look at the camera, against the plane's normal; uneven scales only divide the depth
        assert (out["normals"][0][hit].astype(np.float64) @ NORMAL < -0.99).all()
        scaled = rr.render(volume, k[None], rot, tr, h, w, step=step, scales=[0.75], brick=BRICK)
        assert scaled["mask"].tobytes() == out["mask"].tobytes() and scaled["normals"].tobytes() == out["normals"].tobytes()
        assert np.abs(scaled["depth"].astype(np.float64) * 0.75 - out["depth"]).max() <= 1e-6 * 40.0
