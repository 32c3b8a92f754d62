"""fusion.TSDFVolume.render on the device against tests/fusion_render_restate.py: depth, mask, colours and normals are compared by
``tobytes()``, with the empty-space skipping on and off.  The volumes are the ones of tests/test_gpu_fusion.py, integrated by the
restatement from its scenes, the sizes around the render kernel's brick (endo_fusion_render_tile), and the hand-made volumes of
tests/test_gpu_fusion_mesh.py; the images are no multiple of the pixel tile; the cameras are the scenes' own poses, one with four times
the focal length and one looking along +x.  Run with ``pytest -m gpu`` on an MI355X."""
import importlib

import numpy as np
import pytest
import torch

import fusion_render_restate as rr
import fusion_restate as fr
from test_gpu_fusion import FRAMES, KINDS, TRUNC, VS, origin_of, scene, volume_sizes
from test_gpu_fusion_mesh import CASES as HAND_MADE, wanted

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
fusion = ea.fusion

IMAGES = [(16, 24), (37, 53)]          # whole 8 x 8 wave tiles with a block's second tile column empty; partial tiles on both sides
OUTPUTS = ("depth", "mask", "colors", "normals")
# (min_weight, step, boundaries, uneven scales)
PLAIN, MASKED = (1.0, 0.5, False, False), (2.0, 1.0, True, True)


def brick():
    (b,) = set(fusion.RENDER_BRICK)
    return b


def render_sizes():
    b = brick()
    sizes = dict(volume_sizes())
    sizes.update({"brick": (b, b, b), "brick_under": (b - 4, b - 1, b - 1), "brick_over": (b + 4, b + 1, b + 1)})
    return sizes


def cameras(n, h, w, centre):
    """(intrinsics (n, 3, 3), rotations, translations) around a volume centred at ``centre``: the poses of scene(n, ...), which look at
    (0, 0, 30), moved with the volume; for n = 3 the inside camera, the front one with four times the focal length (the volume fills
    the image) and one looking along +x from just outside the volume's -x side (its rays leave through every face)."""
    focal = 20.0 if h == 16 else 40.0
    shift = np.asarray(centre, np.float64) - np.array([0.0, 0.0, 30.0])
    if n == 3:
        poses = [KINDS["inside"][:2], KINDS["front"][:2], (fr.rotation_about((0, 1, 0), 90.0), (-12.5, 0.3, 30.2))]
        focals = [focal, 4.0 * focal, focal]
    else:
        poses = [KINDS[kind][:2] for kind in FRAMES[n]]
        focals = [focal] * n
    k = np.stack([fr.intrinsics(fl, h, w) for fl in focals])
    return k, np.stack([p[0] for p in poses]), np.array([p[1] for p in poses], np.float64) + shift


def boundaries_of(n, h, w):
    """The scenes' mask: a masked border and a hole."""
    mask = np.ones((n, h, w), np.float32)
    mask[:, 0, :] = mask[:, -1, :] = mask[:, :, 0] = mask[:, :, -1] = 0.0
    mask[:, h // 3:h // 3 + 2, w // 4:w // 4 + 3] = 0.0
    return mask


def centre_of(volume):
    return volume.origin.astype(np.float64) + 0.5 * float(volume.vs) * np.array([volume.nx, volume.ny, volume.nz])


_volumes, _renders = {}, {}


def integrated(size, n, h, w):
    """The restatement's volume of one size after scene(n, h, w): made once per key and left unchanged."""
    key = (size, n, h, w)
    if key not in _volumes:
        dims = render_sizes()[size]
        volume = fr.Volume(origin_of(dims), VS, dims, truncation=TRUNC)
        fr.integrate(volume, *scene(n, h, w, False), scales=np.ones(n, np.float32))
        _volumes[key] = volume
    return _volumes[key]


def arguments(volume, n, h, w, params):
    min_weight, step, masked, uneven = params
    k, rotations, translations = cameras(n, h, w, centre_of(volume))
    return dict(intrinsics=k, rotations=rotations, translations=translations, height=h, width=w,
                scales=(0.5 + 0.25 * np.arange(n)).astype(np.float32) if uneven else None,
                boundaries=boundaries_of(n, h, w) if masked else None, min_weight=min_weight, step=step)


def restated(key, volume, n, h, w, params):
    """(the restatement's outputs, its stats), made once per key and left unchanged."""
    key = (key, n, h, w, params)
    if key not in _renders:
        stats = {}
        _renders[key] = (rr.render(volume, brick=brick(), stats=stats, **arguments(volume, n, h, w, params)), stats)
    return _renders[key]


def on_device(volume):
    out = fusion.TSDFVolume(volume.origin, float(volume.vs), (volume.nx, volume.ny, volume.nz), truncation=float(volume.trunc), device="cuda:0")
    out.tsdf.copy_(torch.from_numpy(volume.tsdf))
    out.weight.copy_(torch.from_numpy(volume.weight))
    out.color.copy_(torch.from_numpy(volume.color))
    return out


def device_render(device, kw, skip):
    d = device.device
    return device.render(torch.from_numpy(kw["intrinsics"]).to(d), kw["rotations"], kw["translations"], kw["height"], kw["width"],
                         scales=kw["scales"], boundaries=None if kw["boundaries"] is None else torch.from_numpy(kw["boundaries"]).to(d),
                         min_weight=kw["min_weight"], step=kw["step"], skip=skip)


def assert_same_render(got, want, what):
    for name in OUTPUTS:
        a = got[name].cpu().numpy() if torch.is_tensor(got[name]) else got[name]
        b = want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s is %s %s, not %s %s" % (what, name, a.dtype, a.shape, b.dtype, b.shape)
        assert a.tobytes() == b.tobytes(), "%s: %s differs in %d of %d values" % (what, name, int((a != b).sum()), a.size)


def check(key, volume, n, h, w):
    device = on_device(volume)
    before = device._planes.cpu().numpy()
    for params in (PLAIN, MASKED):
        want, _ = restated(key, volume, n, h, w, params)
        kw = arguments(volume, n, h, w, params)
        got = {skip: device_render(device, kw, skip) for skip in (True, False)}
        assert all(t.is_cuda for t in got[True].values())
        for skip in (True, False):
            assert_same_render(got[skip], want, "%s n=%d %dx%d %s skip=%s" % (key, n, h, w, params, skip))
    assert device._planes.cpu().numpy().tobytes() == before.tobytes()          # a render only reads the five planes


@pytest.mark.parametrize("h, w", IMAGES)
@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("size", ["box", "under", "over", "40x24x20", "brick", "brick_under", "brick_over"])
def test_render_of_an_integrated_volume_matches_the_restatement(size, n, h, w):
    volume = integrated(size, n, h, w)
    check(size, volume, n, h, w)
    if size == "40x24x20" and n == 8:          # on the input: the front and the tilted camera see the surface
        outcome = restated(size, volume, n, h, w, PLAIN)[1]["outcome"]
        assert FRAMES[8][0] == "front" and FRAMES[8][7] == "tilted"
        assert (outcome[0] == rr.HIT).sum() >= 50 and (outcome[7] == rr.HIT).sum() >= 50


@pytest.mark.parametrize("n, h, w", [(3, 16, 24), (8, 37, 53)])
@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_render_of_a_hand_made_volume_matches_the_restatement(name, n, h, w):
    check(name, wanted(name)[0], n, h, w)


def test_the_cases_meet_every_outcome():
    """Conditions on the inputs, on the restatement alone: over the cases a ray hits, ends without a hit, misses through observed
    space and is not cast; and a skipped sample precedes an ending one."""
    seen, skipped_before_end, observed_miss = set(), 0, 0
    for n, h, w in ((3, 16, 24), (8, 37, 53)):
        volume = integrated("40x24x20", n, h, w)
        for params in (PLAIN, MASKED):
            stats = restated("40x24x20", volume, n, h, w, params)[1]
            seen.update(np.unique(stats["outcome"]).tolist())
            skipped_before_end += stats["skipped_before_end"]
            assert stats["skipped"] > 0
        plain = {}
        rr.render(volume, brick=brick(), stats=plain, skip=False, **arguments(volume, n, h, w, PLAIN))
        observed_miss += plain["observed_miss"]
        assert plain["unsafe"] == 0
    assert seen == {rr.NO_RAY, rr.HIT, rr.ENDED, rr.MISS} and skipped_before_end > 0 and observed_miss > 0


def test_a_cleared_volume_renders_zeros():
    volume = integrated("40x24x20", 8, 16, 24)
    device = on_device(volume)
    device.clear()
    kw = arguments(volume, 8, 16, 24, MASKED)
    for skip in (True, False):
        out = device_render(device, kw, skip)
        for name in OUTPUTS:
            assert out[name].shape[0] == 8 and int(torch.count_nonzero(out[name])) == 0, name


def test_argument_errors_and_frames_without_a_scale():
    volume = integrated("40x24x20", 3, 16, 24)
    device = on_device(volume)
    kw = arguments(volume, 3, 16, 24, PLAIN)
    k = torch.from_numpy(kw["intrinsics"]).cuda()
    pose = (kw["rotations"], kw["translations"], 16, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        device.render(k.cpu(), *pose)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        device.render(k, *pose, boundaries=torch.ones(3, 16, 24))
    with pytest.raises(ValueError, match="boundaries"):
        device.render(k, *pose, boundaries=torch.ones(2, 16, 24, device="cuda:0"))
    with pytest.raises(ValueError, match="intrinsics"):
        device.render(k.double(), *pose)
    with pytest.raises(ValueError, match="rotations"):
        device.render(k, kw["rotations"][:2], kw["translations"], 16, 24)
    with pytest.raises(ValueError, match="scales"):
        device.render(k, *pose, scales=[1.0, 1.0])
    with pytest.raises(ValueError, match="step"):
        device.render(k, *pose, step=TRUNC / VS + 0.25)
    # a scale that is no scale: the frame renders nothing, the others what they render alone
    scales = np.array([np.nan, 1.0, 0.0], np.float32)
    got = device.render(k, *pose, scales=scales)
    want = rr.render(volume, brick=brick(), **dict(kw, scales=scales))
    assert_same_render(got, want, "scales nan, 1, 0")
    assert int(torch.count_nonzero(got["mask"][0])) == 0 and int(torch.count_nonzero(got["mask"][2])) == 0
    assert got["mask"][1].cpu().numpy().tobytes() == restated("40x24x20", volume, 3, 16, 24, PLAIN)[0]["mask"][1].tobytes()
