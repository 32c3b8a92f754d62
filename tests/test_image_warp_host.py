"""CPU-only checks of the image warping (images_warping, _bilinear_interpolate, _warp_coordinate_generate): the plain-torch restatement
(tests/image_warp_restate.py) reproduces what the reference's own functions gave (tests/golden/image_warp.npz, written by
tests/golden/make_image_warp_golden.py), the fixture holds the cases it is for, and the host side -- exported names, the C entry
points in the ctypes table and the header, refusals, argument validation -- behaves.  No GPU compute is launched here."""

import importlib
import os
import re

import numpy as np
import pytest
import torch

import image_warp_restate as iwr

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "image_warp.npz"
ENTRY_POINTS = ("endo_warp_coordinates_fwd", "endo_warp_coordinates_bwd", "endo_image_warp_fwd", "endo_image_warp_bwd")
EXACT_SHAPES = {"a": (1, 3, 6, 8), "b": (2, 1, 5, 9), "c": (1, 4, 7, 6)}


def arr(g, key):
    return torch.from_numpy(np.array(g[key]))


def rel(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("mode", iwr.MODES)
def test_restatement_reproduces_direct(golden, mode):
    """Output and the three gradients of the ``direct`` record to 1e-6 (max abs error / max |ref|): the same ATen call."""
    g = golden(FIXTURE)
    images, u, v, cot = (arr(g, "direct::" + k) for k in ("images", "u", "v", "cotangent"))
    out, grads = iwr.value_and_grads(images, u, v, mode, cot)
    assert rel(out, arr(g, "direct::%s::out" % mode)) <= 1e-6
    for name, got in zip(("grad_images", "grad_u", "grad_v"), grads):
        want = arr(g, "direct::%s::%s" % (mode, name))
        assert got.shape == want.shape and float(want.abs().max()) > 0
        assert rel(got, want) <= 1e-6, "%s %s: %.3e" % (mode, name, rel(got, want))


@pytest.mark.parametrize("mode", iwr.MODES)
def test_restatement_reproduces_exact(golden, mode):
    g = golden(FIXTURE)
    for key, shape in EXACT_SHAPES.items():
        images, u, v = (arr(g, "exact::%s::%s" % (key, k)) for k in ("images", "u", "v"))
        assert tuple(images.shape) == shape
        with torch.no_grad():
            out = iwr.images_warping(images, u, v, mode)
        assert rel(out, arr(g, "exact::%s::%s::out" % (key, mode))) <= 1e-6, (key, mode)


def test_restatement_reproduces_chain(golden):
    """Coordinates, warped images, MaskedL1Loss and its gradient with respect to the depth, each to 1e-6."""
    import losses_restate as lr
    g = golden(FIXTURE)
    x = iwr.chain_batch()
    depth = x["depth"].clone().requires_grad_(True)
    u, v = iwr.warp_coordinates(depth, x["mask"], x["t"], x["R"], x["K"])
    warped = iwr.images_warping(arr(g, "chain::images_2"), u, v, "zeros")
    loss = lr.masked_l1(arr(g, "chain::images_1"), warped, x["mask"])
    grad, = torch.autograd.grad(loss, depth)
    assert rel(u.detach(), arr(g, "chain::u")) <= 1e-6 and rel(v.detach(), arr(g, "chain::v")) <= 1e-6
    assert rel(warped.detach(), arr(g, "chain::warped")) <= 1e-6
    assert rel(loss.detach(), arr(g, "chain::loss")) <= 1e-6
    assert rel(grad[:, 0], arr(g, "chain::grad_depth")[:, 0]) <= 1e-6


def test_fixture_holds_the_cases_it_is_for(golden):
    """The conditions make_image_warp_golden.py asserts as it writes, read back from the file."""
    g = golden(FIXTURE)
    images, u, v, cot = (np.array(g["direct::" + k]) for k in ("images", "u", "v", "cotangent"))
    assert images.shape == cot.shape == (2, 3, 16, 24) and u.shape == v.shape == (2, 16, 24)
    assert 0.5 <= iwr.check_direct_coordinates(u, v, 16, 24) <= 0.7          # the fractional parts and the spread are asserted inside
    assert u.min() < -0.5 and u.max() > 24.5 and v.min() < -0.5 and v.max() > 16.5
    assert len(np.unique(cot)) > 100
    for mode in iwr.MODES:
        for name in ("out", "grad_images", "grad_u", "grad_v"):
            a = np.array(g["direct::%s::%s" % (mode, name)])
            assert np.isfinite(a).all() and np.abs(a).max() > 0
    for key, (n, c, h, w) in EXACT_SHAPES.items():
        eu, ev = np.array(g["exact::%s::u" % key], np.float64) - 0.5, np.array(g["exact::%s::v" % key], np.float64) - 0.5
        assert np.array(g["exact::%s::images" % key]).shape == (n, c, h, w)
        want = set((x, y) for x in (-1.0, -0.5, 0.0, w - 1.0, w - 0.5, float(w)) for y in (-1.0, -0.5, 0.0, h - 1.0, h - 0.5, float(h)))
        assert set(zip(eu.reshape(-1).tolist(), ev.reshape(-1).tolist())) == want
    assert sorted(c for _, c, _, _ in EXACT_SHAPES.values()) == [1, 3, 4]
    x = iwr.chain_batch()
    for name in ("images_1", "images_2"):
        im = np.array(g["chain::" + name])
        assert im.shape == (2, 3, 32, 64) and max(iwr.adjacent_difference(im)) <= 0.05
    cu, cv = np.array(g["chain::u"]), np.array(g["chain::v"])
    assert iwr.check_chain_coordinates(cu, cv, x["mask"].numpy()) <= iwr.KINK_SHARE          # all four taps inside under the mask, too
    with torch.no_grad():
        ou, ov = iwr.warp_coordinates(x["depth"], x["mask"], x["t"], x["R"], x["K"])
    assert np.array_equal(ou.numpy(), cu) and np.array_equal(ov.numpy(), cv)          # the reference's coordinates are the oracle's, bit for bit
    assert float(np.array(g["chain::loss"])) > 0 and np.abs(np.array(g["chain::grad_depth"])).max() > 0


def test_names_and_entry_points():
    for name in ("images_warping", "_bilinear_interpolate", "_warp_coordinate_generate"):
        assert callable(getattr(ea, name)) and getattr(ea, name) is getattr(ea.models, name)
    text = open(os.path.join(ROOT, "include", "endo_hip.h")).read()
    declared = set(re.findall(r"\b(endo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for name in ENTRY_POINTS:
        assert name in ea._lib.SIGNATURES and name in declared, name
    assert re.search(r"models\.py:377-429", text) and re.search(r"models\.py:317-336", text)


def test_entry_points_validate_before_any_device_work():
    lib = ea._lib.load()
    p = lambda: None          # every pointer null: ENDO_E_BADARG whatever the sizes are
    assert lib.endo_warp_coordinates_fwd(p(), p(), p(), p(), p(), p(), p(), 1, 4, 4, None) == -1
    assert lib.endo_warp_coordinates_bwd(p(), p(), p(), p(), p(), p(), p(), p(), 1, 4, 4, None) == -1
    assert lib.endo_image_warp_fwd(p(), p(), p(), p(), 1, 1, 4, 4, 0, None) == -1
    assert lib.endo_image_warp_bwd(p(), p(), p(), p(), p(), p(), p(), 1, 1, 4, 4, 0, None) == -1
    # sizes and the padding mode are checked before a pointer is touched: these are host addresses no kernel may see
    import ctypes
    buf = ctypes.create_string_buffer(64)
    a = ctypes.c_void_p(ctypes.addressof(buf))
    for n, c, h, w, mode in ((0, 1, 4, 4, 0), (1, 0, 4, 4, 0), (1, 1, 0, 4, 0), (1, 1, 4, -1, 0), (1, 1, 4, 4, 3), (1, 1, 4, 4, -1),
                             (1, 1, 1 << 16, 1 << 16, 0)):
        assert lib.endo_image_warp_fwd(a, a, a, a, n, c, h, w, mode, None) == -1, (n, c, h, w, mode)
        assert lib.endo_image_warp_bwd(a, a, a, a, a, a, a, n, c, h, w, mode, None) == -1, (n, c, h, w, mode)
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 1 << 16, 1 << 16)):
        assert lib.endo_warp_coordinates_fwd(a, a, a, a, a, a, a, n, h, w, None) == -1
        assert lib.endo_warp_coordinates_bwd(a, a, a, a, a, a, a, a, n, h, w, None) == -1


def test_cpu_tensors_are_refused():
    images, u, v = torch.zeros(1, 3, 4, 5), torch.zeros(1, 4, 5), torch.zeros(20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.images_warping(images, u, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea._bilinear_interpolate(images.permute(0, 2, 3, 1), u, v, padding_mode="border")
    d = torch.ones(1, 4, 5, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea._warp_coordinate_generate(d, d, torch.zeros(1, 3, 1), torch.eye(3).reshape(1, 3, 3), torch.eye(3).reshape(1, 3, 3))


def test_bad_arguments_raise_value_error():
    images, u, v = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5), torch.zeros(40)
    with pytest.raises(ValueError, match="padding_mode"):
        ea.images_warping(images, u, v, padding_mode="mirror")
    with pytest.raises(ValueError, match="padding_mode"):
        ea._bilinear_interpolate(images.permute(0, 2, 3, 1), u, v, padding_mode="nearest")
    with pytest.raises(ValueError):
        ea.images_warping(images, u[:1], v)
    with pytest.raises(ValueError):
        ea.images_warping(images, u, torch.zeros(41))
    with pytest.raises(ValueError):
        ea.images_warping(images[0], u, v)
    d = torch.ones(2, 4, 5, 1)
    pose = (torch.zeros(2, 3, 1), torch.eye(3).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1))
    with pytest.raises(ValueError):
        ea._warp_coordinate_generate(d.permute(0, 3, 1, 2), d, *pose)
    with pytest.raises(ValueError):
        ea._warp_coordinate_generate(d, d[:1], *pose)
    with pytest.raises(RuntimeError, match="no gradient"):
        ea._warp_coordinate_generate(d, d.clone().requires_grad_(True), *pose)
    with pytest.raises(RuntimeError, match="no gradient"):
        ea._warp_coordinate_generate(d, d, pose[0].clone().requires_grad_(True), pose[1], pose[2])
