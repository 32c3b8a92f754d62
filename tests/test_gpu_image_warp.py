"""The reference's image warping (models.py:317-336, 377-429) on the device, forward and backward, through images_warping,
_bilinear_interpolate and _warp_coordinate_generate:

  * against what the reference's own functions gave (tests/golden/image_warp.npz): the ``direct`` record in the three padding modes,
    values and all three gradients, no pixel excluded; the ``exact`` record with coordinates on the kinks, values; the ``chain`` record
    depth -> coordinates -> warped images -> MaskedL1Loss -> depth gradient;
  * against the fp32 restatement (tests/image_warp_restate.py) at the smallest shapes on both sides of the kernels' constants: fewer
    pixels than a wave, planes that are no multiple of 64, and one plane past the launch's cap of 1024 blocks of 256;
  * gradients that were not requested, non-finite coordinates under the guarded allocator, the workspace contract.

Bounds, all max abs error / max |ref|, the project's own for the same arithmetic: coordinates 1e-5 (test_flow_from_depth), sampled
values 5e-5 (test_depth_warping), gradients 1e-4.  The image gradient arrives by fp32 atomics whose order is not fixed: where two runs
of it are compared with each other the bound is 1e-6 (a few additions of rounding 6e-8 each), everything else is compared bit for bit.
Run with ``pytest -m gpu`` on an MI355X."""

import functools
import importlib
import os

import numpy as np
import pytest
import torch

import image_warp_restate as iwr
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

FIXTURE = "image_warp.npz"
COORD_TOL, VALUE_TOL, GRAD_TOL, ATOMIC_ORDER_TOL = 1e-5, 5e-5, 1e-4, 1e-6
EXACT_SHAPES = ("a", "b", "c")
# (3, 3, 7, 9): 63 pixels per plane, fewer than a wave; (2, 1 / 4, 37, 53): 1961 pixels, eight blocks, the last partial, no multiple of
# 64; (1, 1, 513, 512): 262 656 pixels, past the cap of 1024 blocks x 256 threads, so the grid-stride loop takes a partial second pass
SHAPES = [(3, 3, 7, 9), (2, 1, 37, 53), (2, 4, 37, 53), (1, 1, 513, 512)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def assert_close(got, want, tol, what):
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))
    err = rel_err(got, want)
    print("%s: max abs err / max |ref| = %.3e (bound %.1e)" % (what, err, tol))
    assert err <= tol, "%s: max abs err / max |ref| = %.3e > %.1e" % (what, err, tol)


def arr(g, key):
    return torch.from_numpy(np.array(g[key]))


def run_warp(images, u, v, mode, cotangent=None, needs=(True, True, True)):
    """images_warping on device copies: (output, [gradient or None for images, u, v])."""
    args = [a.to(dev()).requires_grad_(bool(need)) for a, need in zip((images, u, v), needs)]
    out = ea.images_warping(args[0], args[1], args[2], padding_mode=mode)
    if cotangent is None:
        return out.detach(), [None, None, None]
    out.backward(cotangent.to(dev()))
    return out.detach(), [a.grad for a in args]


@pytest.mark.parametrize("mode", iwr.MODES)
def test_direct_record(golden, mode):
    g = golden(FIXTURE)
    images, u, v, cot = (arr(g, "direct::" + k) for k in ("images", "u", "v", "cotangent"))
    out, grads = run_warp(images, u, v, mode, cot)
    assert_close(out, arr(g, "direct::%s::out" % mode), VALUE_TOL, "direct %s output" % mode)
    for name, got in zip(("grad_images", "grad_u", "grad_v"), grads):
        assert_close(got, arr(g, "direct::%s::%s" % (mode, name)), GRAD_TOL, "direct %s %s" % (mode, name))
    # the NHWC form is the same call between two permutes
    nhwc = ea._bilinear_interpolate(images.permute(0, 2, 3, 1).to(dev()), u.reshape(-1).to(dev()), v.reshape(-1).to(dev()), padding_mode=mode)
    assert nhwc.shape == (2, 16, 24, 3) and torch.equal(nhwc.permute(0, 3, 1, 2), out)


@pytest.mark.parametrize("mode", iwr.MODES)
def test_exact_record(golden, mode):
    g = golden(FIXTURE)
    for key in EXACT_SHAPES:
        images, u, v = (arr(g, "exact::%s::%s" % (key, k)) for k in ("images", "u", "v"))
        out, _ = run_warp(images, u, v, mode)
        assert_close(out, arr(g, "exact::%s::%s::out" % (key, mode)), VALUE_TOL, "exact %s %s output" % (key, mode))


@functools.lru_cache(maxsize=None)
def chain_on_device():
    """The chain once: depth -> coordinates -> images 2 warped into frame 1 -> MaskedL1Loss under the boundary -> depth gradient."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", FIXTURE), allow_pickle=False)
    x = {k: t.to(dev()) for k, t in iwr.chain_batch().items()}
    depth = x["depth"].clone().requires_grad_(True)
    u, v = ea._warp_coordinate_generate(depth.permute(0, 2, 3, 1), x["mask"].permute(0, 2, 3, 1), x["t"], x["R"], x["K"])
    warped = ea.images_warping(arr(g, "chain::images_2").to(dev()), u, v, padding_mode="zeros")
    loss = ea.MaskedL1Loss()([arr(g, "chain::images_1").to(dev()), warped, x["mask"]])
    loss.backward()
    return g, x, u.detach(), v.detach(), warped.detach(), loss.detach(), depth.grad


def test_chain_coordinates():
    g, x, u, v, _, _, _ = chain_on_device()
    assert u.shape == v.shape == (2, 32, 64, 1)
    assert_close(u[..., 0], arr(g, "chain::u"), COORD_TOL, "chain u")
    assert_close(v[..., 0], arr(g, "chain::v"), COORD_TOL, "chain v")
    # FlowfromDepthLayer is the same code with ((u - x) / W, (v - y) / H) behind it (W, H device scalars: a true division, as in the kernel)
    flow = ea.FlowfromDepthLayer()([x["depth"], x["mask"], x["t"], x["R"], x["K"]])
    xs = torch.arange(64, dtype=torch.float32, device=dev()).reshape(1, 1, 64)
    ys = torch.arange(32, dtype=torch.float32, device=dev()).reshape(1, 32, 1)
    fu, fv = (u[..., 0] - xs) / torch.tensor(64.0, device=dev()), (v[..., 0] - ys) / torch.tensor(32.0, device=dev())
    print("chain flow from the coordinates: %d of %d values differ from FlowfromDepthLayer's" % (
        int((fu != flow[:, 0]).sum()) + int((fv != flow[:, 1]).sum()), flow.numel()))
    assert torch.equal(fu, flow[:, 0]) and torch.equal(fv, flow[:, 1])


def test_chain_warped_images():
    """5e-5 of max |ref| for the sampler, plus what the admitted coordinate error (1e-5 of max |u|, max |v|) can move a bilinear sample
    of an image whose adjacent pixels differ by at most (L_x, L_y)."""
    g, _, _, _, warped, _, _ = chain_on_device()
    want = arr(g, "chain::warped")
    l_x, l_y = iwr.adjacent_difference(np.array(g["chain::images_2"]))
    bound = VALUE_TOL * float(want.abs().max()) + COORD_TOL * (float(np.abs(g["chain::u"]).max()) * l_x + float(np.abs(g["chain::v"]).max()) * l_y)
    err = float((warped.cpu().double() - want.double()).abs().max())
    print("chain warped images: max abs err %.3e (bound %.3e; L_x %.4f, L_y %.4f)" % (err, bound, l_x, l_y))
    assert warped.shape == want.shape and err <= bound


def test_chain_loss():
    g, _, _, _, _, loss, _ = chain_on_device()
    assert_close(loss.reshape(()), arr(g, "chain::loss").reshape(()), 1e-5, "chain MaskedL1Loss")


def test_chain_depth_gradient():
    """Outside the pixels whose reference source location lies within 2e-3 px of a cell boundary in x or y (above the admitted
    coordinate error of 1e-5 x 57 px: there the two sides may pick different cells, and the derivative jumps); at most 2 % of the masked
    pixels are excluded."""
    g, x, _, _, _, _, grad = chain_on_device()
    near = iwr.near_cell_boundary(np.array(g["chain::u"]), np.array(g["chain::v"]))
    masked = x["mask"][:, 0].cpu().numpy() > 0.5
    share = float(near[masked].mean())
    print("chain depth gradient: %.2f %% of the masked pixels excluded" % (100.0 * share))
    assert share <= iwr.KINK_SHARE
    keep = torch.from_numpy(~near)
    want = arr(g, "chain::grad_depth")[:, 0]
    assert grad.shape == (2, 1, 32, 64) and float(want[keep].abs().max()) > 0
    assert_close(grad[:, 0].cpu()[keep], want[keep], GRAD_TOL, "chain depth gradient")


@functools.lru_cache(maxsize=None)
def restatement_case(shape):
    """Inputs built like the direct record's and the restatement's outputs in the three modes, computed once on the CPU."""
    n, c, h, w = shape
    rng = np.random.default_rng(1000 + h * w + c)
    u, v = iwr.direct_coordinates(rng, n, h, w)
    iwr.check_direct_coordinates(u, v, h, w)
    images = torch.from_numpy(rng.uniform(-1.0, 1.0, shape).astype(np.float32))
    cot = torch.from_numpy(rng.normal(0.0, 1.0, shape).astype(np.float32))
    u, v = torch.from_numpy(u), torch.from_numpy(v)
    return images, u, v, cot, {mode: iwr.value_and_grads(images, u, v, mode, cot) for mode in iwr.MODES}


@pytest.mark.parametrize("mode", iwr.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_restatement(shape, mode):
    images, u, v, cot, ref = restatement_case(shape)
    want_out, want_grads = ref[mode]
    out, grads = run_warp(images, u, v, mode, cot)
    assert_close(out, want_out, VALUE_TOL, "%s %s output" % (shape, mode))
    for name, got, want in zip(("grad_images", "grad_u", "grad_v"), grads, want_grads):
        assert_close(got, want, GRAD_TOL, "%s %s %s" % (shape, mode, name))


@pytest.mark.parametrize("mode", iwr.MODES)
def test_gradient_subsets(mode):
    """Images only, coordinates only, u only: None for the rest, and what is asked for is what the full backward gave."""
    images, u, v, cot, _ = restatement_case(SHAPES[2])
    out, full = run_warp(images, u, v, mode, cot)
    for needs in ((True, False, False), (False, True, True), (False, True, False)):
        out_s, grads = run_warp(images, u, v, mode, cot, needs)
        assert torch.equal(out_s, out)
        for i, (need, got) in enumerate(zip(needs, grads)):
            if not need:
                assert got is None, (needs, i)
            elif i == 0:
                assert rel_err(got, full[0]) <= ATOMIC_ORDER_TOL
            else:
                assert torch.equal(got, full[i]), (needs, i)


@pytest.mark.parametrize("mode", iwr.MODES)
def test_non_finite_coordinates(mode):
    """NaN, +inf, -inf and 1e30 at a few coordinates, under the guarded allocator.  A pixel whose source location is not finite gives 0
    and zero coordinate gradients in every mode; 1e30 is a finite location: no tap in range under zeros padding (0, zero gradients),
    the clipped border pixel under border padding (zero gradient in that coordinate), some pixel of the image under reflection.  Every
    other pixel equals the run without them, the image gradient stays finite, and no guard band is touched."""
    images, u, v, cot, _ = restatement_case(SHAPES[2])
    n, c, h, w = images.shape
    bad_u, bad_v = u.clone(), v.clone()
    bad_u[0, 0, 0], bad_v[0, 0, 1], bad_u[0, 0, 2], bad_v[1, 3, 4] = float("nan"), float("inf"), float("-inf"), float("nan")
    bad_u[0, 0, 3] = 1.0e30
    bad_v[1, 5, 6] = 1.0e30
    nonfinite = torch.zeros(n, h, w, dtype=torch.bool)
    nonfinite[0, 0, 0:3] = True
    nonfinite[1, 3, 4] = True
    huge = torch.zeros(n, h, w, dtype=torch.bool)
    huge[0, 0, 3] = huge[1, 5, 6] = True
    out, grads = run_warp(images, u, v, mode, cot)
    with guarded("cuda") as guard:
        out_b, grads_b = run_warp(images, bad_u, bad_v, mode, cot)          # raises unless both calls return 0
        torch.cuda.synchronize()
        assert guard.check() >= 4
    out, out_b = out.cpu(), out_b.cpu()
    gi, gu, gv = (t.cpu() for t in grads)
    gi_b, gu_b, gv_b = (t.cpu() for t in grads_b)
    pix = nonfinite[:, None].expand(n, c, h, w)
    assert bool((out_b[pix] == 0).all()) and bool((gu_b[nonfinite] == 0).all()) and bool((gv_b[nonfinite] == 0).all())
    if mode == "zeros":
        hp = huge[:, None].expand(n, c, h, w)
        assert bool((out_b[hp] == 0).all()) and bool((gu_b[huge] == 0).all()) and bool((gv_b[huge] == 0).all())
    elif mode == "border":
        assert float(gu_b[0, 0, 3]) == 0 and float(gv_b[1, 5, 6]) == 0
    rest = ~(nonfinite | huge)
    assert torch.equal(out_b[rest[:, None].expand(n, c, h, w)], out[rest[:, None].expand(n, c, h, w)])
    assert torch.equal(gu_b[rest], gu[rest]) and torch.equal(gv_b[rest], gv[rest])
    assert bool(torch.isfinite(out_b).all()) and bool(torch.isfinite(gi_b).all()) and bool(torch.isfinite(gu_b).all()) and bool(torch.isfinite(gv_b).all())
    if mode == "zeros":          # the affected pixels scatter nothing: the image gradient is the other run's minus their contributions
        _, only = run_warp(images, torch.where(rest, u, torch.full_like(u, -100.0)), torch.where(rest, v, torch.full_like(v, -100.0)), mode, cot)
        assert rel_err(gi_b, only[0]) <= ATOMIC_ORDER_TOL


def test_workspace_contract():
    """All outputs of the four entry points, grad_images included, pre-filled with NaN: identical to the zero-filled twin."""
    images, u, v, cot, _ = restatement_case(SHAPES[2])
    n, c, h, w = images.shape
    lib, p, s = ea._lib.load(), ea._lib.ptr, ea._lib.stream()
    images, u, v, cot = (t.to(dev()).contiguous() for t in (images, u, v, cot))
    x = {k: t.to(dev()).contiguous() for k, t in iwr.chain_batch().items()}
    cn, _, ch, cw = x["depth"].shape
    t, r, k = x["t"].reshape(cn, 3).contiguous(), x["R"].reshape(cn, 9).contiguous(), x["K"].reshape(cn, 9).contiguous()
    gcoord = torch.randn(cn, ch, cw, device=dev(), generator=torch.Generator(device=dev()).manual_seed(3))
    results = []
    for fill in (float("nan"), 0.0):
        outs = []
        for mode in range(3):
            warped, gi = torch.full_like(images, fill), torch.full_like(images, fill)
            gu, gv = torch.full_like(u, fill), torch.full_like(v, fill)
            assert lib.endo_image_warp_fwd(p(images), p(u), p(v), p(warped), n, c, h, w, mode, s) == 0
            assert lib.endo_image_warp_bwd(p(cot), p(images), p(u), p(v), p(gi), p(gu), p(gv), n, c, h, w, mode, s) == 0
            outs += [warped, gi, gu, gv]
        cu, cv, gd = (torch.full((cn, ch, cw), fill, device=dev()) for _ in range(3))
        assert lib.endo_warp_coordinates_fwd(p(x["depth"]), p(x["mask"]), p(t), p(r), p(k), p(cu), p(cv), cn, ch, cw, s) == 0
        assert lib.endo_warp_coordinates_bwd(p(gcoord), None, p(x["depth"]), p(x["mask"]), p(t), p(r), p(k), p(gd), cn, ch, cw, s) == 0
        results.append(outs + [cu, cv, gd])
    torch.cuda.synchronize()
    for i, (poisoned, zeroed) in enumerate(zip(*results)):
        assert bool(torch.isfinite(poisoned).all()), i
        if i < 12 and i % 4 == 1:          # grad_images: atomics
            assert rel_err(poisoned, zeroed) <= ATOMIC_ORDER_TOL, i
        else:
            assert torch.equal(poisoned, zeroed), i
    # a null cotangent is zero: u's alone plus v's alone is both together
    gd_u, gd_v, gd_uv = (torch.empty(cn, ch, cw, device=dev()) for _ in range(3))
    assert lib.endo_warp_coordinates_bwd(p(gcoord), None, p(x["depth"]), p(x["mask"]), p(t), p(r), p(k), p(gd_u), cn, ch, cw, s) == 0
    assert lib.endo_warp_coordinates_bwd(None, p(gcoord), p(x["depth"]), p(x["mask"]), p(t), p(r), p(k), p(gd_v), cn, ch, cw, s) == 0
    assert lib.endo_warp_coordinates_bwd(p(gcoord), p(gcoord), p(x["depth"]), p(x["mask"]), p(t), p(r), p(k), p(gd_uv), cn, ch, cw, s) == 0
    assert rel_err(gd_u + gd_v, gd_uv) <= 1e-5
