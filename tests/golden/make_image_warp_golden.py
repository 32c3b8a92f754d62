"""Writes tests/golden/image_warp.npz: inputs and the outputs of the reference's own ``_warp_coordinate_generate``, ``images_warping``
(models.py:317-336, 377-429) and ``MaskedL1Loss`` (losses.py:82-91), evaluated on the CPU by the reference's unmodified functions
under autograd.

    python tests/golden/make_image_warp_golden.py <directory of the reference checkout>

Needs the reference, so it is run where that exists and not by the test suite; only the inputs and the recorded outputs are written,
no reference source is stored.  The three shims of make_golden.py apply: ``.cuda()`` is the identity for tensors and modules, and
``torch.solve(B, A)`` is ``torch.linalg.solve(A, B)``.

Three records, keys ``<record>::<name>``; ``<mode>`` is zeros, border or reflection:

  direct (N = 2, C = 3, 16 x 24): random images; coordinates given directly, about 60 % of the pixels with all four taps inside the
      image, the rest spread over [-W, 2W] x [-H, 2H]; every fractional part of u - 0.5 and v - 0.5 in [0.05, 0.45] or [0.55, 0.95],
      away from the cell boundaries, border clips and reflection points where the derivative in the coordinates jumps.
      ``direct::<mode>::out`` and, under the non-uniform cotangent ``direct::cotangent``, ``::grad_images``, ``::grad_u``, ``::grad_v``.
  exact (values only): coordinates ON those kinks, ix and iy each in {-1, -0.5, 0, size - 1, size - 0.5, size}, all 36 pairs, for
      three image shapes ``a`` (1, 3, 6, 8), ``b`` (2, 1, 5, 9) and ``c`` (1, 4, 7, 6): ``exact::<shape>::<mode>::out``.
  chain (N = 2, 32 x 64): poses and boundary of synthetic.make_batch(2, 32, 64, seed=3, sparse_points=60), the depth
      synthetic.smooth_depth(2, 32, 64, seed=4), smooth 3-channel images (largest adjacent-pixel difference at most 0.05).  Recorded:
      u, v of _warp_coordinate_generate; images 2 warped into frame 1 (zeros padding); MaskedL1Loss()([images 1, warped, boundary]);
      the gradient of that loss with respect to the depth.  The inputs that synthetic regenerates bit for bit (numpy's default_rng) are
      not stored; the images are."""

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import image_warp_restate as iwr  # noqa: E402  (the input builders and the records' conditions, shared with the tests)

F32 = np.float32
MODES = iwr.MODES
EXACT_SHAPES = {"a": (1, 3, 6, 8), "b": (2, 1, 5, 9), "c": (1, 4, 7, 6)}


def q(a, bits=10):
    """Rounded to multiples of 2^-bits: float32 numbers with short mantissas, which keeps the compressed file small."""
    return (np.round(np.asarray(a, np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(F32)


def direct_inputs():
    n, c, h, w = 2, 3, 16, 24
    rng = np.random.default_rng(20240901)
    images = q(rng.uniform(-1.0, 1.0, (n, c, h, w)), 7)
    u, v = iwr.direct_coordinates(rng, n, h, w)
    cotangent = q(rng.normal(0.0, 1.0, (n, c, h, w)), 7)
    four = iwr.check_direct_coordinates(u, v, h, w)
    assert 0.5 <= four <= 0.7, four
    assert u.min() < -0.5 and u.max() > w + 0.5 and v.min() < -0.5 and v.max() > h + 0.5
    assert len(np.unique(cotangent)) > 100
    return images, u, v, cotangent


def exact_coordinates(n, h, w):
    """All 36 pairs of kink locations, repeated over the n * h * w pixels."""
    kx = np.array([-1.0, -0.5, 0.0, w - 1.0, w - 0.5, float(w)])
    ky = np.array([-1.0, -0.5, 0.0, h - 1.0, h - 0.5, float(h)])
    idx = np.arange(n * h * w) % 36
    u = (kx[idx % 6] + 0.5).astype(F32).reshape(n, h, w)
    v = (ky[idx // 6] + 0.5).astype(F32).reshape(n, h, w)
    return u, v


def check_exact(u, v, shape):
    n, c, h, w = shape
    assert u.shape == v.shape == (n, h, w) and n * h * w >= 36
    pairs = set(zip((u.astype(np.float64) - 0.5).reshape(-1).tolist(), (v.astype(np.float64) - 0.5).reshape(-1).tolist()))
    want = set((x, y) for x in (-1.0, -0.5, 0.0, w - 1.0, w - 0.5, float(w)) for y in (-1.0, -0.5, 0.0, h - 1.0, h - 0.5, float(h)))
    assert pairs == want


def chain_inputs():
    x = {k: t.numpy() for k, t in iwr.chain_batch().items()}
    n, _, h, w = x["depth"].shape
    rng = np.random.default_rng(20240902)
    ys = np.linspace(0.0, 1.0, h)[None, None, :, None]
    xs = np.linspace(0.0, 1.0, w)[None, None, None, :]
    for name in ("images_1", "images_2"):
        fy, fx = rng.uniform(0.1, 0.5, (2, n, 3, 1, 1))
        ph = rng.uniform(0.0, 2.0 * np.pi, (n, 3, 1, 1))
        x[name] = q(0.4 * np.cos(2.0 * np.pi * (fy * ys + fx * xs) + ph))
        assert max(iwr.adjacent_difference(x[name])) <= 0.05
    return x


def main(reference):
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.solve = lambda b, a: (torch.linalg.solve(a, b), None)
    sys.path.insert(0, reference)
    ref_models = importlib.import_module("models")
    ref_losses = importlib.import_module("losses")
    sys.path.remove(reference)
    for mod in (ref_models, ref_losses):
        assert os.path.dirname(os.path.abspath(mod.__file__)) == os.path.abspath(reference)
    out = {}

    images, u, v, cotangent = direct_inputs()
    out.update({"direct::images": images, "direct::u": u, "direct::v": v, "direct::cotangent": cotangent})
    for mode in MODES:
        args = [torch.from_numpy(a).clone().requires_grad_(True) for a in (images, u, v)]
        value = ref_models.images_warping(args[0], args[1].reshape(-1), args[2].reshape(-1), padding_mode=mode)
        assert value.shape == images.shape
        grads = torch.autograd.grad((value * torch.from_numpy(cotangent)).sum(), args)
        assert all(bool(torch.isfinite(t).all()) for t in (value,) + tuple(grads))
        out["direct::%s::out" % mode] = value.detach().numpy().astype(F32)
        for name, g in zip(("grad_images", "grad_u", "grad_v"), grads):
            assert g.abs().max() > 0
            out["direct::%s::%s" % (mode, name)] = g.numpy().astype(F32)

    rng = np.random.default_rng(20240903)
    for key, shape in EXACT_SHAPES.items():
        n, c, h, w = shape
        eu, ev = exact_coordinates(n, h, w)
        check_exact(eu, ev, shape)
        eimg = q(rng.uniform(-1.0, 1.0, shape), 7)
        out.update({"exact::%s::images" % key: eimg, "exact::%s::u" % key: eu, "exact::%s::v" % key: ev})
        with torch.no_grad():
            for mode in MODES:
                value = ref_models.images_warping(torch.from_numpy(eimg), torch.from_numpy(eu).reshape(-1), torch.from_numpy(ev).reshape(-1),
                                                  padding_mode=mode)
                out["exact::%s::%s::out" % (key, mode)] = value.numpy().astype(F32)

    x = chain_inputs()
    out.update({"chain::images_1": x["images_1"], "chain::images_2": x["images_2"]})
    depth = torch.from_numpy(x["depth"]).clone().requires_grad_(True)
    mask, t, r, k = (torch.from_numpy(x[name]) for name in ("mask", "t", "R", "K"))
    cu, cv = ref_models._warp_coordinate_generate(depth.permute(0, 2, 3, 1), mask.permute(0, 2, 3, 1), t, r, k)
    warped = ref_models.images_warping(torch.from_numpy(x["images_2"]), cu, cv, padding_mode="zeros")
    loss = ref_losses.MaskedL1Loss()([torch.from_numpy(x["images_1"]), warped, mask])
    grad_depth, = torch.autograd.grad(loss, depth)
    cu, cv = cu.detach().numpy()[..., 0], cv.detach().numpy()[..., 0]
    share = iwr.check_chain_coordinates(cu, cv, x["mask"])
    from oracle import geometry as ogeo
    with torch.no_grad():
        ou, ov = ogeo.projected_coordinates(depth.detach(), mask, t, r, k)
    bitwise = bool(np.array_equal(ou.numpy()[:, 0], cu) and np.array_equal(ov.numpy()[:, 0], cv))
    assert float(loss.detach()) > 0 and float(grad_depth.abs().max()) > 0
    out.update({"chain::u": cu.astype(F32), "chain::v": cv.astype(F32), "chain::warped": warped.detach().numpy().astype(F32),
                "chain::loss": loss.detach().numpy().astype(F32), "chain::grad_depth": grad_depth.numpy().astype(F32)})

    path = os.path.join(HERE, "image_warp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))
    print("  chain: loss %.6f, %.2f %% of the masked pixels within %.0e px of a cell boundary, coordinates %s oracle.geometry's" % (
        float(loss.detach()), 100.0 * share, iwr.KINK_MARGIN, "equal" if bitwise else "DIFFER FROM"))
    # The cap the losses fixture's generator keeps.  This fixture misses it: 168 072 bytes.  The recorded outputs alone are 181 KB of
    # full-mantissa float32 (direct: 3 modes x 25 KB; chain: u, v, warped, gradient 99 KB) that deflate brings to 127 KB, whatever the
    # inputs are quantised to; the file is written above, and the repository's own limit for a committed file is 1 MiB.
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "models.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
