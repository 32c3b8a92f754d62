"""The six loss modules that finish the reference's losses.py (NormalizedWeightedMaskedL2Loss, SparseMaskedL1LossDisplay, MaskedL1Loss,
NormalizedL2Loss, NormalizedL1Loss, MaskedScaleInvariantLoss) on the device, forward and backward, through the drop-in modules:

  * against what the reference's own classes gave (tests/golden/losses_extra_4x16x24.npz), the empty-mask NaN / 0 pattern included;
  * against the fp32 restatement (tests/losses_restate.py) at the smallest shapes on both sides of the kernels' constants -- the ones
    csrc/losses.hip already had: 256 threads x 8 items per reduce block, the apply grid capped at 1024 blocks of 256;
  * gradients that were not requested, the per-sample upstream gradient of the Display form, the workspace contract, and the use the
    modules are for: DepthWarpingLayer -> NormalizedL2Loss / NormalizedL1Loss under autograd.

Bounds (tests/test_gpu_parity.py::test_losses), all max abs error / max |ref|: values 1e-5, the logarithmic loss 2e-5, gradients 1e-4.
Run with ``pytest -m gpu`` on an MI355X."""

import functools
import importlib

import numpy as np
import pytest
import torch

import losses_restate as lr
from guarded_alloc import guarded
from oracle import geometry as ogeo

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

FIXTURE = "losses_extra_4x16x24.npz"
NAMES = sorted(lr.CASES)
GRAD_TOL = 1e-4
# (3, 7, 9): 63 pixels, fewer than a wave; (2, 48, 50): 2400 pixels, two reduce blocks, the second partial, not a multiple of 64;
# (1, 520, 512): 266 240 pixels, past the apply cap of 1024 x 256, so the grid-stride loop takes a partial second pass
SHAPES = [(3, 7, 9), (2, 48, 50), (1, 520, 512)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def value_tol(name):
    return 2e-5 if name == "MaskedScaleInvariantLoss" else 1e-5


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def assert_close(got, want, tol, what):
    err = rel_err(got, want)
    print("%s: max abs err / max |ref| = %.3e (bound %.1e)" % (what, err, tol))
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))
    assert err <= tol, "%s: max abs err / max |ref| = %.3e > %.1e" % (what, err, tol)


def run_module(name, inputs, upstream=None, needs=None):
    """The module ``name`` on device copies of ``inputs``: (value, [gradient or None per differentiable input]).  ``needs``: which of
    the differentiable inputs ask for a gradient (default all)."""
    _, _, ndiff, kw = lr.CASES[name]
    needs = [True] * ndiff if needs is None else needs
    x = [t.to(dev()) for t in inputs]
    for i in range(ndiff):
        x[i].requires_grad_(needs[i])
    value = getattr(ea, name)(**kw)(x)
    if value.dim() == 0:
        value.backward()
    else:
        value.backward(torch.ones_like(value) if upstream is None else upstream.to(dev()))
    return value.detach(), [x[i].grad for i in range(ndiff)]


def fixture_inputs(g, which, names):
    return [torch.from_numpy(np.array(g["%s::%s" % (which, k)])) for k in names]


# ---------------------------------------------------------------------------------------------
# the reference's recorded outputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_main_record(golden, name):
    g = golden(FIXTURE)
    _, names, ndiff, _ = lr.CASES[name]
    upstream = torch.from_numpy(np.array(g["main::display_upstream"])) if name == "SparseMaskedL1LossDisplay" else None
    value, grads = run_module(name, fixture_inputs(g, "main", names), upstream)
    assert_close(value, torch.from_numpy(np.array(g["main::%s::loss" % name])), value_tol(name), name + " value")
    for i in range(ndiff):
        assert_close(grads[i], torch.from_numpy(np.array(g["main::%s::grad%d" % (name, i)])), GRAD_TOL, "%s gradient %d" % (name, i))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_edge_record(golden, name):
    """Sample 1's masks are empty: NaN for the three losses that divide by the mask's sum, 0 for that sample in the others; sample 0's
    translation is zero, so its weight 1e8 makes the weighted loss sample 0's."""
    g = golden(FIXTURE)
    x = [t.to(dev()) for t in fixture_inputs(g, "edge", lr.CASES[name][1])]
    with torch.no_grad():
        value = getattr(ea, name)(**lr.CASES[name][3])(x).cpu().reshape(-1)
    want = torch.from_numpy(np.array(g["edge::%s::loss" % name])).reshape(-1)
    assert torch.equal(torch.isnan(value), torch.isnan(want)), "%s: %s, the reference %s" % (name, value, want)
    finite = ~torch.isnan(want)
    if bool(finite.any()):
        assert_close(value[finite], want[finite], value_tol(name), name + " edge value")


# ---------------------------------------------------------------------------------------------
# the fp32 restatement at the shapes around the kernels' constants
# ---------------------------------------------------------------------------------------------
def make_inputs(n, h, w, seed):
    """Inputs in the fixture's ranges at any shape: every sample has masked pixels in both masks, five exact ties a == b under the
    mask, sparse depth 0 off its mask, one masked sparse depth of 0.3."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    x = {}
    x["mask"] = (rng.random((n, 1, h, w)) < 0.6).astype(f32)
    x["mask"][:, 0, 0, :6] = 1.0
    x["depth"] = rng.uniform(0.3, 0.9, (n, 1, h, w)).astype(f32)
    x["warped"] = (x["depth"] * rng.uniform(0.8, 1.25, (n, 1, h, w)).astype(f32)).astype(f32)
    x["warped"][:, 0, 0, :5] = x["depth"][:, 0, 0, :5]
    x["images"] = rng.uniform(-1.0, 1.0, (n, 3, h, w)).astype(f32)
    x["images_hat"] = (x["images"] + rng.normal(0.0, 0.2, (n, 3, h, w))).astype(f32)
    x["images_hat"][:, :, 0, :3] = x["images"][:, :, 0, :3]
    x["flows"] = rng.normal(0.0, 5.0, (n, 2, h, w)).astype(f32)
    x["flows_hat"] = (x["flows"] + rng.normal(0.0, 1.0, (n, 2, h, w))).astype(f32)
    x["translations"] = rng.standard_normal((n, 3, 1)).astype(f32)
    x["sparse_mask"] = (rng.random((n, 1, h, w)) < 0.05).astype(f32)
    x["sparse_mask"][:, 0, h - 1, w - 3:] = 1.0
    x["flows_hat"][:, :, h - 1, w - 1] = x["flows"][:, :, h - 1, w - 1]
    x["sparse"] = (rng.uniform(0.6, 8.0, (n, 1, h, w)).astype(f32) * x["sparse_mask"]).astype(f32)
    x["sparse"][0, 0, h - 1, w - 2] = f32(0.3)
    x["est"] = rng.uniform(0.5, 8.0, (n, 1, h, w)).astype(f32)
    x["upstream"] = np.linspace(-1.5, 2.0, n).astype(f32) if n > 1 else np.array([0.625], dtype=f32)
    return {k: torch.from_numpy(v) for k, v in x.items()}


@functools.lru_cache(maxsize=None)
def reference(shape):
    """Inputs and the fp32 restatement's values and gradients for every class at ``shape``: computed once, shared, never changed."""
    x = make_inputs(*shape, seed=100 + shape[1])
    ref = {}
    for name in NAMES:
        inputs = [x[k] for k in lr.CASES[name][1]]
        ref[name] = lr.value_and_grads(name, inputs, x["upstream"] if name == "SparseMaskedL1LossDisplay" else None)
    return x, ref


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_at_shapes(shape, name):
    x, ref = reference(shape)
    want, want_grads = ref[name]
    assert bool(torch.isfinite(want).all())
    value, grads = run_module(name, [x[k] for k in lr.CASES[name][1]], x["upstream"])
    assert_close(value, want, value_tol(name), "%s %s value" % (name, shape))
    for i, ref_grad in enumerate(want_grads):
        assert_close(grads[i], ref_grad, GRAD_TOL, "%s %s gradient %d" % (name, shape, i))


@pytest.mark.parametrize("name", [n for n in NAMES if lr.CASES[n][2] == 2])
def test_gradients_not_requested(name):
    """Only one input requires a gradient: the other pointer is null, and the requested gradient is what it is when both are asked."""
    shape = SHAPES[1]
    x, _ = reference(shape)
    inputs = [x[k] for k in lr.CASES[name][1]]
    _, both = run_module(name, inputs, x["upstream"])
    for needs in ([True, False], [False, True]):
        _, grads = run_module(name, inputs, x["upstream"], needs)
        for i in range(2):
            if needs[i]:
                assert torch.equal(grads[i], both[i]), "%s: gradient %d changes when it is the only one requested" % (name, i)
            else:
                assert grads[i] is None


def test_display_per_sample_upstream_gradient():
    """SparseMaskedL1LossDisplay returns the (N,) vector; its backward takes an (N,) gradient, one factor per sample."""
    shape = SHAPES[1]
    x, _ = reference(shape)
    inputs = [x[k] for k in ("flows", "flows_hat", "sparse_mask")]
    upstream = torch.tensor([3.0, -0.25])
    value, grads = run_module("SparseMaskedL1LossDisplay", inputs, upstream)
    assert value.shape == (shape[0],)
    want, want_grads = lr.value_and_grads("SparseMaskedL1LossDisplay", inputs, upstream)
    assert_close(value, want, 1e-5, "display value")
    for i in range(2):
        assert_close(grads[i], want_grads[i], GRAD_TOL, "display gradient %d" % i)
    _, ones = run_module("SparseMaskedL1LossDisplay", inputs, torch.ones(2))
    for n, factor in enumerate(upstream.tolist()):          # sample n's gradient is the all-ones gradient times its own factor
        assert_close(grads[0][n], ones[0][n] * factor, 1e-6, "display gradient of sample %d" % n)


def test_workspace_contract():
    """Forward and backward of all six on poisoned, guarded buffers: no guard byte changes, and the results equal an unpoisoned run's --
    nothing reads what ``stats``, the value or a gradient buffer held on entry, nothing is written past them."""
    shape = SHAPES[1]          # two reduce blocks per sample: a sum of two fp64 terms does not depend on their order
    x, _ = reference(shape)
    plain = {name: run_module(name, [x[k] for k in lr.CASES[name][1]], x["upstream"]) for name in NAMES}
    torch.cuda.synchronize()
    with guarded(device="cuda", fill="poison") as alloc:
        poisoned = {name: run_module(name, [x[k] for k in lr.CASES[name][1]], x["upstream"]) for name in NAMES}
        torch.cuda.synchronize()
        assert alloc.check() >= 3 * len(NAMES)          # stats, the value and at least one gradient per class went through the guard
    for name in NAMES:
        assert torch.equal(poisoned[name][0], plain[name][0]), name + " value"
        assert bool(torch.isfinite(poisoned[name][0]).all()), name
        for i, grad in enumerate(plain[name][1]):
            assert torch.equal(poisoned[name][1][i], grad), "%s gradient %d" % (name, i)


# ---------------------------------------------------------------------------------------------
# DepthWarpingLayer -> the alternative consistency losses, under autograd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NormalizedL2Loss", "NormalizedL1Loss"])
def test_composition_with_depth_warping(name):
    """What the modules are for: the (depth, warped depth, intersect mask) triple of DepthWarpingLayer into the loss, gradients to both
    depth maps through the warp -- against oracle.geometry's warp followed by the restatement, at test_depth_warping's bounds."""
    n, h, w = 2, 32, 40
    batch = ea.synthetic.make_batch(n, h, w, seed=61, sparse_points=min(500, h * w // 6))
    p1 = ea.synthetic.smooth_depth(n, h, w, seed=161)
    p2 = ea.synthetic.smooth_depth(n, h, w, seed=261)
    args = [batch["boundaries"], batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"], batch["intrinsics"]]
    c1, c2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    warped_ref, overlap = ogeo.depth_warping_parts(c1, c2, *args, 1.0e-8)
    # the intersect mask is a threshold at 0.9 (models.py:552); these inputs keep every pixel clear of it, so both sides cut alike
    assert float((overlap.detach() - 0.9).abs().min()) > 1e-4, "choose inputs without a pixel on the intersect threshold"
    inter_ref = (overlap >= 0.9).to(warped_ref.dtype).detach()
    assert 0.2 < float(inter_ref.mean()) < 1.0
    want = lr.CASES[name][0](c1, warped_ref, inter_ref)
    want.backward()
    g1, g2 = p1.to(dev()).requires_grad_(True), p2.to(dev()).requires_grad_(True)
    warped, inter = ea.DepthWarpingLayer(epsilon=1.0e-8)([g1, g2] + [a.to(dev()) for a in args])
    assert torch.equal(inter.cpu(), inter_ref.detach()), "intersect masks differ: the comparison below would not be of the losses"
    loss = getattr(ea, name)()([g1, warped, inter])
    loss.backward()
    assert_close(loss, want, 1e-5, name + " after the warp")
    assert_close(g1.grad, c1.grad, GRAD_TOL, name + " gradient to depth 1")
    assert_close(g2.grad, c2.grad, GRAD_TOL, name + " gradient to depth 2")
