"""The kernel forms the benchmark grids take, at grids the fp64 oracle can afford (tests/test_plan_coverage.py: ADDED_CASES and why each is there).

Every case: forward and backward in train mode; FIRST the pass's own plan (FCDenseNet57.last_plan) must hold the forms the case exists for and equal
what the CPU query promised for it; then depth and all 210 parameter gradients against the fp64 oracle on the activation pattern the pass took, as
test_network_backward_kernel_forms does and with its bounds: depth 1e-5 of its maximum, gradients GRAD_TOL (5e-5 where the plan holds the
F(4x4, 3x3) forward); with bf16 operands the bounds of test_bf16_operand_mode_on_pattern.  Run with ``pytest -m gpu`` on an MI355X."""

import importlib

import numpy as np
import pytest
import torch

import test_gpu_parity as tp
import test_plan_coverage as cov
from device_pattern import pattern_of
from guarded_alloc import guarded
from oracle import network as onet

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
TEST = "test_gpu_plan_forms.test_forms_against_fp64"


def oracle_on_pattern(state, x, cot, pattern):
    """fp64 depth and parameter gradients of one sample group on the branch the HIP pass took."""
    st = tp.state_as(state, torch.float64)
    names = onet.trainable_names()
    for nm in names:
        st[nm].requires_grad_(True)
    y = onet.forward(st, x.double(), training=True, pattern=pattern)
    grads = torch.autograd.grad((y * cot.double()).sum(), [st[nm] for nm in names])
    return y.detach(), dict(zip(names, grads))


def on_device(x, offset_bytes):
    """x on the GPU, its first element `offset_bytes` past an allocation's (256-byte aligned) start."""
    if not offset_bytes:
        return x.to(tp.dev())
    assert offset_bytes % 4 == 0
    buf = torch.empty(x.numel() + offset_bytes // 4, dtype=torch.float32, device=tp.dev())
    view = buf[offset_bytes // 4:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 256 == offset_bytes
    return view


@pytest.mark.parametrize("c", cov.cases(TEST), ids=lambda c: c.tag)
def test_forms_against_fp64(c):
    """Measured on an MI355X -- depth error / max depth, worst gradient tensor's error / its max (its bound):
        model-256x320       1.6e-6   1.6e-5 (5e-5)      model-512x640        1.8e-6   2.6e-5 (5e-5)
        f34-level-4         1.5e-6   1.6e-5 (5e-5)      f34-level-5          2.1e-6   1.7e-5 (5e-5)
        partial-tiles       1.8e-6   2.8e-5 (5e-5)      direct-32x8          1.3e-6   1.6e-5 (3e-5)
        newmap-vec16        9.0e-7   9.5e-6 (3e-5)      first-wgrad-direct   9.0e-7   9.5e-6 (3e-5)
        first-wgrad-f34     2.2e-6   3.4e-5 (5e-5)      model-256x320-bf16   6.8e-3   9.2e-2 (bf16 operands: 2e-2, 1e-1)
    the figures test_network_backward_kernel_forms states for the same forms at its sizes (depth 0.9e-6 .. 2.2e-6; gradients 0.7e-5 .. 2.2e-5,
    2.0e-5 .. 3.5e-5 with the F(4x4, 3x3) forward): no form missed its bound, none was set here.  The worst tensors are the bottleneck's and the first
    up block's, whose BatchNorm normalises over the fewest values.  0.8 .. 5 s per case, the fp64 oracle nearly all of it."""
    n, h, w = c.shape
    total = n * c.groups
    with tp.kernel_options(c.options):
        state, model = tp.make_model(62)
    rng = np.random.default_rng(16)
    x = torch.from_numpy(rng.uniform(-1, 1, (total, 3, h, w)).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((total, 1, h, w)).astype(np.float32))
    model.train()
    # the tape and the gradient workspace between guard bytes and NaN on entry (tests/guarded_alloc.py): these grids put the benchmark's kernel
    # forms, and blocks that walk long runs of tiles, on buffers a hundred times smaller than the benchmark's
    with guarded(device="cuda") as g:
        y = ea.models._NetFunction.apply(on_device(x, c.x_offset), model._anchor, model, c.groups)
        patterns = pattern_of(y, model, n, h, w, c.groups)
        (y * cot.to(tp.dev())).sum().backward()
        torch.cuda.synchronize()
        g.check()

    plan = model.last_plan(total, h, w, c.groups, entries=True)
    cov.assert_takes(plan, c.takes, c.tag)
    promised = cov.plan_of_case(c)
    assert plan == promised, "the pass planned otherwise than the query: %s" % sorted(set(plan) ^ set(promised), key=str)

    bf16 = cov.mode_of(c.options) == "bf16"
    wino4 = any(kind == "dense_fwd" and form == "Wino4" for kind, form, _ in cov.forms_of(plan))
    depth_tol = tp.BF16_FWD_TOL if bf16 else 1e-5
    grad_tol = tp.BF16_GRAD_TOL if bf16 else 5e-5 if wino4 else tp.GRAD_TOL
    y64, g64 = [], None
    for grp in range(c.groups):
        yg, part = oracle_on_pattern(state, x[grp * n:(grp + 1) * n], cot[grp * n:(grp + 1) * n], patterns[grp])
        y64.append(yg)
        g64 = part if g64 is None else {k: g64[k] + part[k] for k in part}
    y64 = torch.cat(y64)
    print("%s: depth max err / max |depth| = %.2e (bound %.0e)" % (c.tag, tp.rel_err(y, y64), depth_tol))
    worst = tp.assert_grads_on_pattern(dict(model.named_parameters()), g64, None, float("inf"), c.tag)
    print("%s: worst gradient tensor %.2e %s (bound %.0e)" % (c.tag, worst[0][0], worst[0][2], grad_tol))
    tp.assert_close(y, y64, depth_tol, "depth, %s" % c.tag)
    tp.assert_grads_on_pattern(dict(model.named_parameters()), g64, None, grad_tol, c.tag)
