"""The transition-up layers in their nine-product sub-pixel form (csrc/conv_dma_kernels.h: tu_fwd_subpix_kernel, tu_dgrad_subpix_kernel;
csrc/wgrad_subpix_kernels.h) against the fp64 oracle, held to the error of the sixteen-product form they replace.

Every case: forward and backward in train mode; FIRST the pass's own plan must hold the transition-up forms the case exists for; then, on the
activation pattern the pass took, the depth, the gradient of every transition-up weight and bias, and the gradient arriving at the
transitions' source maps -- read off the tensors it alone decides: the convolution weight gradients of the four layers whose new maps a
transition reads (the bottleneck's and the first four up blocks').

Bound: the nine-product form's differences cost rounding (1.6x the rms error of the sixteen-product form on white noise, the worst input).
PARENT holds, per case and tensor, the (max, rms) absolute error against fp64 that the sixteen-product kernels of the parent commit gave on
the same cases and tensors on an MI355X; the new kernels may be at most 2x that, per tensor, on both.  Run with ``pytest -m gpu`` on an MI355X."""

import importlib

import numpy as np
import pytest
import torch

import test_gpu_parity as tp
import test_gpu_plan_forms as forms
import test_plan_coverage as cov
from device_pattern import pattern_of

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

SUBPIX = [("tu_fwd", "Subpix"), ("tu_wgrad", "Subpix")]
# tag: (samples per group, height, width), groups, options, the (kind, form, level) the pass must have taken
CASES = {
    # source widths 48 / 24 / 12 take the sub-pixel form, width 6 the plain one; the level-1 and level-2 launches are partial tiles
    "partial-2x64x96": ((2, 64, 96), 1, {},
                        [(k, f, l) for k, f in SUBPIX for l in (0, 1, 2)] + [("tu_dgrad", "Subpix16x4", 0), ("tu_dgrad", "Subpix16x4", 2), ("tu_dgrad", "Plain", 3)]),
    # whole tiles, the data-gradient tile shapes of the benchmark's plan (tests/test_plan_coverage.py: model-256x320)
    "bench-forms-1x128x192": ((1, 128, 192), 2, {cov.CHIP_DIVISOR: 27},
                              [(k, f, l) for k, f in SUBPIX for l in (0, 1, 2)] + [("tu_dgrad", "Subpix32x8", 0), ("tu_dgrad", "Subpix16x8", 1)]),
    # a source level 2 rows high: every row is a border row of some tile
    "two-rows-2x32x64": ((2, 32, 64), 1, {},
                         [(k, f, l) for k, f in SUBPIX for l in (0, 1, 2, 3)] + [("tu_dgrad", "Subpix16x4", 3)]),
}

TENSORS = (["transUpBlocks.%d.convTrans.1.%s" % (i, part) for i in range(5) for part in ("weight", "bias")] +
           ["bottleneck.bottleneck.layers.%d.conv.weight" % j for j in range(4)] +
           ["denseBlocksUp.%d.layers.%d.conv.weight" % (i, j) for i in range(4) for j in range(4)])

# (max, rms) absolute error against fp64 of the parent commit's sixteen-product kernels: {case: {tensor or "depth": (max, rms)}}
PARENT = {
    "partial-2x64x96": {
        "depth": (6.4829e-06, 1.3744e-06),
        "transUpBlocks.0.convTrans.1.weight": (2.6409e-05, 4.0710e-06),
        "transUpBlocks.0.convTrans.1.bias": (3.5763e-07, 1.2354e-07),
        "transUpBlocks.1.convTrans.1.weight": (3.6428e-05, 6.3984e-06),
        "transUpBlocks.1.convTrans.1.bias": (4.7684e-07, 2.0711e-07),
        "transUpBlocks.2.convTrans.1.weight": (3.9486e-05, 8.7839e-06),
        "transUpBlocks.2.convTrans.1.bias": (9.5367e-07, 3.9290e-07),
        "transUpBlocks.3.convTrans.1.weight": (5.9579e-05, 1.1723e-05),
        "transUpBlocks.3.convTrans.1.bias": (2.0266e-06, 8.3168e-07),
        "transUpBlocks.4.convTrans.1.weight": (1.1304e-04, 1.3690e-05),
        "transUpBlocks.4.convTrans.1.bias": (3.3314e-06, 1.2759e-06),
        "bottleneck.bottleneck.layers.0.conv.weight": (4.3906e-05, 5.1691e-06),
        "bottleneck.bottleneck.layers.1.conv.weight": (3.7091e-05, 4.6421e-06),
        "bottleneck.bottleneck.layers.2.conv.weight": (2.9940e-05, 4.4582e-06),
        "bottleneck.bottleneck.layers.3.conv.weight": (3.5654e-05, 3.9941e-06),
        "denseBlocksUp.0.layers.0.conv.weight": (5.5505e-05, 7.0225e-06),
        "denseBlocksUp.0.layers.1.conv.weight": (4.9302e-05, 6.3490e-06),
        "denseBlocksUp.0.layers.2.conv.weight": (5.2503e-05, 6.6882e-06),
        "denseBlocksUp.0.layers.3.conv.weight": (7.5798e-05, 6.0701e-06),
        "denseBlocksUp.1.layers.0.conv.weight": (7.8704e-05, 9.5762e-06),
        "denseBlocksUp.1.layers.1.conv.weight": (7.7603e-05, 9.7763e-06),
        "denseBlocksUp.1.layers.2.conv.weight": (9.3323e-05, 8.9875e-06),
        "denseBlocksUp.1.layers.3.conv.weight": (6.0177e-05, 8.8354e-06),
        "denseBlocksUp.2.layers.0.conv.weight": (1.0600e-04, 1.3356e-05),
        "denseBlocksUp.2.layers.1.conv.weight": (1.2197e-04, 1.2640e-05),
        "denseBlocksUp.2.layers.2.conv.weight": (9.9149e-05, 1.2282e-05),
        "denseBlocksUp.2.layers.3.conv.weight": (9.7007e-05, 1.1570e-05),
        "denseBlocksUp.3.layers.0.conv.weight": (1.2443e-04, 1.6157e-05),
        "denseBlocksUp.3.layers.1.conv.weight": (1.2232e-04, 1.7220e-05),
        "denseBlocksUp.3.layers.2.conv.weight": (1.5164e-04, 1.5436e-05),
        "denseBlocksUp.3.layers.3.conv.weight": (1.2523e-04, 1.6245e-05),
    },
    "bench-forms-1x128x192": {
        "depth": (1.3731e-05, 2.9173e-06),
        "transUpBlocks.0.convTrans.1.weight": (8.6569e-05, 1.7333e-05),
        "transUpBlocks.0.convTrans.1.bias": (6.5565e-07, 1.9557e-07),
        "transUpBlocks.1.convTrans.1.weight": (1.3578e-04, 2.7644e-05),
        "transUpBlocks.1.convTrans.1.bias": (1.2750e-06, 4.4046e-07),
        "transUpBlocks.2.convTrans.1.weight": (1.7716e-04, 3.8271e-05),
        "transUpBlocks.2.convTrans.1.bias": (2.2685e-06, 8.4820e-07),
        "transUpBlocks.3.convTrans.1.weight": (2.5787e-04, 5.0894e-05),
        "transUpBlocks.3.convTrans.1.bias": (5.0068e-06, 1.8436e-06),
        "transUpBlocks.4.convTrans.1.weight": (4.9324e-04, 6.6259e-05),
        "transUpBlocks.4.convTrans.1.bias": (7.0397e-06, 2.2476e-06),
        "bottleneck.bottleneck.layers.0.conv.weight": (1.2125e-04, 1.8509e-05),
        "bottleneck.bottleneck.layers.1.conv.weight": (1.1055e-04, 1.8018e-05),
        "bottleneck.bottleneck.layers.2.conv.weight": (1.1180e-04, 1.6894e-05),
        "bottleneck.bottleneck.layers.3.conv.weight": (9.7013e-05, 1.7059e-05),
        "denseBlocksUp.0.layers.0.conv.weight": (2.3838e-04, 3.0041e-05),
        "denseBlocksUp.0.layers.1.conv.weight": (2.4207e-04, 2.8387e-05),
        "denseBlocksUp.0.layers.2.conv.weight": (2.2340e-04, 2.8567e-05),
        "denseBlocksUp.0.layers.3.conv.weight": (2.6872e-04, 2.8706e-05),
        "denseBlocksUp.1.layers.0.conv.weight": (3.1803e-04, 4.2888e-05),
        "denseBlocksUp.1.layers.1.conv.weight": (3.4921e-04, 4.2792e-05),
        "denseBlocksUp.1.layers.2.conv.weight": (3.6366e-04, 4.1027e-05),
        "denseBlocksUp.1.layers.3.conv.weight": (3.3393e-04, 3.7993e-05),
        "denseBlocksUp.2.layers.0.conv.weight": (5.0296e-04, 5.6688e-05),
        "denseBlocksUp.2.layers.1.conv.weight": (4.0041e-04, 5.4970e-05),
        "denseBlocksUp.2.layers.2.conv.weight": (3.4645e-04, 5.3501e-05),
        "denseBlocksUp.2.layers.3.conv.weight": (4.1066e-04, 5.0718e-05),
        "denseBlocksUp.3.layers.0.conv.weight": (7.4957e-04, 7.0096e-05),
        "denseBlocksUp.3.layers.1.conv.weight": (4.8591e-04, 7.3833e-05),
        "denseBlocksUp.3.layers.2.conv.weight": (5.4267e-04, 6.9018e-05),
        "denseBlocksUp.3.layers.3.conv.weight": (5.5061e-04, 7.2471e-05),
    },
    "two-rows-2x32x64": {
        "depth": (5.1380e-06, 1.3282e-06),
        "transUpBlocks.0.convTrans.1.weight": (1.8266e-05, 2.5220e-06),
        "transUpBlocks.0.convTrans.1.bias": (3.5763e-07, 1.0783e-07),
        "transUpBlocks.1.convTrans.1.weight": (2.4232e-05, 3.7746e-06),
        "transUpBlocks.1.convTrans.1.bias": (3.5763e-07, 1.3296e-07),
        "transUpBlocks.2.convTrans.1.weight": (2.4416e-05, 4.9586e-06),
        "transUpBlocks.2.convTrans.1.bias": (5.9605e-07, 2.3212e-07),
        "transUpBlocks.3.convTrans.1.weight": (2.9616e-05, 6.4603e-06),
        "transUpBlocks.3.convTrans.1.bias": (1.3113e-06, 4.2673e-07),
        "transUpBlocks.4.convTrans.1.weight": (5.6979e-05, 7.6276e-06),
        "transUpBlocks.4.convTrans.1.bias": (3.1724e-06, 8.7880e-07),
        "bottleneck.bottleneck.layers.0.conv.weight": (7.2063e-05, 3.4244e-06),
        "bottleneck.bottleneck.layers.1.conv.weight": (5.9885e-05, 2.6189e-06),
        "bottleneck.bottleneck.layers.2.conv.weight": (5.7277e-05, 3.0675e-06),
        "bottleneck.bottleneck.layers.3.conv.weight": (7.7221e-05, 2.8667e-06),
        "denseBlocksUp.0.layers.0.conv.weight": (6.9979e-05, 4.2919e-06),
        "denseBlocksUp.0.layers.1.conv.weight": (4.8134e-05, 3.6244e-06),
        "denseBlocksUp.0.layers.2.conv.weight": (5.2703e-05, 3.6523e-06),
        "denseBlocksUp.0.layers.3.conv.weight": (6.4376e-05, 4.0603e-06),
        "denseBlocksUp.1.layers.0.conv.weight": (5.0893e-05, 5.4446e-06),
        "denseBlocksUp.1.layers.1.conv.weight": (4.1005e-05, 5.3437e-06),
        "denseBlocksUp.1.layers.2.conv.weight": (5.0398e-05, 5.3678e-06),
        "denseBlocksUp.1.layers.3.conv.weight": (4.6062e-05, 4.8895e-06),
        "denseBlocksUp.2.layers.0.conv.weight": (5.1157e-05, 7.1956e-06),
        "denseBlocksUp.2.layers.1.conv.weight": (5.2556e-05, 7.1551e-06),
        "denseBlocksUp.2.layers.2.conv.weight": (5.3175e-05, 6.9874e-06),
        "denseBlocksUp.2.layers.3.conv.weight": (5.7257e-05, 6.6407e-06),
        "denseBlocksUp.3.layers.0.conv.weight": (7.3424e-05, 8.8452e-06),
        "denseBlocksUp.3.layers.1.conv.weight": (6.8098e-05, 9.1437e-06),
        "denseBlocksUp.3.layers.2.conv.weight": (7.7056e-05, 8.7358e-06),
        "denseBlocksUp.3.layers.3.conv.weight": (8.6600e-05, 8.7210e-06),
    },
}


def errors(got, want):
    d = got.detach().double().cpu() - want
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


@pytest.mark.parametrize("tag", list(CASES))
def test_nine_products_against_fp64(tag):
    """Measured on an MI355X, new error / the sixteen-product kernels' error over the case's 31 tensors (all in profiles/r07_ab_runs.txt):
        partial-2x64x96         max 0.78 .. 1.25   rms 0.94 .. 1.16      depth 5.9e-6 (parent 6.5e-6)
        bench-forms-1x128x192   max 0.74 .. 1.16   rms 0.88 .. 1.11      depth 1.3e-5 (1.4e-5)
        two-rows-2x32x64        max 0.83 .. 1.36   rms 0.78 .. 1.46      depth 5.3e-6 (5.1e-6)
    The largest ratios are the transition-up biases', whose true gradient is zero (they feed a training-mode BatchNorm): 1e-6 of pure rounding.
    2 s per case, the fp64 oracle nearly all of it."""
    (n, h, w), groups, options, takes = CASES[tag]
    total = n * groups
    with tp.kernel_options(options):
        state, model = tp.make_model(62)
    rng = np.random.default_rng(16)
    x = torch.from_numpy(rng.uniform(-1, 1, (total, 3, h, w)).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((total, 1, h, w)).astype(np.float32))
    model.train()
    y = ea.models._NetFunction.apply(x.to(tp.dev()), model._anchor, model, groups)
    patterns = pattern_of(y, model, n, h, w, groups)
    (y * cot.to(tp.dev())).sum().backward()
    torch.cuda.synchronize()

    cov.assert_takes(model.last_plan(total, h, w, groups, entries=True), takes, tag)

    y64, g64 = [], None
    for grp in range(groups):
        yg, part = forms.oracle_on_pattern(state, x[grp * n:(grp + 1) * n], cot[grp * n:(grp + 1) * n], patterns[grp])
        y64.append(yg)
        g64 = part if g64 is None else {k: g64[k] + part[k] for k in part}
    params = dict(model.named_parameters())
    measured = {"depth": errors(y, torch.cat(y64))}
    for name in TENSORS:
        measured[name] = errors(params[name].grad, g64[name])
    for name, (emax, erms) in measured.items():
        pmax, prms = PARENT.get(tag, {}).get(name, (float("nan"), float("nan")))
        print("TU9 %s %s max %.4e rms %.4e | parent max %.4e rms %.4e | ratio %.2f %.2f" % (tag, name, emax, erms, pmax, prms, emax / pmax, erms / prms))
    assert set(PARENT.get(tag, ())) == set(measured), "no parent figures for %s" % tag
    bad = [(name, measured[name], PARENT[tag][name]) for name in measured
           if not (measured[name][0] <= 2.0 * PARENT[tag][name][0] and measured[name][1] <= 2.0 * PARENT[tag][name][1])]
    assert not bad, "%s: over 2x the sixteen-product form's error against fp64: %s" % (tag, bad)
