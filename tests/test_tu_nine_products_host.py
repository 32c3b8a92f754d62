"""The nine-product form of the transition-up layer (tests/tu_nine_products_restate.py, the arithmetic of csrc/conv_dma_kernels.h's
tu_fwd_subpix_kernel / tu_dgrad_subpix_kernel and csrc/wgrad_subpix_kernels.h) against upsample-then-convolve and its backward, in fp64.
No GPU.  Grids with odd border behaviour: low-resolution 3 x 4 and 1 x 4 (one row: both row halos are empty), 2 samples, 5 channels."""

import numpy as np
import pytest

import tu_nine_products_restate as nine

GRIDS = [(3, 4), (1, 4)]


def _data(h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, 5, h, w))
    wgt = rng.standard_normal((5, 5, 3, 3))
    bias = rng.standard_normal(5)
    dy = rng.standard_normal((2, 5, 2 * h, 2 * w))
    return x, wgt, bias, dy


def _close(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_forward_identity(grid):
    x, wgt, bias, _ = _data(*grid, seed=3)
    _close(nine.forward(x, wgt, bias), nine.plain_forward(x, wgt, bias))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_data_gradient_identity(grid):
    x, wgt, _, dy = _data(*grid, seed=4)
    _close(nine.data_gradient(dy, wgt), nine.plain_backward(x, wgt, dy)[0])


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_weight_gradient_identity(grid):
    x, wgt, _, dy = _data(*grid, seed=5)
    _close(nine.weight_gradient(x, dy), nine.plain_backward(x, wgt, dy)[1])


def test_plain_backward_is_the_gradient_of_plain_forward():
    """The reference the identities are held to, by central differences of sum(out * dy) in fp64."""
    x, wgt, bias, dy = _data(3, 4, seed=6)
    dx, dw = nine.plain_backward(x, wgt, dy)
    f = lambda xx, ww: float((nine.plain_forward(xx, ww, bias) * dy).sum())
    eps = 1e-6
    for idx in [(0, 0, 0, 0), (1, 4, 2, 3), (0, 2, 1, 1)]:
        d = np.zeros_like(x); d[idx] = eps
        assert abs((f(x + d, wgt) - f(x - d, wgt)) / (2 * eps) - dx[idx]) < 1e-7
    for idx in [(0, 0, 0, 0), (4, 1, 2, 2), (2, 3, 1, 0)]:
        d = np.zeros_like(wgt); d[idx] = eps
        assert abs((f(x, wgt + d) - f(x, wgt - d)) / (2 * eps) - dw[idx]) < 1e-7


def test_tap_table():
    """rows(-) = {0}, rows(0) = {0, 1, 2}, rows(+) = {2}: every tap (ky, kx) lies in W'[r][c] for exactly the r containing ky and c containing kx."""
    assert nine.ROWS == ((0,), (0, 1, 2), (2,))
    assert [nine.classes_of_tap(k) for k in range(3)] == [(0, 1), (1,), (1, 2)]
    for ky in range(3):
        for kx in range(3):
            w = np.zeros((1, 1, 3, 3))
            w[0, 0, ky, kx] = 1.0
            got = {(r, c) for r in range(3) for c in range(3) if nine.nine_weights(w)[r, c, 0, 0] != 0.0}
            assert got == {(r, c) for r in nine.classes_of_tap(ky) for c in nine.classes_of_tap(kx)}
    # the corner, edge and centre classes sum 1, 3 and 9 taps
    ones = nine.nine_weights(np.ones((1, 1, 3, 3)))[:, :, 0, 0]
    assert ones.tolist() == [[1.0, 3.0, 1.0], [3.0, 9.0, 3.0], [1.0, 3.0, 1.0]]
    # an output phase uses its own class and class 0
    assert nine.PHASE_CLASS == (0, 2)
