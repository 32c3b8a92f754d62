"""The transition-up layer (nearest x2, then conv3x3 with zero padding; reference models.py:70-80) as NINE products per low-resolution pixel,
restated in numpy from the header comments of csrc/conv_dma_kernels.h (tu_fwd_subpix_kernel, tu_dgrad_subpix_kernel) and
csrc/wgrad_subpix_kernels.h -- and the plain upsample-then-convolve layer with its backward, to hold the three identities against.

Index classes r, c in (0, 1, 2) = (-, 0, +).  ROWS[r] = the original kernel rows summed into class r (columns likewise):
    W'[r][c] = sum over ky in ROWS[r], kx in ROWS[c] of w[:, :, ky, kx]
    X'[r][c] = the separable difference image of x: rows x[y-1] - x[y], x[y], x[y+1] - x[y], then the columns the same way (x = 0 outside)
    M[r][c]  = W'[r][c] X'[r][c];   out(2y + a, 2x + b) = M[ra][cb] + M[ra][0] + M[0][cb] + M[0][0] + bias,  ra = - for a = 0, + for a = 1
No GPU, no library: arrays are (samples, channels, height, width), weights (cout, cin, 3, 3), everything in the dtype given."""

import numpy as np

ROWS = ((0,), (0, 1, 2), (2,))          # kernel rows (and columns) summed into the classes -, 0, +
PHASE_CLASS = (0, 2)                     # output phase a (or b) = 0 uses class -, 1 uses class +; both use class 0


def classes_of_tap(k):
    """The classes whose sum contains kernel row (or column) k."""
    return tuple(r for r in range(3) if k in ROWS[r])


def nine_weights(w):
    """W'[r][c][co][ci]."""
    out = np.zeros((3, 3) + w.shape[:2], w.dtype)
    for r in range(3):
        for c in range(3):
            for ky in ROWS[r]:
                for kx in ROWS[c]:
                    out[r, c] += w[:, :, ky, kx]
    return out


def _shift(x, d, axis):
    """y[i] = x[i + d] along `axis`, zero where i + d is outside."""
    out = np.zeros_like(x)
    n = x.shape[axis]
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    if d > 0:
        src[axis], dst[axis] = slice(d, n), slice(0, n - d)
    elif d < 0:
        src[axis], dst[axis] = slice(0, n + d), slice(-d, n)
    out[tuple(dst)] = x[tuple(src)]
    return out


def _difference(x, axis):
    """(x[i-1] - x[i], x[i], x[i+1] - x[i]) along `axis`."""
    return (_shift(x, -1, axis) - x, x, _shift(x, 1, axis) - x)


def input_transform(x):
    """X'[r][c] of the low-resolution input."""
    return [[xc for xc in _difference(xr, 3)] for xr in _difference(x, 2)]


def forward(x, w, bias):
    wp = nine_weights(w)
    xt = input_transform(x)
    m = [[np.einsum("oi,nihw->nohw", wp[r, c], xt[r][c]) for c in range(3)] for r in range(3)]
    n, _, h, wd = x.shape
    out = np.zeros((n, w.shape[0], 2 * h, 2 * wd), x.dtype)
    for a in range(2):
        for b in range(2):
            ra, cb = PHASE_CLASS[a], PHASE_CLASS[b]
            out[:, :, a::2, b::2] = m[ra][cb] + m[ra][1] + m[1][cb] + m[1][1]
    return out + bias[None, :, None, None]


def _combine(g0, g1):
    return (g0, g0 + g1, g1)


def output_gradient_transform(dy):
    """Gt[r][c] = dM[r][c]: rows g0, g0 + g1, g1 of the four stride-2 phase planes of dy; columns likewise."""
    rows = _combine(dy[:, :, 0::2, :], dy[:, :, 1::2, :])
    return [list(_combine(g[:, :, :, 0::2], g[:, :, :, 1::2])) for g in rows]


def weight_gradient(x, dy):
    xt = input_transform(x)
    gt = output_gradient_transform(dy)
    dw = np.zeros((dy.shape[1], x.shape[1], 3, 3), x.dtype)
    for r in range(3):
        for c in range(3):
            dwp = np.einsum("nohw,nihw->oi", gt[r][c], xt[r][c])
            for ky in ROWS[r]:
                for kx in ROWS[c]:
                    dw[:, :, ky, kx] += dwp
    return dw


def _adjoint_rows(g0, g1, axis):
    """T- = g0[i+1] - g0[i], T0 = g0[i] + g1[i], T+ = g1[i-1] - g1[i] along `axis`."""
    return (_shift(g0, 1, axis) - g0, g0 + g1, _shift(g1, -1, axis) - g1)


def data_gradient(dy, w):
    wp = nine_weights(w)
    rows = _adjoint_rows(dy[:, :, 0::2, :], dy[:, :, 1::2, :], 2)
    dx = 0
    for r in range(3):
        cols = _adjoint_rows(rows[r][:, :, :, 0::2], rows[r][:, :, :, 1::2], 3)
        for c in range(3):
            dx = dx + np.einsum("oi,nohw->nihw", wp[r, c], cols[c])
    return dx


# ---------------------------------------------------------------------------------------------
# the plain layer
# ---------------------------------------------------------------------------------------------
def upsample(x):
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)


def conv3x3(u, w, bias):
    n, _, h, wd = u.shape
    pad = np.zeros(u.shape[:2] + (h + 2, wd + 2), u.dtype)
    pad[:, :, 1:-1, 1:-1] = u
    out = np.zeros((n, w.shape[0], h, wd), u.dtype)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oi,nihw->nohw", w[:, :, ky, kx], pad[:, :, ky:ky + h, kx:kx + wd])
    return out + bias[None, :, None, None]


def plain_forward(x, w, bias):
    return conv3x3(upsample(x), w, bias)


def plain_backward(x, w, dy):
    """(d input, d weight) of plain_forward."""
    u = upsample(x)
    n, _, h, wd = u.shape
    pad_u = np.zeros(u.shape[:2] + (h + 2, wd + 2), u.dtype)
    pad_u[:, :, 1:-1, 1:-1] = u
    du_pad = np.zeros_like(pad_u)
    dw = np.zeros_like(w)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = np.einsum("nohw,nihw->oi", dy, pad_u[:, :, ky:ky + h, kx:kx + wd])
            du_pad[:, :, ky:ky + h, kx:kx + wd] += np.einsum("oi,nohw->nihw", w[:, :, ky, kx], dy)
    du = du_pad[:, :, 1:-1, 1:-1]
    dx = du[:, :, 0::2, 0::2] + du[:, :, 0::2, 1::2] + du[:, :, 1::2, 0::2] + du[:, :, 1::2, 1::2]
    return dx, dw
