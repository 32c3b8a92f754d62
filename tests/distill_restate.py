"""Plain-torch restatement of the distillation head (csrc/distill.hip, endo_distill_head): the teacher-student term of the reference's
utils.learn_from_teacher (utils.py:1471-1480) over ScaleInvariantLoss (losses.py:22-32), its gradient under autograd, ``accumulate``
and the guard flag.  The operations and their order are the reference's, in the dtype of the inputs: on .double() inputs the same
functions give the fp64 value of the same graph.  Pinned to the reference's own outputs by tests/golden/distill.npz
(tests/test_distill_host.py); the kernels are checked against it at the shapes the fixture does not hold (tests/test_gpu_distill.py).
Also the input builder the fixture's generator and the tests share."""

import numpy as np
import torch

DIMS = (1, 2, 3)
F32 = np.float32


def scale_invariant(pred, goal, b, eps):
    """losses.py:22-32: mean over the samples of  sum r^2 / sum b + (sum r)^2 / (sum b)^2,  r = log(b p + eps) - log(b g + eps)."""
    eps = torch.tensor(eps, dtype=pred.dtype, device=pred.device)
    r = torch.log(b * pred + eps) - torch.log(b * goal + eps)
    s = b.sum(DIMS)
    r1 = r.sum(DIMS)
    return ((r * r).sum(DIMS) / s + (r1 * r1) / (s * s)).mean()


def term(p1, p2, g1, g2, b, weight=1.0, eps=1.0e-8):
    """utils.py:1471-1480 times ``weight``."""
    return weight * (0.5 * scale_invariant(p1.abs(), g1.abs(), b, eps) + 0.5 * scale_invariant(p2.abs(), g2.abs(), b, eps))


def head(p1, p2, g1, g2, b, weight=1.0, eps=1.0e-8, accumulate=False, losses=None, grads=None):
    """What endo_distill_head leaves: (losses [total, dcl, sfl, flag, distill], grad_pred_1, grad_pred_2).  accumulate: ``losses`` (its
    first four values) and ``grads`` (a pair) are what a loss head left; the term is added to them."""
    p1 = p1.detach().clone().requires_grad_(True)
    p2 = p2.detach().clone().requires_grad_(True)
    distill = term(p1, p2, g1, g2, b, weight, eps)
    d1, d2 = torch.autograd.grad(distill, (p1, p2))
    distill = distill.detach()
    zero = torch.zeros_like(distill)
    if accumulate:
        total = losses[0] + distill
        flag = ((losses[3] != 0) | ~torch.isfinite(total)).to(distill.dtype)
        return torch.stack([total, losses[1], losses[2], flag, distill]), grads[0] + d1, grads[1] + d2
    flag = (~torch.isfinite(distill)).to(distill.dtype)
    return torch.stack([distill, zero, zero, flag, distill]), d1, d2


def head_inputs(n, h, w, seed, zeros=6, empty_sample=None, non_negative=False):
    """Predictions and goals of both signs with magnitudes in 0.05 - 4 (multiples of 2^-10), a {0, 1} boundary at about 60 %, and
    ``zeros`` exact zeros in each prediction map on boundary pixels of sample 0.  numpy float32, keys pred_1, pred_2, goal_1, goal_2,
    boundaries."""
    rng = np.random.default_rng(seed)
    x = {"boundaries": (rng.random((n, 1, h, w)) < 0.6).astype(F32)}
    for key in ("pred_1", "pred_2", "goal_1", "goal_2"):
        mag = np.round(rng.uniform(0.05, 4.0, (n, 1, h, w)) * 1024.0) / 1024.0
        sign = 1.0 if non_negative else np.where(rng.random((n, 1, h, w)) < 0.5, -1.0, 1.0)
        x[key] = (mag * sign).astype(F32)
    if empty_sample is not None:
        x["boundaries"][empty_sample] = 0.0
    ys, xs = np.nonzero(x["boundaries"][0, 0])
    zeros = min(zeros, len(ys) // 3)
    for k in range(zeros):
        x["pred_1"][0, 0, ys[3 * k], xs[3 * k]] = 0.0
        x["pred_2"][0, 0, ys[3 * k + 1], xs[3 * k + 1]] = 0.0
    return x


def robust_inputs():
    """The three argument pairs of the fixture's ``robust`` record: equal lengths with differences of both signs and a tie, a longer
    first argument, a shorter first argument."""
    a = np.array([0.5, 0.25, 1.0, 0.75, 0.125, 2.0, 0.375], dtype=np.float64)
    b = np.array([0.375, 0.5, 1.0, 0.25, 0.25, 1.5, 0.75], dtype=np.float64)
    return (a, b), (a, b[:5]), (a[:4], b)
