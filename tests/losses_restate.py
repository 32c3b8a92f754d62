"""Plain-torch restatement of the six loss classes of the reference's losses.py that oracle/losses.py does not carry
(NormalizedWeightedMaskedL2Loss 35-54, SparseMaskedL1LossDisplay 69-79, MaskedL1Loss 82-91, NormalizedL2Loss 94-109, NormalizedL1Loss
149-164, MaskedScaleInvariantLoss 167-186); csrc/losses.hip is checked against it and it is pinned to the reference's own outputs by
tests/golden/losses_extra_4x16x24.npz (tests/test_losses_extra_host.py).  The operations and their order are the reference's, on the
device and in the dtype of the inputs, so the same functions evaluated on .double() inputs give the fp64 value of the same graph."""

import torch

DIMS = (1, 2, 3)


def _like(value, t):
    return torch.tensor(value, dtype=t.dtype, device=t.device)


def _per_sample(t):
    return t.sum(DIMS)


def _squared_ratio(a, b, m):
    """(sum m (a - b)^2, sum m (a^2 + b^2)) per sample: numerator and twice the mass term of both L2 ratio losses."""
    d = a - b
    return _per_sample(m * d * d), _per_sample(m * (a * a + b * b))


def normalized_weighted_masked_l2(a, b, m, t, epsilon=1.0):
    """losses.py:40-54: per sample  sum m (a-b)^2 / (0.5 sum m (a^2+b^2) + epsilon), averaged over the batch with the weights
    1 / (1e-8 + |t_n|) -- the batch is coupled through them; nobody asks for a gradient to the translations."""
    num, mass = _squared_ratio(a, b, m)
    length = torch.sqrt((t.reshape(-1, 3) ** 2).sum(1))
    weight = _like(1.0, a) / (_like(1.0e-8, a) + length)
    return (num / (0.5 * mass + _like(epsilon, a)) * weight).sum() / weight.sum()


def sparse_masked_l1_display(f, f_hat, m, epsilon=1.0):
    """losses.py:74-79: sum m |f - f^| / (epsilon + sum m) as the (N,) vector, no batch mean."""
    return _per_sample(m * (f - f_hat).abs()) / (_like(epsilon, f) + _per_sample(m))


def masked_l1(x, x_hat, m, epsilon=1.0):
    """losses.py:87-91: the (N, 1, H, W) mask broadcasts over the image channels above the line and counts each pixel once below."""
    return torch.mean(_per_sample(m * (x - x_hat).abs()) / (_like(epsilon, x) + _per_sample(m)))


def _masked_mean(a, m, eps):
    return _per_sample(m * a) / (eps + _per_sample(m))


def normalized_l2(a, b, m, eps=1.0e-3):
    """losses.py:99-109: mean_n( sum m (a-b)^2 / (0.5 sum m (a^2+b^2) + 1e-5 mu^2) ), the masked mean mu of a formed without a graph."""
    with torch.no_grad():
        mu = _masked_mean(a, m, eps)
    num, mass = _squared_ratio(a, b, m)
    return torch.mean(num / (0.5 * mass + 1.0e-5 * mu * mu))


def normalized_l1(a, b, m, eps=1.0e-3):
    """losses.py:154-164: mean_n( sum m |a-b| / (0.5 sum m (|a|+|b|) + 1e-5 mu) ); here mu stays in the graph."""
    mu = _masked_mean(a, m, eps)
    return torch.mean(_per_sample(m * (a - b).abs()) / (0.5 * _per_sample(m * (a.abs() + b.abs())) + 1.0e-5 * mu))


def masked_scale_invariant(est, sparse, m, epsilon=1.0e-8):
    """losses.py:173-186: r = 0 where sparse < 0.5, else log(est + epsilon) - log(sparse) -- SELECTED: the branch not taken holds
    log(0) = -inf wherever the sparse depth is 0; then mean_n( sum m r^2 / sum m + (sum m r)^2 / (sum m)^2 )."""
    r = torch.where(sparse < 0.5, _like(0.0, est), torch.log(est + _like(epsilon, est)) - torch.log(sparse))
    count = _per_sample(m)
    first = _per_sample(m * (r * r)) / count
    total = _per_sample(m * r)
    return torch.mean(first + total * total / (count * count))


# name -> (function, names of its inputs in the fixture, how many of the leading inputs are differentiable, constructor keywords)
CASES = {
    "NormalizedWeightedMaskedL2Loss": (normalized_weighted_masked_l2, ("depth", "warped", "mask", "translations"), 2, {"epsilon": 1.0}),
    "SparseMaskedL1LossDisplay": (sparse_masked_l1_display, ("flows", "flows_hat", "sparse_mask"), 2, {"epsilon": 1.0}),
    "MaskedL1Loss": (masked_l1, ("images", "images_hat", "mask"), 2, {"epsilon": 1.0}),
    "NormalizedL2Loss": (normalized_l2, ("depth", "warped", "mask"), 2, {"eps": 1.0e-3}),
    "NormalizedL1Loss": (normalized_l1, ("depth", "warped", "mask"), 2, {"eps": 1.0e-3}),
    "MaskedScaleInvariantLoss": (masked_scale_invariant, ("est", "sparse", "sparse_mask"), 1, {"epsilon": 1.0e-8}),
}


def value_and_grads(name, inputs, upstream=None):
    """The value of CASES[name] on ``inputs`` (a list of tensors in the order of the table) and its gradients with respect to the
    differentiable ones; ``upstream`` weights a non-scalar value (the Display form), default all ones."""
    fn, _, ndiff, _ = CASES[name]
    args = [t.detach().clone().requires_grad_(i < ndiff) for i, t in enumerate(inputs)]
    value = fn(*args)
    scalar = value if value.dim() == 0 else (value * (torch.ones_like(value) if upstream is None else upstream)).sum()
    grads = torch.autograd.grad(scalar, args[:ndiff])
    return value.detach(), [g.detach() for g in grads]
