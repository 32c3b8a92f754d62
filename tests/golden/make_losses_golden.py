"""Writes tests/golden/losses_extra_4x16x24.npz: inputs and the outputs of the reference's own NormalizedWeightedMaskedL2Loss,
SparseMaskedL1LossDisplay, MaskedL1Loss, NormalizedL2Loss, NormalizedL1Loss and MaskedScaleInvariantLoss (losses.py:35-54, 69-109,
149-186), evaluated on the CPU by the reference's unmodified modules under autograd.

    python tests/golden/make_losses_golden.py <directory of the reference checkout>

Needs the reference, so it is run where that exists and not by the test suite; only the inputs and the recorded outputs are written,
no reference source is stored.  ``.cuda()`` is made the identity for the process, as make_golden.py does (the constructors call it).

Two records, keys ``<record>::<input>`` and ``<record>::<class>::loss`` / ``::grad<i>``:

  main (N = 4, 16 x 24): every class's value and its gradients with respect to its differentiable inputs, all finite.  {0, 1} masks at
      about 60 %, no sample empty; depths in 0.3 - 0.9, warped = depth x U(0.8, 1.25), and six masked pixels with warped == depth
      exactly (|.|'s gradient at a tie); 3-channel images; translations ~ N(0, 1); a 5 % sparse mask, sparse depths in 0.6 - 8 and 0
      off the mask (log(0) in the unselected branch), estimations in 0.5 - 8, one masked pixel with sparse depth 0.3 (r = 0, still
      counted); SparseMaskedL1LossDisplay's gradients are taken under the non-uniform (N,) upstream gradient ``main::display_upstream``.
  edge (N = 2), values only: sample 1's masks are empty (NormalizedL1Loss, NormalizedL2Loss, MaskedScaleInvariantLoss: NaN; the
      others: that sample contributes 0); sample 0's translation is zero, so its weight is 1e8 and the weighted loss is sample 0's."""

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32

# class -> (its inputs in forward's order, how many of the leading ones are differentiable, constructor keywords = the defaults)
CLASSES = {
    "NormalizedWeightedMaskedL2Loss": (("depth", "warped", "mask", "translations"), 2, {"epsilon": 1.0}),
    "SparseMaskedL1LossDisplay": (("flows", "flows_hat", "sparse_mask"), 2, {"epsilon": 1.0}),
    "MaskedL1Loss": (("images", "images_hat", "mask"), 2, {"epsilon": 1.0}),
    "NormalizedL2Loss": (("depth", "warped", "mask"), 2, {"eps": 1.0e-3}),
    "NormalizedL1Loss": (("depth", "warped", "mask"), 2, {"eps": 1.0e-3}),
    "MaskedScaleInvariantLoss": (("est", "sparse", "sparse_mask"), 1, {"epsilon": 1.0e-8}),
}
NAN_ON_EMPTY = ("NormalizedL2Loss", "NormalizedL1Loss", "MaskedScaleInvariantLoss")


def q(a, bits=10):
    """Rounded to multiples of 2^-bits: float32 numbers with short mantissas, which keeps the compressed file small."""
    return (np.round(np.asarray(a, np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(F32)


def inputs(n, h, w, seed):
    rng = np.random.default_rng(seed)
    x = {}
    x["mask"] = (rng.random((n, 1, h, w)) < 0.6).astype(F32)
    x["depth"] = q(rng.uniform(0.3, 0.9, (n, 1, h, w)))
    x["warped"] = (x["depth"] * rng.uniform(0.8, 1.25, (n, 1, h, w)).astype(F32)).astype(F32)
    x["images"] = q(rng.uniform(-1.0, 1.0, (n, 3, h, w)), 7)
    x["images_hat"] = q(x["images"] + rng.normal(0.0, 0.2, (n, 3, h, w)), 7)
    x["flows"] = q(rng.normal(0.0, 5.0, (n, 2, h, w)), 5)
    x["flows_hat"] = q(x["flows"] + rng.normal(0.0, 1.0, (n, 2, h, w)), 5)
    x["translations"] = rng.standard_normal((n, 3, 1)).astype(F32)
    x["sparse_mask"] = (rng.random((n, 1, h, w)) < 0.05).astype(F32)
    x["sparse"] = (q(rng.uniform(0.6, 8.0, (n, 1, h, w))) * x["sparse_mask"]).astype(F32)
    x["est"] = q(rng.uniform(0.5, 8.0, (n, 1, h, w)))
    return x


def main_inputs():
    x = inputs(4, 16, 24, 20240611)
    ys, xs = np.nonzero(x["mask"][0, 0])
    for k in range(6):          # exact ties on masked pixels, first sample
        x["warped"][0, 0, ys[3 * k], xs[3 * k]] = x["depth"][0, 0, ys[3 * k], xs[3 * k]]
    ys, xs = np.nonzero(x["sparse_mask"][1, 0])
    x["sparse"][1, 0, ys[0], xs[0]] = F32(0.3)          # masked, below 0.5: r = 0 and still counted in sum m
    x["display_upstream"] = np.array([0.5, -1.25, 2.0, 0.75], dtype=F32)
    assert all(x["mask"][i].sum() > 0 and x["sparse_mask"][i].sum() > 1 for i in range(4))
    assert 0.5 < x["mask"].mean() < 0.7 and set(np.unique(x["mask"])) == {0.0, 1.0}
    assert int(((x["warped"] == x["depth"]) & (x["mask"] > 0)).sum()) >= 5
    assert np.all(x["sparse"][x["sparse_mask"] == 0] == 0)
    low = (x["sparse_mask"] > 0) & (x["sparse"] < 0.5)
    assert int(low.sum()) == 1 and float(x["sparse"][low][0]) == float(F32(0.3))
    assert x["sparse"][(x["sparse_mask"] > 0) & ~low].min() >= 0.6 and x["est"].min() >= 0.5
    return x


def edge_inputs():
    x = inputs(2, 16, 24, 20240612)
    x["mask"][1] = 0.0
    x["sparse_mask"][1] = 0.0
    x["sparse"][1] = 0.0
    x["translations"][0] = 0.0
    assert x["mask"][1].sum() == 0 and x["sparse_mask"][1].sum() == 0 and x["mask"][0].sum() > 0 and x["sparse_mask"][0].sum() > 0
    assert not x["translations"][0].any() and x["translations"][1].any()
    return x


def main(reference):
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, reference)
    ref = importlib.import_module("losses")
    sys.path.remove(reference)
    assert os.path.dirname(os.path.abspath(ref.__file__)) == os.path.abspath(reference)
    out = {}
    x = main_inputs()
    for key, value in x.items():
        out["main::" + key] = value
    for name, (names, ndiff, kw) in CLASSES.items():
        args = [torch.from_numpy(x[k]).clone().requires_grad_(i < ndiff) for i, k in enumerate(names)]
        value = getattr(ref, name)(**kw)(args)
        if name == "SparseMaskedL1LossDisplay":
            assert value.shape == (4,)
            scalar = (value * torch.from_numpy(x["display_upstream"])).sum()
        else:
            assert value.dim() == 0
            scalar = value
        grads = torch.autograd.grad(scalar, args[:ndiff])
        assert bool(torch.isfinite(value).all()) and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads), name
        out["main::%s::loss" % name] = value.detach().numpy().astype(F32)
        for i, g in enumerate(grads):
            out["main::%s::grad%d" % (name, i)] = g.numpy().astype(F32)
    e = edge_inputs()
    for key, value in e.items():
        out["edge::" + key] = value
    with torch.no_grad():
        for name, (names, _, kw) in CLASSES.items():
            value = getattr(ref, name)(**kw)([torch.from_numpy(e[k]) for k in names]).numpy().astype(F32)
            out["edge::%s::loss" % name] = value
            if name in NAN_ON_EMPTY:
                assert np.isnan(value), name          # 0 / 0 for the empty sample, so the batch mean
            elif name == "SparseMaskedL1LossDisplay":
                assert value.shape == (2,) and value[0] > 0 and value[1] == 0
            else:
                assert np.isfinite(value) and value > 0, name
        one = [torch.from_numpy(e[k][:1]) for k in CLASSES["NormalizedWeightedMaskedL2Loss"][0]]
        alone = float(ref.NormalizedWeightedMaskedL2Loss()(one))          # the 1e8 weight: the batch value is sample 0's
        assert abs(float(out["edge::NormalizedWeightedMaskedL2Loss::loss"]) - alone) <= 1e-6 * alone
    path = os.path.join(HERE, "losses_extra_4x16x24.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))
    for name in CLASSES:
        print("  %-32s main %s  edge %s" % (name, out["main::%s::loss" % name], out["edge::%s::loss" % name]))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "losses.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
