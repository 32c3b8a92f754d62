"""Writes tests/golden/depth_metrics_4x16x24.npz: inputs and the outputs of the reference's own AbsRelError and Threshold
(losses.py:189-227), evaluated on the CPU by the reference's unmodified module.

    python tests/golden/make_metrics_golden.py <directory of the reference checkout>

Needs the reference, so it is run where that exists and not by the test suite; only the inputs and the recorded outputs are written,
no reference source is stored.  The inputs: 4 samples of 16 x 24; sparse masks at about 5 %, sparse depth 0 outside the mask; sample 2's
mask is empty (the reference returns NaN for it, asserted below); in sample 0 one masked point has predicted depth 0; in sample 1 three
masked points have d = 1.25 s, 1.25^2 s and 1.25^3 s exactly (powers of two times 1.25^k are float32 numbers), which sit ON the strict
`<` of sigma 1, 2, 3 and so count for the next threshold only."""

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1.0e-8


def inputs():
    rng = np.random.default_rng(20240607)
    n, h, w = 4, 16, 24
    masks = (rng.random((n, 1, h, w)) < 0.05).astype(np.float32)
    masks[2] = 0.0
    sparse = (rng.uniform(0.5, 8.0, (n, 1, h, w)).astype(np.float32) * masks).astype(np.float32)
    depths = (rng.uniform(0.5, 8.0, (n, 1, h, w))).astype(np.float32)
    close = rng.random((n, 1, h, w)) < 0.7          # most predictions near the sparse depth, so every sigma is away from 0 and 1
    near = (sparse * rng.uniform(0.7, 1.6, (n, 1, h, w)).astype(np.float32)).astype(np.float32)
    depths = np.where((masks > 0) & close, near, depths).astype(np.float32)
    ys, xs = np.nonzero(masks[0, 0])
    depths[0, 0, ys[0], xs[0]] = 0.0          # a masked point whose predicted depth is 0: s / (eps + 0) is huge, counts nowhere
    for k, (y, x) in enumerate(((1, 1), (5, 7), (9, 20))):          # exactly on the three thresholds
        masks[1, 0, y, x] = 1.0
        sparse[1, 0, y, x] = np.float32(2.0 ** k)
        depths[1, 0, y, x] = np.float32(2.0 ** k * 1.25 ** (k + 1))
        assert float(depths[1, 0, y, x]) == 2.0 ** k * 1.25 ** (k + 1)
    assert np.all(sparse[masks == 0] == 0) and masks[2].sum() == 0 and all(masks[i].sum() > 0 for i in (0, 1, 3))
    return depths, sparse, masks


def main(reference):
    sys.path.insert(0, reference)
    ref = importlib.import_module("losses")
    sys.path.remove(reference)
    assert os.path.dirname(os.path.abspath(ref.__file__)) == os.path.abspath(reference)
    depths, sparse, masks = inputs()
    x = [torch.from_numpy(a) for a in (depths, sparse, masks)]
    with torch.no_grad():
        abs_rel = ref.AbsRelError(eps=EPS)(x).numpy()
        sigmas = [s.numpy() for s in ref.Threshold(eps=EPS)(x)]
    assert abs_rel.shape == (4,) and all(s.shape == (4,) for s in sigmas)
    assert np.isnan(abs_rel[2]) and all(np.isnan(s[2]) for s in sigmas)          # the empty mask: 0 / 0
    assert np.all(np.isfinite(np.delete(abs_rel, 2))) and all(np.all(np.isfinite(np.delete(s, 2))) for s in sigmas)
    count = masks[1].sum()
    assert sigmas[0][1] * count + 3 <= count          # the three points on the thresholds are not below 1.25
    path = os.path.join(HERE, "depth_metrics_4x16x24.npz")
    np.savez_compressed(path, depths=depths, sparse=sparse, masks=masks, eps=np.float64(EPS), abs_rel=abs_rel.astype(np.float32),
                        sigma_1=sigmas[0].astype(np.float32), sigma_2=sigmas[1].astype(np.float32), sigma_3=sigmas[2].astype(np.float32))
    print("wrote %s: abs rel %s, sigma %s" % (path, abs_rel, [s.tolist() for s in sigmas]))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "losses.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
