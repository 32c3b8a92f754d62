"""Writes tests/golden/consistency_forms.npz: inputs and the outputs of the reference's own train.py loss body (train.py:272-315) with
NormalizedL2Loss, NormalizedL1Loss and NormalizedWeightedMaskedL2Loss (losses.py:94-109, 149-164, 35-54) in NormalizedDistanceLoss's
place, evaluated on the CPU by the reference's unmodified classes under autograd, in fp32 and in fp64.

    python tests/golden/make_consistency_forms_golden.py <directory of the reference checkout>

Needs the reference, so it is run where that exists and not by the test suite; only inputs and recorded outputs are written, no
reference source is stored.  ``.cuda()`` and the missing imports are stubbed as make_golden.py does (its import_reference).  For the
fp64 evaluations ``.cuda()`` is ``.double()`` on floating-point tensors instead of the identity: every constant the reference's layers
build in fp32 (pixel grids, eps, eye) passes through it, so the same classes then run the same graph in fp64.  Network weights come
from oracle.network.synthetic_state seeds, batches from synthetic.make_batch seeds (consistency_forms_restate.head_batch /
empty_batch), not from stored tensors.  The weighted form's list argument holds the direction's own translations.

Records, keys ``<record>::...``; <form> is l2, l1 or weighted_l2, <p> is f32 or f64:

  head (N = 4, 24 x 40 -- neither a multiple of the fused kernels' 16 x 32 tile): consistency_forms_restate.head_batch() -- make_batch
      with the translations scaled by 0.5, 1, 2.5 and 6 per sample, so the weighted form's weights spread by a factor of 13 and 40 % of
      sample 3's boundary pixels sample outside the frame (asserted) -- and the stored positive predictions ``head::pred_1`` / ``_2``:
      smooth maps rounded to 2^-12 and moved by a few of those steps until, in both directions, no intersect pixel's source location
      lies within 1e-3 px of a cell boundary, no pixel's sampled mask within 1e-3 of the 0.9 threshold and no intersect pixel has
      |depth - warped depth| < 1e-4 (the derivative of the chain jumps at each).  Weights 20 / 0.1, epsilons 1e-8, the classes' default
      eps.  ``head::<form>::losses_<p>`` = [total, dcl, sfl], ``head::<form>::grad_pred_1_<p>`` / ``_2_<p>`` = d total / d prediction.
  empty: the head record's predictions on consistency_forms_restate.empty_batch() -- sample 1's pose throws it wholly out of frame
      (its intersect masks are empty in both directions, asserted).  ``empty::<form>::losses_f32``: NaN for l2 and l1 (0 / 0), finite
      for weighted_l2 (eps = 1); ``empty::nan`` = [1, 1, 0] in the order l2, l1, weighted_l2.
  step (2 x 64 x 96): the network of STUDENT_SEED (keep_depth_positive(perturb_affine(.)), train mode), two iterations of train.py's
      body with NormalizedWeightedMaskedL2Loss on synthetic.make_batch(seed = BATCH_SEED + i, 500 sparse points) + clip_grad_norm_(10) +
      SGD(1e-3, 0.9).  Per iteration i and precision: ``step::<i>::losses_<p>`` = [total, dcl, sfl], ``step::<i>::grad_norm_<p>`` (before
      clipping), ``step::<i>::pred_1_<p>``."""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (import_reference's stubs, load_reference_net, the deterministic weights)
import make_photometric_golden as mp  # noqa: E402  (q, nudge, boundary_distance)
import consistency_forms_restate as cr  # noqa: E402

STUDENT_SEED, BATCH_SEED = 4, 200
N, H, W = 2, 64, 96
F32 = np.float32
KINK_MARGIN, THRESHOLD_MARGIN, SIGN_MARGIN = 1.0e-3, 1.0e-3, 1.0e-4


def set_precision(dtype):
    """The ``.cuda()`` shim of the evaluation's precision (module docstring)."""
    if dtype == torch.float64:
        torch.Tensor.cuda = lambda self, *a, **k: self.double() if self.is_floating_point() else self
    else:
        torch.Tensor.cuda = lambda self, *a, **k: self


def loss_class(ref, form, h, w):
    cls = getattr(ref["losses"], cr.CLASS_NAMES[form])
    return cls(height=h, width=w) if form == "distance" else cls()


def loss_body(ref, form, batch, p1, p2):
    """train.py:279-315 on the given predictions with the class of ``form``; the layers are built here, under the current shim."""
    b = batch["boundaries"]
    h, w = b.shape[2], b.shape[3]
    scaling = ref["models"].DepthScalingLayer(epsilon=cr.EPSILON)
    flow_layer = ref["models"].FlowfromDepthLayer()
    warp_layer = ref["models"].DepthWarpingLayer(epsilon=cr.EPSILON)
    sfl_fn = ref["losses"].SparseMaskedL1Loss()
    dcl_fn = loss_class(ref, form, h, w)
    p12 = (batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"], batch["intrinsics"])
    p21 = (batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"], batch["intrinsics"])
    s1, _ = scaling([p1, batch["sparse_depths_1"], batch["sparse_depth_masks_1"]])
    s2, _ = scaling([p2, batch["sparse_depths_2"], batch["sparse_depth_masks_2"]])
    f1 = flow_layer([s1, b, *p12]) * b
    f2 = flow_layer([s2, b, *p21]) * b
    sfl = cr.SFL_WEIGHT * 0.5 * (sfl_fn([batch["sparse_flows_1"] * b, f1, batch["sparse_flow_masks_1"] * b]) +
                                 sfl_fn([batch["sparse_flows_2"] * b, f2, batch["sparse_flow_masks_2"] * b]))
    w21, i1 = warp_layer([s1, s2, b, *p12])
    w12, i2 = warp_layer([s2, s1, b, *p21])
    fourth = {"distance": ([batch["intrinsics"]], [batch["intrinsics"]]), "weighted_l2": ([p12[0]], [p21[0]])}.get(form, ([], []))
    dcl = cr.DCL_WEIGHT * 0.5 * (dcl_fn([s1, w21, i1] + fourth[0]) + dcl_fn([s2, w12, i2] + fourth[1]))
    return dcl + sfl, dcl, sfl, (s1, s2, w21, w12, i1, i2)


def cast(batch, dtype):
    return {k: v.to(dtype) for k, v in batch.items()}


def kinks(ref, batch, preds):
    """Per frame the pixels whose prediction has to move (head record's conditions), and the share of boundary pixels of each sample
    that sample outside the frame in direction 1."""
    set_precision(torch.float32)
    b = batch["boundaries"]
    with torch.no_grad():
        _, _, _, (s1, s2, w21, w12, i1, i2) = loss_body(ref, "l1", batch, torch.from_numpy(preds[0]), torch.from_numpy(preds[1]))
    bad, outside = [], None
    for own, other, warped, inter, t, r in ((s1, s2, w21, i1, batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"]),
                                            (s2, s1, w12, i2, batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"])):
        with torch.no_grad():
            u, v = ref["models"]._warp_coordinate_generate(own.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1), t, r, batch["intrinsics"])
            _, overlap = cr.geometry.depth_warping_parts(own, other, b, t, r, batch["intrinsics"], cr.EPSILON)
        u, v = u.numpy()[..., 0], v.numpy()[..., 0]
        on = inter.numpy()[:, 0] > 0.5
        inside = b.numpy()[:, 0] > 0.5
        near_cell = on & (mp.boundary_distance(u, v) <= KINK_MARGIN)
        near_threshold = inside & (np.abs(overlap.numpy()[:, 0] - 0.9) <= THRESHOLD_MARGIN)
        near_sign = on & (np.abs((own - warped).numpy()[:, 0]) < SIGN_MARGIN)
        bad.append(near_cell | near_threshold | near_sign)
        if outside is None:
            h, w = inside.shape[1:]
            gone = inside & ((u - 0.5 < -1) | (u - 0.5 > w) | (v - 0.5 < -1) | (v - 0.5 > h))
            outside = gone.reshape(gone.shape[0], -1).sum(1) / inside.reshape(inside.shape[0], -1).sum(1)
    return bad, outside, (i1.numpy(), i2.numpy())


def head_record(ref, out):
    n, h, w = cr.HEAD_SHAPE
    batch = cr.head_batch()
    norms = batch["translations_1_wrt_2"].reshape(n, 3).norm(dim=1).numpy()
    assert norms.max() / norms.min() > 8.0, norms
    rng = np.random.default_rng(20250301)
    preds = [mp.q(mg.synthetic.smooth_depth(n, h, w, seed=41 + i).numpy(), 12) for i in range(2)]
    for attempt in range(100):
        bad, outside, inters = kinks(ref, batch, preds)
        if not (bad[0].any() or bad[1].any()):
            break
        preds = [mp.nudge(p, b_[:, None], rng, 1 + attempt // 4) for p, b_ in zip(preds, bad)]
    else:
        raise AssertionError("head: pixels near a kink remain")
    assert min(float(p.min()) for p in preds) > 0.05
    assert outside.max() > 0.02, outside          # some boundary pixels sample outside the frame ...
    shares = [float(i.mean()) for i in inters]
    assert min(float(i[s].mean()) for i in inters for s in range(n)) > 0.05, shares          # ... and no sample's intersect is empty
    out["head::pred_1"], out["head::pred_2"] = preds
    out["head::conditions"] = np.array([attempt + 1, float(outside.max()), min(shares), float(norms.max() / norms.min())])
    for form in cr.NEW_FORMS:
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            set_precision(dtype)
            p1 = torch.from_numpy(preds[0]).to(dtype).requires_grad_(True)
            p2 = torch.from_numpy(preds[1]).to(dtype).requires_grad_(True)
            total, dcl, sfl, _ = loss_body(ref, form, cast(batch, dtype), p1, p2)
            assert total.dtype == dtype
            g1, g2 = torch.autograd.grad(total, [p1, p2])
            assert all(bool(torch.isfinite(t).all()) for t in (total, g1, g2)) and float(dcl) > 0 and float(g1.abs().max()) > 0
            np_dtype = F32 if dtype == torch.float32 else np.float64
            out["head::%s::losses_%s" % (form, tag)] = np.array([float(total), float(dcl), float(sfl)], np_dtype)
            out["head::%s::grad_pred_1_%s" % (form, tag)] = g1.numpy().astype(np_dtype)
            out["head::%s::grad_pred_2_%s" % (form, tag)] = g2.numpy().astype(np_dtype)
        e = [float(np.abs(out["head::%s::%s_f32" % (form, k)].astype(np.float64) - out["head::%s::%s_f64" % (form, k)]).max() /
                   np.abs(out["head::%s::%s_f64" % (form, k)]).max()) for k in ("losses", "grad_pred_1", "grad_pred_2")]
        print("  head %-11s [total, dcl, sfl] = %s   fp32 against fp64 (max abs / max |ref|): losses %.2e  gradients %.2e %.2e" % (
            form, out["head::%s::losses_f64" % form], e[0], e[1], e[2]))
    set_precision(torch.float32)


def empty_record(ref, out):
    batch = cr.empty_batch()
    p1, p2 = torch.from_numpy(out["head::pred_1"]), torch.from_numpy(out["head::pred_2"])
    nan = []
    for form in cr.NEW_FORMS:
        with torch.no_grad():
            total, dcl, sfl, (_, _, _, _, i1, i2) = loss_body(ref, form, batch, p1, p2)
        assert float(i1[cr.EMPTY_SAMPLE].sum()) == 0.0 and float(i2[cr.EMPTY_SAMPLE].sum()) == 0.0
        assert float(i1.sum()) > 0 and float(i2.sum()) > 0 and bool(torch.isfinite(sfl))
        out["empty::%s::losses_f32" % form] = np.array([float(total), float(dcl), float(sfl)], F32)
        nan.append(int(bool(torch.isnan(total))))
    assert nan == [1, 1, 0], nan
    out["empty::nan"] = np.array(nan, np.int64)
    print("  empty: NaN %s, weighted_l2 %s" % (nan, out["empty::weighted_l2::losses_f32"]))


def step_record(ref, out):
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        set_precision(dtype)
        torch.manual_seed(0)
        net = mg.load_reference_net(ref, mg.onet.keep_depth_positive(mg.onet.perturb_affine(mg.onet.synthetic_state(STUDENT_SEED),
                                                                                          STUDENT_SEED + 1))).train().to(dtype)
        opt = torch.optim.SGD(net.parameters(), lr=1.0e-3, momentum=0.9)
        np_dtype = F32 if dtype == torch.float32 else np.float64
        for i in range(2):
            batch = cast(mg.synthetic.make_batch(N, H, W, seed=BATCH_SEED + i, sparse_points=500), dtype)
            b = batch["boundaries"]
            p1 = net(b * batch["colors_1"])
            p2 = net(b * batch["colors_2"])
            total, dcl, sfl, _ = loss_body(ref, "weighted_l2", batch, p1, p2)
            opt.zero_grad()
            total.backward()
            gnorm = torch.nn.utils.clip_grad_norm_(net.parameters(), 10.0)
            opt.step()
            assert total.dtype == dtype and bool(torch.isfinite(total)) and float(gnorm) > 0 and float(dcl) > 0
            out["step::%d::losses_%s" % (i, tag)] = np.array([float(total), float(dcl), float(sfl)], np_dtype)
            out["step::%d::grad_norm_%s" % (i, tag)] = np.array(float(gnorm), np_dtype)
            out["step::%d::pred_1_%s" % (i, tag)] = p1.detach().numpy().astype(np_dtype)
    set_precision(torch.float32)
    out["step::shape"] = np.array([N, H, W, STUDENT_SEED, BATCH_SEED])
    for i in range(2):
        l32, l64 = out["step::%d::losses_f32" % i].astype(np.float64), out["step::%d::losses_f64" % i]
        g32, g64 = float(out["step::%d::grad_norm_f32" % i]), float(out["step::%d::grad_norm_f64" % i])
        p32, p64 = out["step::%d::pred_1_f32" % i].astype(np.float64), out["step::%d::pred_1_f64" % i]
        print("  step %d: losses %s grad norm %.6f   fp32 against fp64: losses %.2e  grad norm %.2e  pred_1 %.2e" % (
            i, l64, g64, np.abs(l32 - l64).max() / np.abs(l64).max(), abs(g32 - g64) / g64, np.abs(p32 - p64).max() / np.abs(p64).max()))


def main(reference):
    mg.REF = reference
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = mg.import_reference()
    assert os.path.dirname(os.path.abspath(ref["losses"].__file__)) == os.path.abspath(reference)
    out = {}
    head_record(ref, out)
    empty_record(ref, out)
    step_record(ref, out)
    path = os.path.join(HERE, "consistency_forms.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 900 * 1000, os.path.getsize(path)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "losses.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
