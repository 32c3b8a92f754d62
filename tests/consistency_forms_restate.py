"""Plain-torch restatement of the depth-consistency term with each of the reference's four consistency losses, and of the loss head
around it: depth warping both ways (oracle.geometry: reference models.py:469-554) -> NormalizedDistanceLoss (oracle.losses: losses.py
112-146), NormalizedL2Loss, NormalizedL1Loss or NormalizedWeightedMaskedL2Loss (losses_restate: losses.py:94-109, 149-164, 35-54) per
direction -> dcl_weight * 0.5 * (term_1 + term_2), train.py:305-314 with the class in NormalizedDistanceLoss's place.  The weighted
form takes each direction's own translations.  csrc/geometry.hip's fused kernels are checked against it, and it is pinned to the
reference's own outputs by tests/golden/consistency_forms.npz (tests/test_consistency_forms_host.py).  Everything runs in the dtype of
its inputs, so .double() inputs give the fp64 value of the same graph.

Also the inputs of that fixture's records, regenerated from seeds here and in tests/golden/make_consistency_forms_golden.py instead of
being stored: ``head_batch`` and ``empty_batch``."""

import importlib

import numpy as np
import torch

import losses_restate as lr
from oracle import geometry, losses as olosses

synthetic = importlib.import_module("endoscopydepthestimation-pytorch_amd.synthetic")

FORMS = ("distance", "l2", "l1", "weighted_l2")
NEW_FORMS = FORMS[1:]
DEFAULT_EPS = {"distance": 1.0e-5, "l2": 1.0e-3, "l1": 1.0e-3, "weighted_l2": 1.0}          # the classes' own defaults
CLASS_NAMES = {"distance": "NormalizedDistanceLoss", "l2": "NormalizedL2Loss", "l1": "NormalizedL1Loss",
               "weighted_l2": "NormalizedWeightedMaskedL2Loss"}
SFL_WEIGHT, DCL_WEIGHT, EPSILON = 20.0, 0.1, 1.0e-8          # train.py's weights and the layers' epsilon

# the head record: N = 4 at 24 x 40 -- 1.5 x 1.25 tiles of the fused kernels' 16 x 32 -- with the translations of make_batch scaled per
# sample, so that the weighted form's weights differ by a factor of 13 across the batch and 40 % of sample 3's pixels leave the frame
HEAD_SHAPE, HEAD_SEED, HEAD_POINTS = (4, 24, 40), 31, 100
HEAD_TRANSLATION_SCALES = (0.5, 1.0, 2.5, 6.0)
EMPTY_SAMPLE, EMPTY_TRANSLATION = 1, (40.0, -30.0, 0.25)          # sample 1 moved ~50 scene units sideways: nothing of it lands in frame


def scale_translations(batch, scales):
    """translations_1_wrt_2[i] * scales[i]; the inverse pose's translation -R^T t scales with it."""
    s = torch.tensor(scales, dtype=batch["translations_1_wrt_2"].dtype).reshape(-1, 1, 1)
    out = dict(batch)
    out["translations_1_wrt_2"] = batch["translations_1_wrt_2"] * s
    out["translations_2_wrt_1"] = batch["translations_2_wrt_1"] * s
    return out


def head_batch():
    n, h, w = HEAD_SHAPE
    return scale_translations(synthetic.make_batch(n, h, w, seed=HEAD_SEED, sparse_points=HEAD_POINTS), HEAD_TRANSLATION_SCALES)


def throw_out_of_frame(batch, sample, translation=EMPTY_TRANSLATION):
    """``batch`` with ``sample``'s relative pose replaced by a pure translation that leaves no pixel of it in the other frame."""
    out = {k: v.clone() for k, v in batch.items()}
    t = torch.tensor(translation, dtype=out["translations_1_wrt_2"].dtype).reshape(3, 1)
    out["rotations_1_wrt_2"][sample] = torch.eye(3)
    out["rotations_2_wrt_1"][sample] = torch.eye(3)
    out["translations_1_wrt_2"][sample] = t
    out["translations_2_wrt_1"][sample] = -t
    return out


def empty_batch():
    return throw_out_of_frame(head_batch(), EMPTY_SAMPLE)


def consistency_loss(form, depth, warped, intersect, intrinsics, translations, eps=None):
    """One direction's term: the class of ``form`` on its own list argument."""
    eps = DEFAULT_EPS[form] if eps is None else eps
    if form == "distance":
        return olosses.normalized_distance(depth, warped, intersect, intrinsics, eps)
    if form == "l2":
        return lr.normalized_l2(depth, warped, intersect, eps)
    if form == "l1":
        return lr.normalized_l1(depth, warped, intersect, eps)
    if form == "weighted_l2":
        return lr.normalized_weighted_masked_l2(depth, warped, intersect, translations, eps)
    raise ValueError(form)


def warp_consistency(form, depth_1, depth_2, batch, dcl_weight=1.0, epsilon=EPSILON, eps=None):
    """dcl_weight * 0.5 * (L(d1, warp(d2 -> 1)) + L(d2, warp(d1 -> 2))); also returns the warped maps and intersect masks."""
    b, k = batch["boundaries"], batch["intrinsics"]
    t12, r12 = batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"]
    t21, r21 = batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"]
    warped_21, inter_1 = geometry.depth_warping(depth_1, depth_2, b, t12, r12, k, epsilon)
    warped_12, inter_2 = geometry.depth_warping(depth_2, depth_1, b, t21, r21, k, epsilon)
    dcl = dcl_weight * 0.5 * (consistency_loss(form, depth_1, warped_21, inter_1, k, t12, eps) +
                              consistency_loss(form, depth_2, warped_12, inter_2, k, t21, eps))
    return dcl, {"warped_21": warped_21, "warped_12": warped_12, "inter_1": inter_1, "inter_2": inter_2}


def warp_consistency_value_and_grads(form, depth_1, depth_2, batch, dcl_weight=1.0, epsilon=EPSILON, eps=None):
    d1 = depth_1.detach().clone().requires_grad_(True)
    d2 = depth_2.detach().clone().requires_grad_(True)
    dcl, _ = warp_consistency(form, d1, d2, batch, dcl_weight, epsilon, eps)
    g1, g2 = torch.autograd.grad(dcl, (d1, d2))
    return dcl.detach(), g1, g2


def head(form, pred_1, pred_2, batch, sfl_weight=SFL_WEIGHT, dcl_weight=DCL_WEIGHT, epsilon=EPSILON, eps=None):
    """train.py:279-315 on the given predictions with the class of ``form``: (total, dcl, sfl, extras)."""
    b = batch["boundaries"]
    scaled_1, _ = geometry.depth_scaling(pred_1, batch["sparse_depths_1"], batch["sparse_depth_masks_1"], epsilon)
    scaled_2, _ = geometry.depth_scaling(pred_2, batch["sparse_depths_2"], batch["sparse_depth_masks_2"], epsilon)
    flow_1 = geometry.flow_from_depth(scaled_1, b, batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"], batch["intrinsics"]) * b
    flow_2 = geometry.flow_from_depth(scaled_2, b, batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"], batch["intrinsics"]) * b
    sfl = sfl_weight * 0.5 * (
        olosses.sparse_masked_l1(batch["sparse_flows_1"] * b, flow_1, batch["sparse_flow_masks_1"] * b) +
        olosses.sparse_masked_l1(batch["sparse_flows_2"] * b, flow_2, batch["sparse_flow_masks_2"] * b))
    dcl, extras = warp_consistency(form, scaled_1, scaled_2, batch, dcl_weight, epsilon, eps)
    extras.update(scaled_1=scaled_1, scaled_2=scaled_2)
    return dcl + sfl, dcl, sfl, extras


def head_value_and_grads(form, pred_1, pred_2, batch, dtype=torch.float32, **kw):
    """([total, dcl, sfl] as a tensor of ``dtype``, d total / d pred_1, d total / d pred_2) with everything cast to ``dtype``."""
    x = {k: v.to(dtype) for k, v in batch.items()}
    p1 = pred_1.detach().to(dtype).clone().requires_grad_(True)
    p2 = pred_2.detach().to(dtype).clone().requires_grad_(True)
    total, dcl, sfl, _ = head(form, p1, p2, x, **kw)
    g1, g2 = torch.autograd.grad(total, (p1, p2), allow_unused=True)
    return torch.stack([total.detach(), dcl.detach(), sfl.detach()]), g1, g2


def record_bound(ref64, ref32, factor=4.0, floor=1.0e-6):
    """The bound a device result is held to against a record's fp64 values: ``factor`` x the reference's own fp32-versus-fp64 error
    (max abs), never tighter than ``floor`` of max |ref| -- what csrc/geometry.hip grants the order of its atomic sums."""
    ref64 = np.asarray(ref64, np.float64)
    err32 = float(np.max(np.abs(np.asarray(ref32, np.float64) - ref64)))
    return max(factor * err32, floor * float(np.max(np.abs(ref64))))
