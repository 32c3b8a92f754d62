"""Drop-in replacements for the loss modules of reference ``losses.py`` used on the training path
(SparseMaskedL1Loss, NormalizedDistanceLoss -- train.py:210-211) plus ScaleInvariantLoss, on HIP
kernels.  ``forward(x)`` takes ONE list argument, as in the reference (losses.py:22-23, 62-63,
122-123).  Per-sample sums are reduced with wave shuffles + one fp64 atomic per block; the batch
mean happens in a one-wave finalize kernel.  AbsRelError and Threshold (losses.py:189-227, the error measures against the sparse
reconstruction that evaluate.validation_outputs reports) are forward only: one launch of endo_depth_metrics, no atomics.
The reference's other six classes (NormalizedWeightedMaskedL2Loss, SparseMaskedL1LossDisplay, MaskedL1Loss, NormalizedL2Loss,
NormalizedL1Loss, MaskedScaleInvariantLoss -- losses.py:35-54, 69-109, 149-186) follow the same pattern, forward and backward.
PhotometricLoss (not a reference class) is the chain _warp_coordinate_generate -> images_warping -> MaskedL1Loss as one forward and one
backward kernel.
"""

import collections

import torch
from torch import nn

from . import _lib


class _SparseL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, flows_hat, masks, eps):
        lib = _lib.load()
        flows = _lib.dev_f32(flows, "flows")
        flows_hat = _lib.dev_f32(flows_hat, "flows from depth")
        masks = _lib.dev_f32(masks, "sparse masks")
        n, c, h, w = flows.shape
        loss = torch.empty((), dtype=torch.float32, device=flows.device)
        stats = torch.empty((n, 2), dtype=torch.float64, device=flows.device)
        _lib.check(lib.endo_sparse_l1_fwd(_lib.ptr(flows), _lib.ptr(flows_hat), _lib.ptr(masks), _lib.ptr(loss), _lib.ptr(stats),
                                          n, c, h * w, eps, _lib.stream()), "endo_sparse_l1_fwd")
        ctx.save_for_backward(flows, flows_hat, masks, stats)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        flows, flows_hat, masks, stats = ctx.saved_tensors
        n, c, h, w = flows.shape
        grad_loss = _lib.dev_f32(grad_loss, "grad")
        g_f = torch.empty_like(flows) if ctx.needs_input_grad[0] else None
        g_h = torch.empty_like(flows_hat) if ctx.needs_input_grad[1] else None
        _lib.check(lib.endo_sparse_l1_bwd(_lib.ptr(grad_loss), _lib.ptr(flows), _lib.ptr(flows_hat), _lib.ptr(masks),
                                          _lib.ptr(stats), _lib.ptr(g_f), _lib.ptr(g_h), n, c, h * w, ctx.eps, _lib.stream()),
                   "endo_sparse_l1_bwd")
        return g_f, g_h, None, None


class SparseMaskedL1Loss(nn.Module):
    """reference losses.py:57-66."""

    def __init__(self, epsilon=1.0):
        super().__init__()
        self.epsilon = float(epsilon)

    def forward(self, x):
        flows, flows_from_depth, sparse_masks = x
        return _SparseL1Fn.apply(flows, flows_from_depth, sparse_masks, self.epsilon)


class _NormDistFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, warped, intersect, intrinsics, eps):
        lib = _lib.load()
        depth = _lib.dev_f32(depth, "depth maps")
        warped = _lib.dev_f32(warped, "warped depth maps")
        intersect = _lib.dev_f32(intersect, "intersect masks")
        n, _, h, w = depth.shape
        k = _lib.dev_f32(intrinsics, "intrinsics").reshape(n, 9)
        loss = torch.empty((), dtype=torch.float32, device=depth.device)
        stats = torch.empty((n, 4), dtype=torch.float64, device=depth.device)
        _lib.check(lib.endo_norm_dist_fwd(_lib.ptr(depth), _lib.ptr(warped), _lib.ptr(intersect), _lib.ptr(k), _lib.ptr(loss),
                                          _lib.ptr(stats), n, h, w, eps, _lib.stream()), "endo_norm_dist_fwd")
        ctx.save_for_backward(depth, warped, intersect, k, stats)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        depth, warped, intersect, k, stats = ctx.saved_tensors
        n, _, h, w = depth.shape
        grad_loss = _lib.dev_f32(grad_loss, "grad")
        g_d = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(warped) if ctx.needs_input_grad[1] else None
        _lib.check(lib.endo_norm_dist_bwd(_lib.ptr(grad_loss), _lib.ptr(depth), _lib.ptr(warped), _lib.ptr(intersect), _lib.ptr(k),
                                          _lib.ptr(stats), _lib.ptr(g_d), _lib.ptr(g_w), n, h, w, ctx.eps, _lib.stream()),
                   "endo_norm_dist_bwd")
        return g_d, g_w, None, None, None


class NormalizedDistanceLoss(nn.Module):
    """reference losses.py:112-146.  ``height`` / ``width`` are accepted for signature parity; the
    pixel grid is generated inside the kernel."""

    def __init__(self, height, width, eps=1.0e-5):
        super().__init__()
        self.height, self.width, self.eps = int(height), int(width), float(eps)

    def forward(self, x):
        depth_maps, warped_depth_maps, intersect_masks, intrinsics = x
        if depth_maps.shape[2] != self.height or depth_maps.shape[3] != self.width:
            raise RuntimeError("NormalizedDistanceLoss was built for %dx%d" % (self.height, self.width))
        return _NormDistFn.apply(depth_maps, warped_depth_maps, intersect_masks, intrinsics, self.eps)


class _ScaleInvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, goal, boundaries, eps):
        lib = _lib.load()
        pred = _lib.dev_f32(pred, "predicted depths")
        goal = _lib.dev_f32(goal, "goal depths")
        boundaries = _lib.dev_f32(boundaries, "boundaries")
        n, hw = pred.shape[0], pred.shape[1] * pred.shape[2] * pred.shape[3]
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        stats = torch.empty((n, 3), dtype=torch.float64, device=pred.device)
        _lib.check(lib.endo_scale_inv_fwd(_lib.ptr(pred), _lib.ptr(goal), _lib.ptr(boundaries), _lib.ptr(loss), _lib.ptr(stats), n,
                                          hw, eps, _lib.stream()), "endo_scale_inv_fwd")
        ctx.save_for_backward(pred, goal, boundaries, stats)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        pred, goal, boundaries, stats = ctx.saved_tensors
        n, hw = pred.shape[0], pred.shape[1] * pred.shape[2] * pred.shape[3]
        grad_loss = _lib.dev_f32(grad_loss, "grad")
        g_p = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        g_g = torch.empty_like(goal) if ctx.needs_input_grad[1] else None
        _lib.check(lib.endo_scale_inv_bwd(_lib.ptr(grad_loss), _lib.ptr(pred), _lib.ptr(goal), _lib.ptr(boundaries), _lib.ptr(stats),
                                          _lib.ptr(g_p), _lib.ptr(g_g), n, hw, ctx.eps, _lib.stream()), "endo_scale_inv_bwd")
        return g_p, g_g, None, None


class ScaleInvariantLoss(nn.Module):
    """reference losses.py:17-32."""

    def __init__(self, epsilon=1.0e-8):
        super().__init__()
        self.epsilon = float(epsilon)

    def forward(self, x):
        predicted_depths, goal_depths, boundaries = x
        return _ScaleInvFn.apply(predicted_depths, goal_depths, boundaries, self.epsilon)


def _no_grad_inputs(owner, **tensors):
    """Masks, sparse depths and translations are never differentiated by the reference; asking for such a gradient is an error here,
    not a silent None."""
    for name, t in tensors.items():
        if t.requires_grad:
            raise RuntimeError("%s: %s get no gradient (the reference does not differentiate them); detach them" % (owner, name))


class _RatioFn(torch.autograd.Function):
    """NormalizedL2Loss / NormalizedL1Loss / NormalizedWeightedMaskedL2Loss: ``name`` picks the endo_<name>_fwd / _bwd pair;
    ``translations`` is None except for the weighted form."""

    @staticmethod
    def forward(ctx, depth, warped, masks, translations, eps, name):
        lib = _lib.load()
        depth = _lib.dev_f32(depth, "depth maps")
        warped = _lib.dev_f32(warped, "warped depth maps")
        masks = _lib.dev_f32(masks, "masks")
        if depth.dim() != 4 or warped.shape != depth.shape or masks.shape != depth.shape:
            raise ValueError("%s needs three (N, C, H, W) tensors of one shape" % name)
        n, hw = depth.shape[0], depth.shape[1] * depth.shape[2] * depth.shape[3]
        loss = torch.empty((), dtype=torch.float32, device=depth.device)
        stats = torch.empty((n, 4), dtype=torch.float64, device=depth.device)
        args = [_lib.ptr(depth), _lib.ptr(warped), _lib.ptr(masks)]
        if translations is not None:
            translations = _lib.dev_f32(translations, "translations").reshape(-1)
            if translations.numel() != 3 * n:
                raise ValueError("%s needs (N, 3) translations" % name)
            args.append(_lib.ptr(translations))
        _lib.check(getattr(lib, "endo_%s_fwd" % name)(*args, _lib.ptr(loss), _lib.ptr(stats), n, hw, eps, _lib.stream()),
                   "endo_%s_fwd" % name)
        ctx.save_for_backward(depth, warped, masks, stats)
        ctx.eps, ctx.name = eps, name
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        depth, warped, masks, stats = ctx.saved_tensors
        n, hw = depth.shape[0], depth.shape[1] * depth.shape[2] * depth.shape[3]
        grad_loss = _lib.dev_f32(grad_loss, "grad")
        g_d = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(warped) if ctx.needs_input_grad[1] else None
        _lib.check(getattr(lib, "endo_%s_bwd" % ctx.name)(_lib.ptr(grad_loss), _lib.ptr(depth), _lib.ptr(warped), _lib.ptr(masks),
                                                          _lib.ptr(stats), _lib.ptr(g_d), _lib.ptr(g_w), n, hw, ctx.eps, _lib.stream()),
                   "endo_%s_bwd" % ctx.name)
        return g_d, g_w, None, None, None, None


class NormalizedWeightedMaskedL2Loss(nn.Module):
    """reference losses.py:35-54.  The per-sample weights 1 / (1e-8 + |translation|) couple the batch; they are formed on the device."""

    def __init__(self, epsilon=1.0):
        super().__init__()
        self.epsilon = float(epsilon)

    def forward(self, x):
        depth_maps, warped_depth_maps, intersect_masks, translations = x
        _no_grad_inputs("NormalizedWeightedMaskedL2Loss", masks=intersect_masks, translations=translations)
        return _RatioFn.apply(depth_maps, warped_depth_maps, intersect_masks, translations, self.epsilon, "weighted_l2")


class NormalizedL2Loss(nn.Module):
    """reference losses.py:94-109.  The mean depth in the denominator is a constant in the backward (the reference's no_grad)."""

    def __init__(self, eps=1.0e-3):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        depth_maps, warped_depth_maps, intersect_masks = x
        _no_grad_inputs("NormalizedL2Loss", masks=intersect_masks)
        return _RatioFn.apply(depth_maps, warped_depth_maps, intersect_masks, None, float(self.eps), "norm_l2")


class NormalizedL1Loss(nn.Module):
    """reference losses.py:149-164.  Here the mean depth is differentiated, as the reference's autograd does."""

    def __init__(self, eps=1.0e-3):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        depth_maps, warped_depth_maps, masks = x
        _no_grad_inputs("NormalizedL1Loss", masks=masks)
        return _RatioFn.apply(depth_maps, warped_depth_maps, masks, None, float(self.eps), "norm_l1")


class _MaskedScaleInvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, sparse, masks, eps):
        lib = _lib.load()
        est = _lib.dev_f32(est, "absolute depth estimations")
        sparse = _lib.dev_f32(sparse, "input sparse depths")
        masks = _lib.dev_f32(masks, "input sparse masks")
        if est.dim() != 4 or sparse.shape != est.shape or masks.shape != est.shape:
            raise ValueError("MaskedScaleInvariantLoss needs three (N, C, H, W) tensors of one shape")
        n, hw = est.shape[0], est.shape[1] * est.shape[2] * est.shape[3]
        loss = torch.empty((), dtype=torch.float32, device=est.device)
        stats = torch.empty((n, 3), dtype=torch.float64, device=est.device)
        _lib.check(lib.endo_masked_scale_inv_fwd(_lib.ptr(est), _lib.ptr(sparse), _lib.ptr(masks), _lib.ptr(loss), _lib.ptr(stats), n,
                                                 hw, eps, _lib.stream()), "endo_masked_scale_inv_fwd")
        ctx.save_for_backward(est, sparse, masks, stats)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        est, sparse, masks, stats = ctx.saved_tensors
        n, hw = est.shape[0], est.shape[1] * est.shape[2] * est.shape[3]
        grad_loss = _lib.dev_f32(grad_loss, "grad")
        g_e = torch.empty_like(est) if ctx.needs_input_grad[0] else None
        _lib.check(lib.endo_masked_scale_inv_bwd(_lib.ptr(grad_loss), _lib.ptr(est), _lib.ptr(sparse), _lib.ptr(masks), _lib.ptr(stats),
                                                 _lib.ptr(g_e), n, hw, ctx.eps, _lib.stream()), "endo_masked_scale_inv_bwd")
        return g_e, None, None, None


class MaskedScaleInvariantLoss(nn.Module):
    """reference losses.py:167-186: ScaleInvariantLoss against sparse depths.  The log ratio is selected where the sparse depth is at
    least 0.5 (0 elsewhere, mask or no mask); an empty mask gives NaN, as the reference's 0 / 0 does."""

    def __init__(self, epsilon=1.0e-8):
        super().__init__()
        self.epsilon = float(epsilon)

    def forward(self, x):
        absolute_depth_estimations, input_sparse_depths, input_sparse_masks = x
        _no_grad_inputs("MaskedScaleInvariantLoss", sparse_depths=input_sparse_depths, masks=input_sparse_masks)
        return _MaskedScaleInvFn.apply(absolute_depth_estimations, input_sparse_depths, input_sparse_masks, self.epsilon)


class MaskedL1Loss(nn.Module):
    """reference losses.py:82-91: the photometric term.  Arithmetically SparseMaskedL1Loss with C image channels under the
    (N, 1, H, W) mask, so it runs on the same kernels (endo_sparse_l1_fwd / _bwd)."""

    def __init__(self, epsilon=1.0):
        super().__init__()
        self.epsilon = float(epsilon)

    def forward(self, x):
        images, twice_warped_images, intersect_masks = x
        _no_grad_inputs("MaskedL1Loss", masks=intersect_masks)
        _one_channel_mask("MaskedL1Loss", images, twice_warped_images, intersect_masks)
        return _SparseL1Fn.apply(images, twice_warped_images, intersect_masks, self.epsilon)


def _one_channel_mask(owner, maps, maps_hat, masks):
    if maps.dim() != 4 or maps_hat.shape != maps.shape or tuple(masks.shape) != (maps.shape[0], 1, maps.shape[2], maps.shape[3]):
        raise ValueError("%s needs two (N, C, H, W) tensors and an (N, 1, H, W) mask" % owner)


class _PhotometricFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, colors_1, colors_2, mask, intersect, t, r, k, eps, mode):
        lib = _lib.load()
        n, c, h, w = colors_1.shape
        loss = torch.empty((), dtype=torch.float32, device=depth.device)
        stats = torch.empty((n, 2), dtype=torch.float64, device=depth.device)
        plane = torch.empty(int(lib.endo_photometric_workspace_floats(n, h, w)), dtype=torch.float32, device=depth.device)
        _lib.check(lib.endo_photometric_fwd(_lib.ptr(colors_1), _lib.ptr(colors_2), _lib.ptr(depth), _lib.ptr(mask), _lib.ptr(intersect),
                                            _lib.ptr(t), _lib.ptr(r), _lib.ptr(k), _lib.ptr(loss), _lib.ptr(stats), _lib.ptr(plane),
                                            n, c, h, w, eps, mode, _lib.stream()), "endo_photometric_fwd")
        ctx.save_for_backward(stats, plane)
        ctx.eps, ctx.shape = eps, (n, 1, h, w)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        stats, plane = ctx.saved_tensors
        n, _, h, w = ctx.shape
        grad_loss = _lib.dev_f32(grad_loss, "grad")
        g_d = torch.empty(ctx.shape, dtype=torch.float32, device=plane.device)
        _lib.check(lib.endo_photometric_bwd(_lib.ptr(grad_loss), _lib.ptr(stats), _lib.ptr(plane), _lib.ptr(g_d), 0, n, h, w, ctx.eps,
                                            _lib.stream()), "endo_photometric_bwd")
        return (g_d,) + (None,) * 9


class PhotometricLoss(nn.Module):
    """The photometric term: frame 2's colours sampled where the frame-1 pixels land under depth and pose, against frame 1's colours,
    under the intersect mask -- the scalar of the chain

        [u, v] = _warp_coordinate_generate(depth.permute(0, 2, 3, 1), mask.permute(0, 2, 3, 1), t, R, K)
        warped = images_warping(colors_2, u, v, padding_mode)
        MaskedL1Loss(epsilon)([colors_1, warped, intersect_masks])

    as one forward and one backward kernel (endo_photometric_fwd / _bwd), without the planes u, v and warped.  ``forward`` takes ONE
    list ``[colors_1, colors_2, depth_maps_1, img_masks, intersect_masks, translation_vectors, rotation_matrices, intrinsic_matrices]``:
    colours (N, C, H, W), depth and both masks (N, 1, H, W), as for ``DepthWarpingLayer``.  The gradient reaches the depth only; colours,
    masks or poses that ask for one raise.  A pixel whose coordinate is not finite samples nothing and gets zero gradient."""

    def __init__(self, epsilon=1.0, padding_mode="zeros"):
        super().__init__()
        from .models import PADDING_MODES
        if padding_mode not in PADDING_MODES:
            raise ValueError("PhotometricLoss: padding_mode is one of %s, not %r" % (sorted(PADDING_MODES), padding_mode))
        self.epsilon = float(epsilon)
        self.padding_mode = padding_mode
        self._mode = PADDING_MODES[padding_mode]

    def forward(self, x):
        colors_1, colors_2, depth_maps_1, img_masks, intersect_masks, translation_vectors, rotation_matrices, intrinsic_matrices = x
        _no_grad_inputs("PhotometricLoss", colors_1=colors_1, colors_2=colors_2, masks=img_masks, intersect_masks=intersect_masks,
                        translations=translation_vectors, rotations=rotation_matrices, intrinsics=intrinsic_matrices)
        if colors_1.dim() != 4 or colors_2.shape != colors_1.shape:
            raise ValueError("PhotometricLoss needs two (N, C, H, W) colour tensors of one shape, not %s and %s" % (
                tuple(colors_1.shape), tuple(colors_2.shape)))
        n, _, h, w = (int(v) for v in colors_1.shape)
        for name, t in (("depth maps", depth_maps_1), ("image masks", img_masks), ("intersect masks", intersect_masks)):
            if tuple(t.shape) != (n, 1, h, w):
                raise ValueError("PhotometricLoss: %s are (N, 1, H, W) = %s, not %s" % (name, (n, 1, h, w), tuple(t.shape)))
        for name, t, count in (("translation vectors", translation_vectors, 3), ("rotation matrices", rotation_matrices, 9),
                               ("intrinsic matrices", intrinsic_matrices, 9)):
            if t.numel() != n * count:
                raise ValueError("PhotometricLoss: %s hold N x %d numbers, not %d" % (name, count, t.numel()))
        pose = lambda t, cols, what: _lib.dev_f32(t, what).reshape(n, cols)
        return _PhotometricFn.apply(_lib.dev_f32(depth_maps_1, "depth maps"), _lib.dev_f32(colors_1, "colors 1"),
                                    _lib.dev_f32(colors_2, "colors 2"), _lib.dev_f32(img_masks, "image masks"),
                                    _lib.dev_f32(intersect_masks, "intersect masks"), pose(translation_vectors, 3, "translation vectors"),
                                    pose(rotation_matrices, 9, "rotation matrices"), pose(intrinsic_matrices, 9, "intrinsic matrices"),
                                    self.epsilon, self._mode)


class _SparseL1DisplayFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, flows_hat, masks, eps):
        lib = _lib.load()
        flows = _lib.dev_f32(flows, "flows")
        flows_hat = _lib.dev_f32(flows_hat, "flows from depth")
        masks = _lib.dev_f32(masks, "sparse masks")
        n, c, h, w = flows.shape
        out = torch.empty((n,), dtype=torch.float32, device=flows.device)
        stats = torch.empty((n, 2), dtype=torch.float64, device=flows.device)
        _lib.check(lib.endo_sparse_l1_display_fwd(_lib.ptr(flows), _lib.ptr(flows_hat), _lib.ptr(masks), _lib.ptr(out), _lib.ptr(stats),
                                                  n, c, h * w, eps, _lib.stream()), "endo_sparse_l1_display_fwd")
        ctx.save_for_backward(flows, flows_hat, masks, stats)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        flows, flows_hat, masks, stats = ctx.saved_tensors
        n, c, h, w = flows.shape
        grad_out = _lib.dev_f32(grad_out, "grad")
        g_f = torch.empty_like(flows) if ctx.needs_input_grad[0] else None
        g_h = torch.empty_like(flows_hat) if ctx.needs_input_grad[1] else None
        _lib.check(lib.endo_sparse_l1_display_bwd(_lib.ptr(grad_out), _lib.ptr(flows), _lib.ptr(flows_hat), _lib.ptr(masks),
                                                  _lib.ptr(stats), _lib.ptr(g_f), _lib.ptr(g_h), n, c, h * w, ctx.eps, _lib.stream()),
                   "endo_sparse_l1_display_bwd")
        return g_f, g_h, None, None


class SparseMaskedL1LossDisplay(nn.Module):
    """reference losses.py:69-79: SparseMaskedL1Loss per sample, the (N,) vector the reference's outlier detection reads."""

    def __init__(self, epsilon=1.0):
        super().__init__()
        self.epsilon = float(epsilon)

    def forward(self, x):
        flows, flows_from_depth, sparse_masks = x
        _no_grad_inputs("SparseMaskedL1LossDisplay", masks=sparse_masks)
        _one_channel_mask("SparseMaskedL1LossDisplay", flows, flows_from_depth, sparse_masks)
        return _SparseL1DisplayFn.apply(flows, flows_from_depth, sparse_masks, self.epsilon)


_consistency_ws = {}
# The depth-consistency losses the fused kernels hold (csrc/geometry.hip ConsistencyForm): name -> (ENDO_CONSISTENCY_* of
# include/endo_hip.h, the class, the name of its eps attribute, the class's default eps).  The one table: warp_consistency's ``form`` and
# TrainingStep's ``consistency_loss`` (train_step.consistency_loss_spec) read it.
CONSISTENCY_FORMS = collections.OrderedDict((
    ("distance", (0, NormalizedDistanceLoss, "eps", 1.0e-5)),
    ("l2", (1, NormalizedL2Loss, "eps", 1.0e-3)),
    ("l1", (2, NormalizedL1Loss, "eps", 1.0e-3)),
    ("weighted_l2", (3, NormalizedWeightedMaskedL2Loss, "epsilon", 1.0)),
))


def depth_metrics(scaled_depth_maps, sparse_depth_maps, sparse_depth_masks, eps=1.0e-8):
    """endo_depth_metrics on (N, 1, H, W) device tensors: the (N, 4) float32 tensor of [abs rel, sigma 1, sigma 2, sigma 3] per sample,
    without a graph.  A sample whose mask is empty gives NaN in all four, as the reference's 0 / 0 does."""
    lib = _lib.load()
    depth = _lib.dev_f32(scaled_depth_maps.detach(), "scaled depth maps")
    sparse = _lib.dev_f32(sparse_depth_maps.detach(), "sparse depth maps")
    masks = _lib.dev_f32(sparse_depth_masks.detach(), "sparse depth masks")
    if depth.dim() != 4 or depth.shape[1] != 1 or sparse.shape != depth.shape or masks.shape != depth.shape:
        raise ValueError("depth metrics need three (N, 1, H, W) tensors")
    n, _, h, w = (int(v) for v in depth.shape)
    with torch.cuda.device(depth.device):
        out = torch.empty((n, 4), dtype=torch.float32, device=depth.device)
        _lib.check(lib.endo_depth_metrics(_lib.ptr(depth), _lib.ptr(sparse), _lib.ptr(masks), n, h, w, float(eps), _lib.ptr(out),
                                          _lib.stream()), "endo_depth_metrics")
    return out


class AbsRelError(nn.Module):
    """reference losses.py:189-199: the per-sample (N,) mean of |d - s| / (eps + s) over the sparse points.  Forward only."""

    def __init__(self, eps=1.0e-8):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        scaled_depth_maps, sparse_depth_maps, sparse_depth_masks = x
        return depth_metrics(scaled_depth_maps, sparse_depth_maps, sparse_depth_masks, self.eps)[:, 0].contiguous()


class Threshold(nn.Module):
    """reference losses.py:202-227: [sigma_1, sigma_2, sigma_3], each the per-sample (N,) share of sparse points whose
    max(d / s, s / d) is below 1.25, 1.25^2, 1.25^3.  Forward only."""

    def __init__(self, eps=1.0e-8):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        scaled_depth_maps, sparse_depth_maps, sparse_depth_masks = x
        out = depth_metrics(scaled_depth_maps, sparse_depth_maps, sparse_depth_masks, self.eps)
        return [out[:, 1].contiguous(), out[:, 2].contiguous(), out[:, 3].contiguous()]


def _consistency_form(form, form_eps):
    """warp_consistency's ``form`` / ``form_eps`` -> (ENDO_CONSISTENCY_* code, eps), or ValueError."""
    if form not in CONSISTENCY_FORMS:
        raise ValueError("form is one of %s, not %r" % (", ".join(repr(k) for k in CONSISTENCY_FORMS), form))
    code, _, _, default_eps = CONSISTENCY_FORMS[form]
    form_eps = default_eps if form_eps is None else float(form_eps)
    if not (0.0 < form_eps < float("inf")):
        raise ValueError("form_eps must be finite and positive (got %r)" % (form_eps,))
    if form == "distance" and form_eps != default_eps:
        raise ValueError("the fused distance form holds NormalizedDistanceLoss's default eps %g" % default_eps)
    return code, form_eps


def warp_consistency(depth_maps_1, depth_maps_2, img_masks, translations_1_wrt_2, rotations_1_wrt_2, translations_2_wrt_1,
                     rotations_2_wrt_1, intrinsic_matrices, dcl_weight=1.0, epsilon=1.0e-8, form="distance", form_eps=None):
    """Depth warping both ways + NormalizedDistanceLoss both ways, forward and backward, as one library call
    (``endo_warp_consistency``; reference models.py:454-554 and losses.py:112-146 twice each, train.py:305-314, and the autograd
    backward of that chain):

        loss = dcl_weight * 0.5 * (NDL([d1, warp(d2 -> 1), ...]) + NDL([d2, warp(d1 -> 2), ...]))

    Returns ``(loss, d loss / d depth_maps_1, d loss / d depth_maps_2)``.  The same kernels and arithmetic as
    ``DepthWarpingLayer`` + ``NormalizedDistanceLoss`` under autograd (tests/test_gpu_parity.py::test_warp_consistency_call),
    without the ~10 autograd nodes around them -- the chain BASELINE.json's second metric times.

    ``form``: the loss in NormalizedDistanceLoss's place -- "distance", "l2" (NormalizedL2Loss), "l1" (NormalizedL1Loss) or "weighted_l2"
    (NormalizedWeightedMaskedL2Loss, each direction's term weighted by that direction's translations); ``form_eps``: its eps, default
    the class's own (``CONSISTENCY_FORMS``).  The default runs ``endo_warp_consistency``, anything else ``endo_warp_consistency_forms``."""
    default = form == "distance" and form_eps is None          # the call as it always was: nothing to look up or check
    if not default:
        code, form_eps = _consistency_form(form, form_eps)
    lib = _lib.load()
    d1 = _lib.dev_f32(depth_maps_1, "depth maps 1")
    d2 = _lib.dev_f32(depth_maps_2, "depth maps 2")
    mask = _lib.dev_f32(img_masks, "image masks")
    n, _, h, w = d1.shape
    pose = lambda t, cols, what: _lib.dev_f32(t, what).reshape(n, cols)
    t12, r12 = pose(translations_1_wrt_2, 3, "translations"), pose(rotations_1_wrt_2, 9, "rotations")
    t21, r21 = pose(translations_2_wrt_1, 3, "translations"), pose(rotations_2_wrt_1, 9, "rotations")
    k = pose(intrinsic_matrices, 9, "intrinsics")
    need = int(lib.endo_warp_consistency_workspace_floats(n, h, w))
    key = (d1.device, n, h, w)
    ws = _consistency_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _consistency_ws[key] = torch.empty(need, dtype=torch.float32, device=d1.device)
    loss = torch.empty((), dtype=torch.float32, device=d1.device)
    g1, g2 = torch.empty_like(d1), torch.empty_like(d2)
    if default or code == 0:
        _lib.check(lib.endo_warp_consistency(_lib.ptr(d1), _lib.ptr(d2), _lib.ptr(mask), _lib.ptr(t12), _lib.ptr(r12), _lib.ptr(t21),
                                             _lib.ptr(r21), _lib.ptr(k), float(dcl_weight), float(epsilon), _lib.ptr(loss), _lib.ptr(g1),
                                             _lib.ptr(g2), _lib.ptr(ws), n, h, w, _lib.stream()), "endo_warp_consistency")
    else:
        _lib.check(lib.endo_warp_consistency_forms(_lib.ptr(d1), _lib.ptr(d2), _lib.ptr(mask), _lib.ptr(t12), _lib.ptr(r12), _lib.ptr(t21),
                                                   _lib.ptr(r21), _lib.ptr(k), float(dcl_weight), float(epsilon), _lib.ptr(loss),
                                                   _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(ws), n, h, w, code, form_eps, _lib.stream()),
                   "endo_warp_consistency_forms")
    return loss, g1, g2
