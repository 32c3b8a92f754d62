"""One training iteration on the MI355X path -- the counterpart of the batch-loop body of reference
train.py:272-328, built from the drop-in modules of ``models`` / ``losses`` and the fused optimizer.

  colours * boundary -> two network forwards (BN statistics per call, train.py:276-277) -> depth
  scaling -> flow-from-depth both ways -> boundary masking -> sparse-flow loss -> depth warping
  both ways -> depth-consistency loss (-> with photometric_weight > 0 the photometric term both ways) -> weighted sum (+ the
  non-finite flag, on the device) -> backward
  -> ONE all-reduce of gradients + flag -> fused clip_grad_norm_(10) + SGD(0.9), skipped by the kernel when
  any rank's loss was NaN / Inf.

``DistillationStep`` is the same iteration for teacher-student training (reference utils.py:1462-1482): a teacher forward in front, and
``endo_distill_head`` in place of, or after, the loss head.
"""

import collections
import ctypes

import torch

from . import _lib, display, distributed, losses, models


class _MaskMulFn(torch.autograd.Function):
    """a[n,c,h,w] * mask[n,1,h,w] (train.py:272-273, 293-298); the mask carries no gradient."""

    @staticmethod
    def forward(ctx, a, mask):
        lib = _lib.load()
        a = _lib.dev_f32(a, "tensor")
        mask = _lib.dev_f32(mask, "mask")
        n, c, h, w = a.shape
        out = torch.empty_like(a)
        _lib.check(lib.endo_mask_mul(_lib.ptr(a), _lib.ptr(mask), _lib.ptr(out), n, c, h * w, _lib.stream()), "endo_mask_mul")
        ctx.save_for_backward(mask)
        return out

    @staticmethod
    def backward(ctx, grad):
        lib = _lib.load()
        (mask,) = ctx.saved_tensors
        grad = _lib.dev_f32(grad, "grad")
        n, c, h, w = grad.shape
        out = torch.empty_like(grad)
        _lib.check(lib.endo_mask_mul(_lib.ptr(grad), _lib.ptr(mask), _lib.ptr(out), n, c, h * w, _lib.stream()), "endo_mask_mul")
        return out, None


def mask_mul(a, mask):
    return _MaskMulFn.apply(a, mask)


def consistency_loss_spec(consistency_loss, height, width):
    """``TrainingStep``'s ``consistency_loss`` argument -> (name, module, eps): a name of ``losses.CONSISTENCY_FORMS`` stands for that class
    with its default eps; an instance of one of the four classes is used as it is and supplies its own eps.  Anything else, an eps that
    is not finite and positive, or a NormalizedDistanceLoss built for another size is a ValueError."""
    forms = losses.CONSISTENCY_FORMS
    module = None
    if isinstance(consistency_loss, str):
        if consistency_loss in forms:
            name, cls = consistency_loss, forms[consistency_loss][1]
            module = cls(height=height, width=width) if name == "distance" else cls()
    else:
        for name, (_, cls, _, _) in forms.items():
            if isinstance(consistency_loss, cls):
                module = consistency_loss
                break
    if module is None:
        raise ValueError("consistency_loss is one of %s or an instance of losses.%s, not %r" % (
            ", ".join(repr(k) for k in forms), " / ".join(v[1].__name__ for v in forms.values()), consistency_loss))
    eps = float(getattr(module, forms[name][2]))
    if not (0.0 < eps < float("inf")):
        raise ValueError("consistency_loss: the eps of %s must be finite and positive (got %r)" % (type(module).__name__, eps))
    if name == "distance" and (module.height, module.width) != (int(height), int(width)):
        raise ValueError("consistency_loss: this NormalizedDistanceLoss was built for %dx%d, the step for %dx%d" % (
            module.height, module.width, height, width))
    return name, module, eps


class TrainingStep(object):
    def __init__(self, model, optimizer, height, width, sfl_weight=20.0, dcl_weight=0.1, epsilon=1.0e-8, pair_forward=True,
                 fused_head=True, bf16_storage=False, fp16_storage=False, photometric_weight=0.0, photometric_padding="zeros",
                 consistency_loss="distance"):
        self.model = model
        # the depth-consistency term's loss: "distance" (NormalizedDistanceLoss, the reference's train.py:211), "l2", "l1" or
        # "weighted_l2" (the reference's other three, losses.py:94-109, 149-164, 35-54; the weighted form takes each direction's
        # translations, as utils.py:1700-1703 hands them over), or an instance of one of the four, which supplies its own eps.  The
        # default issues the calls the step always has; another one goes through endo_loss_head_forms, under every storage mode
        self.consistency_loss, self.depth_consistency_loss_function, self.consistency_eps = consistency_loss_spec(
            consistency_loss, height, width)
        # photometric_weight > 0 adds  w * 0.5 * (P(frame 1 against frame 2) + P(frame 2 against frame 1))  of losses.PhotometricLoss on
        # the masked colours, each frame's scaled depth and the depth warp's intersect masks to the total (not in the reference's train.py);
        # 0 is the step without it: the same calls as before the term existed
        self.photometric_weight = float(photometric_weight)
        if not self.photometric_weight >= 0.0:
            raise ValueError("photometric_weight must be >= 0 (got %r)" % (photometric_weight,))
        if photometric_padding not in models.PADDING_MODES:
            raise ValueError("photometric_padding is one of %s, not %r" % (sorted(models.PADDING_MODES), photometric_padding))
        self.photometric_padding = photometric_padding
        self.photometric_loss_function = losses.PhotometricLoss(padding_mode=photometric_padding)
        # the network over bf16 level buffers (FCDenseNet.forward_bf16_storage: activations and inter-layer gradients stored as
        # bf16, bf16 matrix cores, fp32 accumulation / statistics / parameter gradients; BASELINE configs[2]); the two frames are two
        # sample groups of one call (each with its own BatchNorm statistics, as the reference's two calls, train.py:276-277); losses,
        # clipping and SGD stay fp32
        # fp16_storage: the same family over IEEE half (FCDenseNet.forward_fp16_storage; BASELINE configs[4]'s storage half)
        self.half_storage = bool(fp16_storage)
        self.bf16_storage = bool(bf16_storage) or self.half_storage
        if self.bf16_storage and not (fused_head and pair_forward):
            raise ValueError("bf16_storage runs through the fused loss head")
        self.epsilon = float(epsilon)
        # everything between the network outputs and d loss / d prediction as one library call (endo_loss_head: the modules'
        # kernels, composed in C) instead of ~60 autograd nodes; needs the grouped pair forward
        self.fused_head = bool(fused_head) and bool(pair_forward) and hasattr(model, "forward_pair_packed")
        if self.fused_head and self.consistency_loss == "distance" and self.consistency_eps != losses.CONSISTENCY_FORMS["distance"][3]:
            raise ValueError("consistency_loss: the fused loss head's distance form holds NormalizedDistanceLoss's default eps %g; "
                             "eps = %g needs fused_head=False" % (losses.CONSISTENCY_FORMS["distance"][3], self.consistency_eps))
        self._head_ws = None
        # both frames of the pair through the network as one grouped batch (FCDenseNet.forward_pair): same values as the
        # reference's two calls (train.py:276-277), half the kernel launches
        self.pair_forward = bool(pair_forward) and hasattr(model, "forward_pair")
        self.optimizer = optimizer
        self.sfl_weight = float(sfl_weight)
        self.dcl_weight = float(dcl_weight)
        self.depth_scaling_layer = models.DepthScalingLayer(epsilon=epsilon)
        self.depth_warping_layer = models.DepthWarpingLayer(epsilon=epsilon)
        self.flow_from_depth_layer = models.FlowfromDepthLayer()
        self.sparse_flow_loss_function = losses.SparseMaskedL1Loss()
        self.bucket = distributed.GradientBucket(model.flat_gradients, getattr(model, "flat_gradient_bucket", None))
        # persistent replicas must start from the same state (nn.DataParallel re-broadcasts on every forward, train.py:197)
        distributed.sync_parameters(model, optimizer)

    def losses(self, batch):
        """Forward part: returns (loss, depth_consistency_loss, sparse_flow_loss, extras)."""
        b = batch["boundaries"]
        colors_1 = mask_mul(batch["colors_1"], b)
        colors_2 = mask_mul(batch["colors_2"], b)
        if self.pair_forward:
            pred_1, pred_2 = self.model.forward_pair(colors_1, colors_2)
        else:
            pred_1 = self.model(colors_1)
            pred_2 = self.model(colors_2)
        scaled_1, std_1 = self.depth_scaling_layer([pred_1, batch["sparse_depths_1"], batch["sparse_depth_masks_1"]])
        scaled_2, std_2 = self.depth_scaling_layer([pred_2, batch["sparse_depths_2"], batch["sparse_depth_masks_2"]])
        flows_1 = self.flow_from_depth_layer([scaled_1, b, batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"],
                                              batch["intrinsics"]])
        flows_2 = self.flow_from_depth_layer([scaled_2, b, batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"],
                                              batch["intrinsics"]])
        with torch.no_grad():
            sparse_flow_masks_1 = mask_mul(batch["sparse_flow_masks_1"], b)
            sparse_flow_masks_2 = mask_mul(batch["sparse_flow_masks_2"], b)
            sparse_flows_1 = mask_mul(batch["sparse_flows_1"], b)
            sparse_flows_2 = mask_mul(batch["sparse_flows_2"], b)
        flows_1 = mask_mul(flows_1, b)
        flows_2 = mask_mul(flows_2, b)
        sfl = self.sfl_weight * 0.5 * (
            self.sparse_flow_loss_function([sparse_flows_1, flows_1, sparse_flow_masks_1]) +
            self.sparse_flow_loss_function([sparse_flows_2, flows_2, sparse_flow_masks_2]))
        warped_21, inter_1 = self.depth_warping_layer([scaled_1, scaled_2, b, batch["translations_1_wrt_2"],
                                                       batch["rotations_1_wrt_2"], batch["intrinsics"]])
        warped_12, inter_2 = self.depth_warping_layer([scaled_2, scaled_1, b, batch["translations_2_wrt_1"],
                                                       batch["rotations_2_wrt_1"], batch["intrinsics"]])
        dcl = self.dcl_weight * 0.5 * (
            self.depth_consistency_loss_function(self._consistency_inputs(scaled_1, warped_21, inter_1, batch, "translations_1_wrt_2")) +
            self.depth_consistency_loss_function(self._consistency_inputs(scaled_2, warped_12, inter_2, batch, "translations_2_wrt_1")))
        extras = {"pred_1": pred_1, "pred_2": pred_2, "scaled_1": scaled_1, "scaled_2": scaled_2,
                  "warped_21": warped_21, "warped_12": warped_12, "inter_1": inter_1, "inter_2": inter_2,
                  "std_1": std_1, "std_2": std_2}
        if self.photometric_weight > 0.0:
            photo = self.photometric_weight * 0.5 * (
                self.photometric_loss_function([colors_1, colors_2, scaled_1, b, inter_1, batch["translations_1_wrt_2"],
                                                batch["rotations_1_wrt_2"], batch["intrinsics"]]) +
                self.photometric_loss_function([colors_2, colors_1, scaled_2, b, inter_2, batch["translations_2_wrt_1"],
                                                batch["rotations_2_wrt_1"], batch["intrinsics"]]))
            extras["photo"] = photo
            return dcl + sfl + photo, dcl, sfl, extras
        return dcl + sfl, dcl, sfl, extras

    def _consistency_inputs(self, scaled, warped, inter, batch, translations):
        """The list argument of the chosen consistency class: the intrinsics fourth for the distance loss, the direction's translations
        fourth for the weighted one, three entries for the other two."""
        if self.consistency_loss == "distance":
            return [scaled, warped, inter, batch["intrinsics"]]
        if self.consistency_loss == "weighted_l2":
            return [scaled, warped, inter, batch[translations]]
        return [scaled, warped, inter]

    def _loss_head(self, lib, tensors, colors, outputs):
        """The loss head call of this step's settings: endo_loss_head / endo_loss_head_photo with the default consistency loss,
        endo_loss_head_forms with another one (``colors``: the two colour pointers, read with photometric_weight > 0 only)."""
        photo = self.photometric_weight > 0.0
        if self.consistency_loss != "distance":
            _lib.check(lib.endo_loss_head_forms(
                *tensors, *(colors if photo else (None, None)), self.sfl_weight, self.dcl_weight, self.photometric_weight, self.epsilon,
                models.PADDING_MODES[self.photometric_padding], *outputs[:-1], losses.CONSISTENCY_FORMS[self.consistency_loss][0],
                self.consistency_eps, outputs[-1]), "endo_loss_head_forms")
        elif photo:          # the masked network inputs are the term's colours (the head is fp32 under every storage mode)
            _lib.check(lib.endo_loss_head_photo(
                *tensors, *colors, self.sfl_weight, self.dcl_weight, self.photometric_weight, self.epsilon,
                models.PADDING_MODES[self.photometric_padding], *outputs), "endo_loss_head_photo")
        else:
            _lib.check(lib.endo_loss_head(*tensors, self.sfl_weight, self.dcl_weight, self.epsilon, *outputs), "endo_loss_head")

    def _fused_iteration(self, batch):
        """Network forward -> endo_loss_head (loss values and d loss / d prediction).  Everything is issued straight through the
        C ABI, without autograd nodes: the caller differentiates the network with ``_fused_backward`` after its guard, which
        saves the autograd engine's start-up latency (~0.1 ms of idle GPU after the loss synchronisation).
        Returns (losses tensor [total, dcl, sfl, flag] -- with photometric_weight > 0 endo_loss_head_photo's [total, dcl, sfl, flag, photo]
        --, network input, forward tape, predictions, d loss / d prediction)."""
        lib = _lib.load()
        self._display_source = None          # the previous call's masked input goes back to the allocator before this call's is taken
        b = _lib.dev_f32(batch["boundaries"], "boundaries")
        c1 = _lib.dev_f32(batch["colors_1"], "colors_1")
        c2 = _lib.dev_f32(batch["colors_2"], "colors_2")
        n, ch, h, w = c1.shape
        with torch.no_grad():
            x = torch.empty((2 * n, ch, h, w), dtype=torch.float32, device=c1.device)          # both frames, masked (train.py:272-273)
            _lib.check(lib.endo_mask_mul(_lib.ptr(c1), _lib.ptr(b), _lib.ptr(x[:n]), n, ch, h * w, _lib.stream()), "endo_mask_mul")
            _lib.check(lib.endo_mask_mul(_lib.ptr(c2), _lib.ptr(b), _lib.ptr(x[n:]), n, ch, h * w, _lib.stream()), "endo_mask_mul")
            if self.bf16_storage:
                pred, tape = self.model._run_forward16(x, 2, self.half_storage)       # both frames as two sample groups of one call
            else:
                pred, tape = self.model._run_forward(x, 2)          # (2N, 1, H, W): frame 1's predictions first
            photo = self.photometric_weight > 0.0
            need = int((lib.endo_loss_head_photo_workspace_floats if photo else lib.endo_loss_head_workspace_floats)(n, h, w))
            if self._head_ws is None or self._head_ws.numel() < need or self._head_ws.device != pred.device:
                self._head_ws = torch.empty(need, dtype=torch.float32, device=pred.device)
            losses_t = torch.empty(5 if photo else 4, dtype=torch.float32, device=pred.device)          # total, dcl, sfl, guard flag (, photo)
            grad_pred = torch.empty_like(pred)
            f = lambda key: _lib.ptr(_lib.dev_f32(batch[key], key))
            pose = lambda key, cols: _lib.ptr(_lib.dev_f32(batch[key], key).reshape(n, cols))
            tensors = [
                _lib.ptr(pred[:n]), _lib.ptr(pred[n:]), _lib.ptr(b), f("sparse_depths_1"), f("sparse_depths_2"),
                f("sparse_depth_masks_1"), f("sparse_depth_masks_2"), f("sparse_flows_1"), f("sparse_flows_2"),
                f("sparse_flow_masks_1"), f("sparse_flow_masks_2"), pose("translations_1_wrt_2", 3), pose("rotations_1_wrt_2", 9),
                pose("translations_2_wrt_1", 3), pose("rotations_2_wrt_1", 9), pose("intrinsics", 9)]
            outputs = [_lib.ptr(losses_t), _lib.ptr(grad_pred[:n]), _lib.ptr(grad_pred[n:]), _lib.ptr(self._head_ws), n, h, w, _lib.stream()]
            self._loss_head(lib, tensors, (_lib.ptr(x[:n]), _lib.ptr(x[n:])), outputs)
        self._display_source = (x, b)          # what display_panels() renders with the head workspace's planes
        return losses_t, x, tape, pred, grad_pred

    def _fused_backward(self, x, tape, grad_pred):
        with torch.no_grad():
            if self.bf16_storage:
                self.model._run_backward16(tuple(x.shape), tape, grad_pred, self.model.training, 2, self.half_storage)
            else:
                self.model._run_backward(x, tape, grad_pred, self.model.training, 2)

    def validation_losses(self, batch):
        """The validation body of reference train.py:403-444 for one batch: the two network forwards and the loss head, nothing else -- no
        backward, no all-reduce, no optimizer: parameters, ``.grad``, momentum and the gradient bucket stay as they are.  The network runs in
        its current mode; the reference validates in ``.train()`` mode (its model is never switched), so BatchNorm uses batch statistics and
        updates the running ones (frame 1's, then frame 2's).  The reference's ``torch.abs`` on the predictions (train.py:418-421) is the
        identity: the network's last operation is already ``torch.abs`` (models.py:186).  Returns the device fp32 [total, dcl, sfl, flag]
        (flag 1.0 when the total is NaN / Inf); nothing is read back to the host.  With the fused head (the default) this is
        ``_fused_iteration`` -- the loss head's backward half runs too, into its workspace and a scratch gradient; with fused_head=False it
        is ``losses()`` under ``torch.no_grad()``."""
        if self.fused_head:
            losses_t, _, _, _, _ = self._fused_iteration(batch)
            return losses_t
        with torch.no_grad():
            loss, dcl, sfl, extras = self.losses(batch)
            bad = (~torch.isfinite(loss)).to(torch.float32).reshape(1)
            parts = [loss.reshape(1), dcl.reshape(1), sfl.reshape(1), bad] + ([extras["photo"].reshape(1)] if "photo" in extras else [])
            return torch.cat(parts).to(torch.float32)

    def display_panels(self):
        """The display panel of this step's latest call -- training (``__call__``) or validation (``validation_losses``) -- as
        train.py:353-371 / 460-478 build it: the device uint8 (8 Hg, Wg, 3) R, G, B image of ``display.panels``.  Rendered from the planes
        the loss head left in its workspace (``endo_loss_head_planes``: scaled depths, masked flows, masked sparse flows) and the masked
        network input the call kept: no recompute.  Issue it on the stream of the call it renders, before the next call of this step
        (which overwrites the workspace).  Needs the fused loss head; on the module path use ``display.panels`` on ``losses()``' extras."""
        if not self.fused_head:
            raise RuntimeError("display_panels renders from the fused loss head's workspace; with fused_head=False build the panel with "
                               "display.panels from losses()' extras")
        source = self.__dict__.get("_display_source")
        if source is None:
            raise RuntimeError("display_panels: no training or validation call to render yet")
        x, b = source
        n2, _, h, w = x.shape
        n = n2 // 2
        offsets = (ctypes.c_int64 * 6)()
        _lib.check(_lib.load().endo_loss_head_planes(n, h, w, offsets), "endo_loss_head_planes")
        p = n * h * w
        ws = self._head_ws
        plane = lambda i, c: ws[offsets[i]:offsets[i] + c * p].view(n, c, h, w)
        return display.panels(x[:n], x[n:], plane(0, 1), plane(1, 1), b, plane(4, 2), plane(5, 2), plane(2, 2), plane(3, 2))

    def __call__(self, batch, lr=None):
        """One iteration.  Nothing in it waits for the host: the non-finite-loss guard (train.py:317-322) is a flag the loss head writes on
        the device, summed over ranks inside the gradient all-reduce and read by the optimizer kernel, which then leaves parameters and
        momentum untouched -- the reference's guarded branch also runs backward() and a step() that changes nothing.  Returns a
        ``StepOutput``: a mapping with the keys "loss", "dcl", "sfl", "grad_norm", "skipped" whose first access makes the one
        device-to-host read of the step (the reference's ``loss.item()``, train.py:317) -- a training loop that reads the PREVIOUS
        iteration's output after launching the current one never idles the GPU."""
        if lr is not None:
            for group in self.optimizer.param_groups:
                group["lr"] = lr
        self.optimizer.zero_grad()
        if self.fused_head:
            losses_t, x, tape, pred, grad_pred = self._fused_iteration(batch)
            self._fused_backward(x, tape, grad_pred)
        else:
            loss, dcl, sfl, extras = self.losses(batch)
            with torch.no_grad():
                bad = (~torch.isfinite(loss.detach())).to(torch.float32).reshape(1)
                parts = [loss.detach().reshape(1), dcl.detach().reshape(1), sfl.detach().reshape(1), bad]
                if "photo" in extras:
                    parts.append(extras["photo"].detach().reshape(1))
                losses_t = torch.cat(parts).to(torch.float32)
            loss.backward()
        scale, flag = self.bucket.all_reduce(losses_t[3:4])
        norm = self.optimizer.step(grad_scale=scale, skip_flag=flag)
        return StepOutput(losses_t, flag, norm, self._readback_slot(losses_t.device))

    def _readback_slot(self, device):
        """A set of pinned host buffers + an event out of a small ring: the numbers of a step are copied out asynchronously right
        behind the optimizer kernel, so that reading step k - 1 after launching step k waits for step k - 1 only."""
        if device.type != "cuda":
            return None
        ring = self.__dict__.setdefault("_readback_ring", [])
        if len(ring) < 8:
            ring.append(_ReadbackSlot())
            return ring[-1]
        self._readback_next = (self.__dict__.get("_readback_next", -1) + 1) % len(ring)
        slot = ring[self._readback_next]
        slot.release()          # an output issued 8 steps ago and never read takes its values now (its copy finished long ago)
        return slot


def _distill_head(pred, goal, boundaries, weight, epsilon, accumulate, losses_t, grad_pred):
    """endo_distill_head on the packed (2N, 1, H, W) predictions of student and teacher (frame 1's samples first)."""
    n2, _, h, w = pred.shape
    n = n2 // 2
    stats = torch.empty(6 * n, dtype=torch.float64, device=pred.device)
    _lib.check(_lib.load().endo_distill_head(
        _lib.ptr(pred[:n]), _lib.ptr(pred[n:]), _lib.ptr(goal[:n]), _lib.ptr(goal[n:]), _lib.ptr(boundaries), weight, epsilon,
        1 if accumulate else 0, _lib.ptr(losses_t), _lib.ptr(grad_pred[:n]), _lib.ptr(grad_pred[n:]), _lib.ptr(stats), n, h * w,
        _lib.stream()), "endo_distill_head")


class DistillationStep(TrainingStep):
    """One teacher-student iteration: reference utils.learn_from_teacher (utils.py:1462-1482) followed by train.py's guard, clip and SGD
    on the student (train.py:317-328), fused like ``TrainingStep``: colours * boundary once -> teacher forward (no_grad, its tape
    dropped) -> student forward -> ``endo_distill_head`` -> student backward -> ONE all-reduce of gradients + flag -> fused clip + SGD.

      distill = distill_weight * 0.5 * (ScaleInvariantLoss(|student(c1)|, |teacher(c1)|, b) + the same for frame 2)

    *Pure mode* (both SfM weights 0, the default): the loss is that term, the batch needs only ``colors_1``, ``colors_2`` and
    ``boundaries``.  *Combined mode* (sfl_weight or dcl_weight > 0; not in the reference: train.py's body plus learn_from_teacher's term):
    ``endo_loss_head`` on the student's predictions, then ``endo_distill_head(accumulate=1)`` into the same losses and d loss / d
    prediction; the batch is a training batch.  The teacher runs in its own current mode; in ``.eval()``, the intended use, a call
    leaves its parameters, BatchNorm buffers and ``num_batches_tracked`` bit for bit and creates no gradient buffer.  fp32 only.
    The ``StepOutput`` has "loss", "dcl", "sfl" (0 in pure mode), "distill", "grad_norm" and "skipped"."""

    def __init__(self, student, teacher, optimizer, height, width, distill_weight=1.0, sfl_weight=0.0, dcl_weight=0.0, epsilon=1.0e-8,
                 consistency_loss="distance"):
        if teacher is student:
            raise ValueError("DistillationStep: teacher and student are the same module")
        for name, value in (("distill_weight", distill_weight), ("sfl_weight", sfl_weight), ("dcl_weight", dcl_weight)):
            if not float(value) >= 0.0:
                raise ValueError("%s must be >= 0 (got %r)" % (name, value))
        for name, model in (("student", student), ("teacher", teacher)):
            if not hasattr(model, "_run_forward"):
                raise ValueError("DistillationStep: the %s must be a models.FCDenseNet (the step drives its C entry points)" % name)
        if student.flat_parameters().device != teacher.flat_parameters().device:
            raise ValueError("DistillationStep: student on %s, teacher on %s" % (student.flat_parameters().device,
                                                                                   teacher.flat_parameters().device))
        TrainingStep.__init__(self, student, optimizer, height, width, sfl_weight=sfl_weight, dcl_weight=dcl_weight, epsilon=epsilon,
                              consistency_loss=consistency_loss)          # combined mode's loss head; pure mode has no consistency term
        self.teacher = teacher
        self.distill_weight = float(distill_weight)
        self.combined = self.sfl_weight > 0.0 or self.dcl_weight > 0.0
        distributed.sync_parameters(teacher)

    def losses(self, batch):
        raise RuntimeError("DistillationStep has no module path; use utils.learn_from_teacher with losses.ScaleInvariantLoss")

    def _fused_iteration(self, batch):
        """Teacher forward -> student forward -> (combined mode: endo_loss_head ->) endo_distill_head.  Returns what
        ``TrainingStep._fused_iteration`` does; the losses tensor is [total, dcl, sfl, flag, distill]."""
        lib = _lib.load()
        self._display_source = None
        b = _lib.dev_f32(batch["boundaries"], "boundaries")
        c1 = _lib.dev_f32(batch["colors_1"], "colors_1")
        c2 = _lib.dev_f32(batch["colors_2"], "colors_2")
        n, ch, h, w = c1.shape
        with torch.no_grad():
            x = torch.empty((2 * n, ch, h, w), dtype=torch.float32, device=c1.device)
            _lib.check(lib.endo_mask_mul(_lib.ptr(c1), _lib.ptr(b), _lib.ptr(x[:n]), n, ch, h * w, _lib.stream()), "endo_mask_mul")
            _lib.check(lib.endo_mask_mul(_lib.ptr(c2), _lib.ptr(b), _lib.ptr(x[n:]), n, ch, h * w, _lib.stream()), "endo_mask_mul")
            goal, _ = self.teacher._run_forward(x, 2)          # two sample groups, as the student's; the tape goes back to the allocator
            pred, tape = self.model._run_forward(x, 2)
            losses_t = torch.empty(5, dtype=torch.float32, device=pred.device)
            grad_pred = torch.empty_like(pred)
            if self.combined:
                need = int(lib.endo_loss_head_workspace_floats(n, h, w))
                if self._head_ws is None or self._head_ws.numel() < need or self._head_ws.device != pred.device:
                    self._head_ws = torch.empty(need, dtype=torch.float32, device=pred.device)
                f = lambda key: _lib.ptr(_lib.dev_f32(batch[key], key))
                pose = lambda key, cols: _lib.ptr(_lib.dev_f32(batch[key], key).reshape(n, cols))
                tensors = [
                    _lib.ptr(pred[:n]), _lib.ptr(pred[n:]), _lib.ptr(b), f("sparse_depths_1"), f("sparse_depths_2"),
                    f("sparse_depth_masks_1"), f("sparse_depth_masks_2"), f("sparse_flows_1"), f("sparse_flows_2"),
                    f("sparse_flow_masks_1"), f("sparse_flow_masks_2"), pose("translations_1_wrt_2", 3), pose("rotations_1_wrt_2", 9),
                    pose("translations_2_wrt_1", 3), pose("rotations_2_wrt_1", 9), pose("intrinsics", 9)]
                self._loss_head(lib, tensors, (None, None), [_lib.ptr(losses_t), _lib.ptr(grad_pred[:n]), _lib.ptr(grad_pred[n:]),
                                                             _lib.ptr(self._head_ws), n, h, w, _lib.stream()])
            _distill_head(pred, goal, b, self.distill_weight, self.epsilon, self.combined, losses_t, grad_pred)
        if self.combined:
            self._display_source = (x, b)
        return losses_t, x, tape, pred, grad_pred

    def validation_losses(self, batch):
        """The forward part for one batch -- both networks and the head(s), no student backward, no all-reduce, no optimizer: the device
        fp32 [total, dcl, sfl, flag, distill].  ``validate(step, ...)`` takes its running means from the first three."""
        return self._fused_iteration(batch)[0]

    def display_panels(self):
        """``TrainingStep.display_panels`` in combined mode; pure mode has no loss-head planes to render."""
        if not self.combined:
            raise RuntimeError("display_panels: a DistillationStep in pure mode (sfl_weight = dcl_weight = 0) runs no loss head, so "
                               "there are no planes to render")
        return TrainingStep.display_panels(self)

    def __call__(self, batch, lr=None):
        """One iteration, as ``TrainingStep.__call__``; the ``StepOutput``'s fifth value is "distill"."""
        if lr is not None:
            for group in self.optimizer.param_groups:
                group["lr"] = lr
        self.optimizer.zero_grad()
        losses_t, x, tape, pred, grad_pred = self._fused_iteration(batch)
        self._fused_backward(x, tape, grad_pred)
        scale, flag = self.bucket.all_reduce(losses_t[3:4])
        norm = self.optimizer.step(grad_scale=scale, skip_flag=flag)
        return StepOutput(losses_t, flag, norm, self._readback_slot(losses_t.device), fifth="distill")


ValidationResult = collections.namedtuple("ValidationResult", ["mean_loss", "mean_depth_consistency_loss", "mean_sparse_flow_loss",
                                                               "running_means", "losses"])
ValidationResult.__doc__ = """What ``validate`` returns: the three running means after the last batch as Python floats (the values train.py's
mean_loss, mean_depth_consistency_loss and mean_sparse_flow_loss hold after its validation loop, bit for bit), ``running_means`` the
float64 numpy (B, 3) means after each batch (what train.py:481-483 logs per batch) and ``losses`` the float32 numpy (B, 3) per-batch
[total, dcl, sfl]."""


def validate(step, batches, initial=None, display_each=None, on_display=None):
    """The validation pass of reference train.py:378-485 with a TrainingStep: ``step.validation_losses`` on every batch of ``batches`` (for
    example ``dataset.TrainingBatches(..., transform=None, shuffle=False)``, the reference's validation loader), the running means of
    train.py:446-456 updated on the device by ``endo_validation_accumulate`` (fp64), and ``on_display(batch_index, panel)`` with the device
    uint8 panel of ``step.display_panels()`` when ``batch_index % display_each == 0`` (the callback may keep the tensor; hand it to
    ``display.stack_and_display`` for a TensorBoard writer).  Nothing in the pass reads the device per batch: the means, their per-batch
    history and the per-batch losses come back in one read at the end.

    initial: the three means (loss, depth consistency, sparse flow) before the pass, default NaN -- in the reference a NaN batch 0 leaves
    the Python variables as the training loop left them, so pass the training means to reproduce that.  With world > 1 each rank's
    result covers its own batches (the reference has one process); averaging across ranks is the caller's.  Returns a
    ``ValidationResult``; the checkpoint name of train.py:486-488 is
    ``'checkpoint_model_epoch_{}_validation_{}.pt'.format(epoch, result.mean_sparse_flow_loss)``."""
    nan = float("nan")
    initial = (nan, nan, nan) if initial is None else tuple(float(v) for v in initial)
    if len(initial) != 3:
        raise ValueError("initial must hold three means (loss, depth consistency, sparse flow)")
    if display_each is not None:
        display_each = int(display_each)
        if display_each <= 0:
            raise ValueError("display_each must be a positive number of batches (got %d)" % display_each)
        if on_display is None:
            raise ValueError("display_each needs an on_display(batch_index, panel) callback")
        if not step.fused_head:
            raise ValueError("validate(display_each=...) renders through TrainingStep.display_panels, which needs the fused loss head")
    elif on_display is not None:
        raise ValueError("on_display needs display_each")
    lib = _lib.load()
    means = history = None
    per_batch = []
    count = 0
    for index, batch in enumerate(batches):
        losses_t = _lib.dev_f32(step.validation_losses(batch), "validation losses")
        if means is None:
            means = torch.tensor(initial, dtype=torch.float64, device=losses_t.device)
            history = torch.empty((max(1, len(batches)) if hasattr(batches, "__len__") else 64, 3), dtype=torch.float64, device=losses_t.device)
        if index >= history.shape[0]:
            grown = torch.empty((2 * history.shape[0], 3), dtype=torch.float64, device=history.device)
            grown[:history.shape[0]].copy_(history)
            history = grown
        _lib.check(lib.endo_validation_accumulate(_lib.ptr(losses_t), index, _lib.ptr(means), _lib.ptr(history), _lib.stream()),
                   "endo_validation_accumulate")
        per_batch.append(losses_t[:3])
        if display_each is not None and index % display_each == 0:
            on_display(index, step.display_panels())
        count = index + 1
    if means is None:
        return ValidationResult(initial[0], initial[1], initial[2], torch.empty((0, 3), dtype=torch.float64).numpy(),
                                torch.empty((0, 3), dtype=torch.float32).numpy())
    host = torch.cat([means, history[:count].reshape(-1), torch.stack(per_batch).double().reshape(-1)]).cpu()          # the one read
    mean = host[:3].tolist()
    running = host[3:3 + 3 * count].reshape(count, 3).numpy()
    losses_host = host[3 + 3 * count:].reshape(count, 3).float().numpy()
    return ValidationResult(mean[0], mean[1], mean[2], running, losses_host)


class _ReadbackSlot(object):
    def __init__(self):
        self.losses = torch.empty(5, dtype=torch.float32).pin_memory()          # the fifth: the photometric or distillation term, when the step has one
        self.flag = torch.empty(1, dtype=torch.float32).pin_memory()
        self.norm = torch.empty(1, dtype=torch.float64).pin_memory()
        self.event = torch.cuda.Event()
        self.owner = None

    def release(self):
        owner = self.owner() if self.owner is not None else None
        if owner is not None:
            owner._read()
        self.owner = None


class StepOutput(object):
    """What one TrainingStep call produced: [total, dcl, sfl] losses, the guard flag after the ranks' consensus and the pre-clip
    gradient norm, copied to pinned host buffers asynchronously right behind the step's last kernel (three copies of a few bytes, no
    kernel).  Read like the dict older versions returned; the first read waits for THOSE copies, not for whatever was queued after
    them.  "loss" is a float; "dcl" / "sfl" / "grad_norm" are 0-dim host tensors (NaN for a skipped step's terms, as before);
    "skipped" is a bool.  A step with photometric_weight > 0 also has "photo", like "dcl"; ``fifth`` names the fifth loss of another
    step ("distill" for a DistillationStep)."""

    def __init__(self, losses, flag, norm, slot, fifth="photo"):
        import weakref
        self._fifth = fifth
        self._host = None
        self._slot = slot
        self._count = int(losses.numel())          # 4, or 5 with the photometric term
        if slot is None:          # host tensors (CPU tests of the glue): copies -- with world > 1 `flag` is a view of the gradient bucket's trailing slot, which the next step overwrites before a one-step-late read
            self._vals = (losses.detach().clone(), flag.detach().clone(), norm.detach().clone())
        else:
            slot.losses[:self._count].copy_(losses, non_blocking=True)
            slot.flag.copy_(flag.reshape(1), non_blocking=True)
            slot.norm.copy_(norm.reshape(1), non_blocking=True)
            slot.event.record()
            slot.owner = weakref.ref(self)

    def _read(self):
        if self._host is None:
            if self._slot is not None:
                self._slot.event.synchronize()
                losses, flag, norm = self._slot.losses[:self._count].tolist(), self._slot.flag.tolist(), self._slot.norm.tolist()
                self._slot.owner = None
                self._slot = None
            else:
                losses, flag, norm = (t.reshape(-1).tolist() for t in self._vals)
                self._vals = None
            skipped = flag[0] != 0.0
            nan = float("nan")
            self._host = {"loss": losses[0], "dcl": torch.tensor(nan if skipped else losses[1]), "sfl": torch.tensor(nan if skipped else losses[2]),
                          "grad_norm": torch.tensor(norm[0], dtype=torch.float64), "skipped": skipped}
            if self._count > 4:
                self._host[self._fifth] = torch.tensor(nan if skipped else losses[4])
        return self._host

    def __getitem__(self, key):
        return self._read()[key]

    def __contains__(self, key):
        return key in ("loss", "dcl", "sfl", "grad_norm", "skipped") or (key == self._fifth and self._count > 4)

    def keys(self):
        return self._read().keys()

    def items(self):
        return self._read().items()

    def __repr__(self):
        return "StepOutput(%r)" % (self._read(),)
