"""The test phase of the reference's evaluate.py (279-346): per frame one masked depth map, one colour|depth PNG panel and one
coloured PLY point cloud, for batches of frames (dataset.TestFrames) on the device.

    per batch   boundaries * colors -> the network in eval mode -> endo_evaluate (csrc/evaluate.hip: three launches whatever the batch
                size): masked depth, the (N, H, 2W, 3) BGR panels, the point clouds of all frames and their offsets; one host read
    per frame   utils.write_png / utils.write_point_cloud on a small writer pool, while the next batch is decoded and run

The reference needs cv2 and plyfile here and runs one frame per batch with all per-pixel work on the host (evaluate.py:292, 329-345).

The same frames with poses from the electromagnetic tracker (reader.read_initial_pose_file) give the reference's posed test output
(utils.write_test_output_with_initial_pose, utils.py:1316-1355): posed_test_outputs / run_posed_test_phase over endo_evaluate_posed
(csrc/evaluate_posed.hip, three launches per batch) write each frame's colour image, depth image and a point cloud normalised to a z
range of 20 units and moved into the tracker's frame, and the whole sequence as one merged cloud.

The validation phase (evaluate.py:119-277) compares a trained network with the sparse reconstruction of a sequence, for batches of
pairs (dataset.TrainingBatches(transform=None, shuffle=False): the reference's SfMDataset(phase="validation")):

    per batch   validation_outputs: the masked pair through the network in eval mode, depth scaling, flows from depth and warped
                depths in both directions with the training step's modules, then endo_evaluate_validation (csrc/
                evaluate_validation.hip: three launches): the 12-section panel, AbsRelError / Threshold of both frames and the point
                clouds of frame 1; one host read
    per batch   run_validation_phase: ``<batch>.png`` and ``<batch>.ply`` on the writer pool, the metrics read once at the end

The reference cannot run this phase as written: it unpacks 17 items from the loader's 18 (evaluate.py:167-171) and needs cv2,
torchvision, plyfile and tensorboardX.

What the reference leaves to another tool (its README, step 4: register the predicted point clouds to the CT model with a similarity
transformation "to calculate residual errors") is registration_errors over the points / offsets any of the outputs above return, and
run_registration_phase: the posed test outputs per batch, each frame's cloud registered to a registration.TargetModel from the tracker's
pose as its start, ``registration_errors.csv`` and the registered clouds.

run_fusion_phase makes one model of the sequence before that step: the posed outputs per batch, their depth maps fused into a
fusion.TSDFVolume around the posed clouds' bounding box (csrc/fusion.hip), the surface written as ``fused_surface.ply`` and, with a
target, registered once.  With refine=K the frames are first tracked against that volume (csrc/fusion_track.hip) and fused again
under the refined poses and scales, K times.

model_depth_errors / run_model_depth_phase measure the predictions against a surface that does not come from them: a mesh.TriangleMesh
(the CT model) drawn from each frame's camera (csrc/mesh_render.hip), the prediction scaled to that depth over the pixels the model
covers and the reference's AbsRel and sigma 1, 2, 3 there -- ``model_depth_errors.csv``.
"""

import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, display, fusion, losses, mesh as mesh_module, models, registration, utils
from .train_step import mask_mul


def _device_f32(t, shape, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a float32 device tensor of shape %s" % (name, tuple(shape)))
    return t.contiguous()


def _checked_inputs(colors, boundaries, predictions, intrinsics):
    """The four inputs of the two *_from_predictions functions, checked and contiguous, and the batch's (N, H, W)."""
    n, _, height, width = (int(v) for v in colors.shape)
    return (_device_f32(colors, (n, 3, height, width), "colors"), _device_f32(boundaries, (n, 1, height, width), "boundaries"),
            _device_f32(predictions, (n, 1, height, width), "predictions"), _device_f32(intrinsics, (n, 3, 3), "intrinsics"), n, height, width)


def _masked_forward(model, batch, caller):
    """evaluate.py:323-327 for a TestFrames batch: the network in eval mode on ``boundaries * colors``.  Returns the masked input,
    the boundaries, the predictions and the intrinsics."""
    if model.training:
        raise RuntimeError("%s runs the network in eval mode: call model.eval() first (evaluate.py:313)" % caller)
    colors = batch["colors"]
    if not torch.is_tensor(colors) or colors.dim() != 4 or colors.shape[1] != 3:
        raise ValueError("colors must be an (N, 3, H, W) tensor")
    n, _, height, width = (int(v) for v in colors.shape)
    colors = _device_f32(colors, (n, 3, height, width), "colors")
    boundaries = _device_f32(batch["boundaries"], (n, 1, height, width), "boundaries")
    intrinsics = _device_f32(batch["intrinsics"], (n, 3, 3), "intrinsics")
    with torch.no_grad(), torch.cuda.device(colors.device):
        masked = boundaries * colors          # evaluate.py:325
        pred = model(masked)
    return masked, boundaries, pred, intrinsics


class _WriterPool:
    """The writer threads of a run_* phase.  submit(fn, *args) records an event behind the non-blocking copies queued so far and
    runs fn(event, *args) on a thread; at most 2 * writers batches of host copies are in flight; leaving the block waits for every
    file and re-raises a writer's exception, after an exception in the block too."""

    def __init__(self, writers):
        self._bound = 2 * max(1, int(writers))
        self._pool = ThreadPoolExecutor(max(1, int(writers)))
        self._pending = deque()

    def __enter__(self):
        return self

    def submit(self, fn, *args):
        ready = torch.cuda.Event()
        ready.record()
        self._pending.append(self._pool.submit(fn, ready, *args))
        while len(self._pending) > self._bound:          # bound the host copies in flight
            self._pending.popleft().result()

    def __exit__(self, *exc):
        try:
            while self._pending:
                self._pending.popleft().result()
        finally:
            self._pool.shutdown(wait=True)
        return False


def test_outputs(model, batch, is_hsv=False, point_cloud_downsampling=1):
    """evaluate.py:323-344 for a TestFrames batch: the network on ``boundaries * colors`` and the per-frame outputs, on the device.
    Returns a dictionary: colors (the masked network input), predictions, depth (N, 1, H, W) fp32, panels (N, H, 2W, 3) uint8 B, G, R
    (what evaluate.py:345 hands to cv2.imwrite), points (capacity N * H * W rows of x, y, z, r, g, b) and offsets: the host list of N + 1
    row offsets, frame f's points being points[offsets[f]:offsets[f + 1]] -- the batch's one read back to the host."""
    masked, boundaries, pred, intrinsics = _masked_forward(model, batch, "test_outputs")
    out = outputs_from_predictions(masked, boundaries, pred, intrinsics, is_hsv, point_cloud_downsampling)
    out["colors"], out["predictions"] = masked, pred
    return out


def outputs_from_predictions(colors, boundaries, predictions, intrinsics, is_hsv=False, point_cloud_downsampling=1):
    """endo_evaluate on a batch: colors (N, 3, H, W) the masked network input, boundaries (N, 1, H, W) in {0, 1}, predictions
    (N, 1, H, W) the network's output, intrinsics (N, 3, 3), all fp32 on the device.  Returns depth, panels, points and the host list
    of offsets as test_outputs does."""
    colors, boundaries, predictions, intrinsics, n, height, width = _checked_inputs(colors, boundaries, predictions, intrinsics)
    lib = _lib.load()
    dev = colors.device
    need = int(lib.endo_evaluate_workspace_bytes(n, height, width))
    if need < 0:
        raise ValueError("a batch of %d frames of %d x %d is outside endo_evaluate's sizes" % (n, height, width))
    with torch.cuda.device(dev):
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        depth = torch.empty((n, 1, height, width), dtype=torch.float32, device=dev)
        panels = torch.empty((n, height, 2 * width, 3), dtype=torch.uint8, device=dev)
        points = torch.empty((n * height * width, 6), dtype=torch.float32, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.endo_evaluate(_lib.ptr(colors), _lib.ptr(boundaries), _lib.ptr(predictions), _lib.ptr(intrinsics), n, height, width,
                                     1 if is_hsv else 0, int(point_cloud_downsampling), _lib.ptr(depth), _lib.ptr(panels), _lib.ptr(points),
                                     _lib.ptr(offsets), _lib.ptr(workspace), need, _lib.stream()), "endo_evaluate")
        host_offsets = offsets.cpu().tolist()          # the batch's one read back (it waits for the stream)
    return {"depth": depth, "panels": panels, "points": points, "offsets": host_offsets}


def _write_frames(ready, names, panels, points, offsets, out_dir, write_png, write_ply, ply_text):
    """One batch's files, on a writer thread, once the device-to-host copies have landed."""
    ready.synchronize()
    for f, name in enumerate(names):
        if write_ply:
            utils.write_point_cloud(os.path.join(out_dir, "{}.ply".format(name)), points[offsets[f]:offsets[f + 1]].numpy(), text=ply_text)
        if write_png:
            utils.write_png(os.path.join(out_dir, "{}.png".format(name)), panels[f].numpy())


def run_test_phase(model, frames, out_dir, write_png=True, write_ply=True, ply_text=True, point_cloud_downsampling=1, writers=4):
    """evaluate.py:317-346: every batch of ``frames`` (a dataset.TestFrames) through test_outputs, then ``<name>.png`` (the colour|depth
    panel) and ``<name>.ply`` (the point cloud; text=False: binary_little_endian) in ``out_dir`` for each frame.  The files are
    formatted and written on ``writers`` threads from pinned host copies, so the next batch's decode and forward do not wait for them.
    Returns the number of frames."""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    count = 0
    with _WriterPool(writers) as pool:
        for batch in frames:
            out = test_outputs(model, batch, is_hsv=frames.is_hsv, point_cloud_downsampling=point_cloud_downsampling)
            names = list(batch["names"])
            count += len(names)
            if not (write_png or write_ply):
                continue
            offsets = out["offsets"]
            panels = out["panels"].to("cpu", non_blocking=True) if write_png else None
            points = out["points"][:offsets[-1]].to("cpu", non_blocking=True) if write_ply else None
            pool.submit(_write_frames, names, panels, points, offsets, out_dir, write_png, write_ply, ply_text)
    return count


def _poses_f64(rotations, translations, n, dev):
    """(N, 3, 3) and (N, 3) float64 device tensors of per-frame poses given as arrays, tensors or lists of per-frame arrays."""
    def as_tensor(x, shape, name):
        if torch.is_tensor(x):
            t = x.detach().to(dtype=torch.float64)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray([np.asarray(v, np.float64) for v in x], np.float64)))
        if t.numel() != int(np.prod(shape)):
            raise ValueError("%s must hold %s float64 values" % (name, tuple(shape)))
        return t.reshape(shape).contiguous().to(dev)
    return as_tensor(rotations, (n, 3, 3), "rotations"), as_tensor(translations, (n, 3), "translations")


def posed_outputs_from_predictions(colors, boundaries, predictions, intrinsics, rotations, translations, is_hsv=False,
                                   point_cloud_downsampling=1, min_threshold=None, max_threshold=None):
    """endo_evaluate_posed (csrc/evaluate_posed.hip, three launches whatever the batch size) on a batch: what the reference's
    utils.write_test_output_with_initial_pose (utils.py:1316-1355) computes per frame on the host.  colors (N, 3, H, W) the masked network
    input, boundaries (N, 1, H, W) in {0, 1}, predictions (N, 1, H, W), intrinsics (N, 3, 3), fp32 on the device; rotations (N, 3, 3) and
    translations (N, 3) float64, each frame's pose in the tracker's frame (arrays, tensors or lists of per-frame arrays).
    min_threshold / max_threshold, when both are given, are utils.py:1285-1288's colour test (compared as float32).
    Returns a dictionary: depth (N, 1, H, W); color_images (N, H, W, 3) uint8 in the reference's channel order -- an RGB input stays
    R, G, B (the reference has no RGB -> BGR swap before cv2.imwrite, so its colour files have red and blue exchanged), an HSV input
    becomes B, G, R; depth_images (N, H, W, 3) uint8 B, G, R; points (capacity N * H * W rows of x, y, z, r, g, b with (r, g, b) =
    channels (2, 1, 0) of the colour image, as the reference reads them); offsets, the host list of N + 1 row offsets; ranges, the host
    (N, 2) float32 array of each frame's (z_min, z_max) over its kept pixels: (+inf, -inf) for a frame without kept pixels (the
    reference raises ZeroDivisionError there: its sentinels are Python ints), z_min == z_max for a frame whose coordinates are not
    finite (scale = 20 / 0).  Offsets and ranges are the batch's one read back to the host."""
    colors, boundaries, predictions, intrinsics, n, height, width = _checked_inputs(colors, boundaries, predictions, intrinsics)
    lib = _lib.load()
    dev = colors.device
    rotations, translations = _poses_f64(rotations, translations, n, dev)
    use_thr = max_threshold is not None and min_threshold is not None
    need = int(lib.endo_evaluate_posed_workspace_bytes(n, height, width))
    if need < 0:
        raise ValueError("a batch of %d frames of %d x %d is outside endo_evaluate_posed's sizes" % (n, height, width))
    with torch.cuda.device(dev):
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        depth = torch.empty((n, 1, height, width), dtype=torch.float32, device=dev)
        color_images = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
        depth_images = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
        points = torch.empty((n * height * width, 6), dtype=torch.float32, device=dev)
        meta = torch.empty(8 * (n + 1) + 8 * n, dtype=torch.uint8, device=dev)          # offsets, then ranges: one read
        offsets = meta[:8 * (n + 1)].view(torch.int64)
        ranges = meta[8 * (n + 1):].view(torch.float32)
        _lib.check(lib.endo_evaluate_posed(_lib.ptr(colors), _lib.ptr(boundaries), _lib.ptr(predictions), _lib.ptr(intrinsics),
                                           _lib.ptr(rotations), _lib.ptr(translations), n, height, width, 1 if is_hsv else 0,
                                           int(point_cloud_downsampling), 1 if use_thr else 0, float(min_threshold) if use_thr else 0.0,
                                           float(max_threshold) if use_thr else 0.0, _lib.ptr(depth), _lib.ptr(color_images),
                                           _lib.ptr(depth_images), _lib.ptr(points), _lib.ptr(offsets), _lib.ptr(ranges),
                                           _lib.ptr(workspace), need, _lib.stream()), "endo_evaluate_posed")
        host = meta.cpu().numpy()          # the batch's one read back (it waits for the stream)
    return {"depth": depth, "color_images": color_images, "depth_images": depth_images, "points": points,
            "offsets": host[:8 * (n + 1)].view(np.int64).tolist(), "ranges": host[8 * (n + 1):].view(np.float32).reshape(n, 2).copy()}


def posed_test_outputs(model, batch, rotations, translations, is_hsv=False, point_cloud_downsampling=1, min_threshold=None,
                       max_threshold=None):
    """A TestFrames batch through the network in eval mode on ``boundaries * colors`` (evaluate.py:323-327) and
    posed_outputs_from_predictions with the batch's poses.  Returns its dictionary plus colors (the masked input) and predictions."""
    masked, boundaries, pred, intrinsics = _masked_forward(model, batch, "posed_test_outputs")
    out = posed_outputs_from_predictions(masked, boundaries, pred, intrinsics, rotations, translations, is_hsv, point_cloud_downsampling,
                                         min_threshold, max_threshold)
    out["colors"], out["predictions"] = masked, pred
    return out


def _write_posed_frames(ready, names, color_images, depth_images, points, offsets, out_dir, write_ply, ply_text):
    """One batch's files, on a writer thread, once the device-to-host copies have landed."""
    ready.synchronize()
    for f, name in enumerate(names):
        if write_ply:
            utils.write_point_cloud(os.path.join(out_dir, "test_point_cloud_{}.ply".format(name)),
                                    points[offsets[f]:offsets[f + 1]].numpy(), text=ply_text)
        if color_images is not None:
            utils.write_png(os.path.join(out_dir, "test_color_{}.png".format(name)), color_images[f].numpy())
            utils.write_png(os.path.join(out_dir, "test_depth_{}.png".format(name)), depth_images[f].numpy())


def _write_merged(ready, path, parts, ply_text):
    ready.synchronize()
    rows = np.concatenate([p.numpy() for p in parts], axis=0) if parts else np.zeros((0, 6), np.float32)
    utils.write_point_cloud(path, rows, text=ply_text)


def run_posed_test_phase(model, frames, translation_dict, rotation_dict, out_dir, write_images=True, write_ply=True, ply_text=True,
                         merged="sequence.ply", point_cloud_downsampling=1, min_threshold=None, max_threshold=None, writers=4):
    """The reference's posed test output for a sequence (utils.write_test_output_with_initial_pose, utils.py:1316-1355, over a test-phase
    loader): every batch of ``frames`` (a dataset.TestFrames) through posed_test_outputs with the poses
    ``translation_dict[name]`` / ``rotation_dict[name]`` (reader.read_initial_pose_file), then per frame
    ``test_point_cloud_<name>.ply``, ``test_color_<name>.png`` and ``test_depth_<name>.png`` in ``out_dir``: the reference's file names with
    PNG in place of JPEG (there is no JPEG entropy coder here; the pixels are the ones the reference hands to cv2.imwrite, red and blue
    exchanged for RGB input included).  All clouds are in the tracker's frame, so ``merged`` (a file name in ``out_dir``, or None) also
    gets the whole sequence as one cloud, frame after frame.  A frame without kept pixels writes an empty cloud (the reference raises
    ZeroDivisionError); a frame whose kept depths are all equal has non-finite coordinates, as in the reference: its own file is
    written so, and it is left out of the merged cloud.  A frame whose name is missing from either dictionary raises KeyError before
    anything runs.  The files are written on run_test_phase's writer pool.
    Returns a dictionary: frames (the number of frames), empty and zero_range (the names of those two kinds of frames) and
    merged_points (the number of rows of the merged cloud)."""
    names_ahead = getattr(frames, "image_file_names", None)
    if names_ahead is not None:
        for name in names_ahead:
            key = os.path.basename(str(name))[-12:-4]
            translation_dict[key], rotation_dict[key]          # KeyError before anything runs
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    count, merged_points = 0, 0
    empty, zero_range, parts = [], [], []
    with _WriterPool(writers) as pool:
        for batch in frames:
            names = list(batch["names"])
            rotations = [rotation_dict[name] for name in names]
            translations = [translation_dict[name] for name in names]
            out = posed_test_outputs(model, batch, rotations, translations, is_hsv=getattr(frames, "is_hsv", False),
                                     point_cloud_downsampling=point_cloud_downsampling, min_threshold=min_threshold,
                                     max_threshold=max_threshold)
            count += len(names)
            offsets, ranges = out["offsets"], out["ranges"]
            good = []
            for f, name in enumerate(names):
                if ranges[f, 0] > ranges[f, 1]:
                    empty.append(name)
                elif ranges[f, 0] == ranges[f, 1]:
                    zero_range.append(name)
                else:
                    good.append(f)
                    merged_points += offsets[f + 1] - offsets[f]
            if not (write_images or write_ply):
                continue
            color_images = out["color_images"].to("cpu", non_blocking=True) if write_images else None
            depth_images = out["depth_images"].to("cpu", non_blocking=True) if write_images else None
            points = out["points"][:offsets[-1]].to("cpu", non_blocking=True) if write_ply else None
            if write_ply and merged:
                parts.extend(points[offsets[f]:offsets[f + 1]] for f in good)
            pool.submit(_write_posed_frames, names, color_images, depth_images, points, offsets, out_dir, write_ply, ply_text)
        if write_ply and merged:
            pool.submit(_write_merged, os.path.join(out_dir, str(merged)), parts, ply_text)
    return {"frames": count, "empty": empty, "zero_range": zero_range, "merged_points": int(merged_points)}


VALIDATION_TITLE ="Results (c1, sd1, d1, wd1, sf1, df1, c2, sd2, d2, wd2, sf2, df2)"          # evaluate.py:258


def validation_outputs(model, batch, epsilon=1.0e-8, is_hsv=False, point_cloud_downsampling=1):
    """evaluate.py:189-274 for a TrainingBatches batch, on the device, under no_grad: the masked colours and sparse flows, the two
    forward passes (one grouped call where the model has forward_pair), DepthScalingLayer, FlowfromDepthLayer in both directions
    (masked) and DepthWarpingLayer in both directions, then one endo_evaluate_validation call.  The reference's torch.abs on the
    predictions (evaluate.py:197, 199) is the identity: the network ends in an absolute value (models.py:186).
    Returns a dictionary of device tensors -- colors_1/2 (masked), sparse_flows_1/2 (masked), predictions_1/2, scaled_depths_1/2,
    flows_1/2 (masked), warped_depths_2_to_1 / _1_to_2, intersect_masks_1/2, panel (12 Hg, Wg, 3) uint8 R, G, B, metrics (N, 2, 4)
    [abs rel, sigma 1, 2, 3] per pair and frame, points (capacity N H W rows) -- and offsets: the host list of N + 1 row offsets,
    pair f's cloud (its frame 1) being points[offsets[f]:offsets[f + 1]] -- the batch's one read back to the host.
    The point colours are the frame's own R, G, B (the reference converts them with COLOR_HSV2BGR_FULL whatever the colour space,
    evaluate.py:202-203); is_hsv=True is not implemented (display.validation_panels)."""
    if model.training:
        raise RuntimeError("validation_outputs runs the network in eval mode: call model.eval() first (evaluate.py:164)")
    if is_hsv:
        raise NotImplementedError("HSV display panels: the reference converts the float colour grid with cv2.COLOR_HSV2RGB_FULL's float path, "
                                  "which is not implemented")
    b = _lib.dev_f32(batch["boundaries"], "boundaries")
    eps = float(epsilon)
    scaling, warping, flow_layer = models.DepthScalingLayer(epsilon=eps), models.DepthWarpingLayer(epsilon=eps), models.FlowfromDepthLayer()
    with torch.no_grad(), torch.cuda.device(b.device):
        colors_1 = mask_mul(batch["colors_1"], b)          # evaluate.py:189-192
        colors_2 = mask_mul(batch["colors_2"], b)
        sparse_flows_1 = mask_mul(batch["sparse_flows_1"], b)
        sparse_flows_2 = mask_mul(batch["sparse_flows_2"], b)
        if hasattr(model, "forward_pair"):
            pred_1, pred_2 = model.forward_pair(colors_1, colors_2)
        else:
            pred_1, pred_2 = model(colors_1), model(colors_2)
        scaled_1, _ = scaling([pred_1, batch["sparse_depths_1"], batch["sparse_depth_masks_1"]])
        scaled_2, _ = scaling([pred_2, batch["sparse_depths_2"], batch["sparse_depth_masks_2"]])
        t12, r12, t21, r21, k = (batch[name] for name in ("translations_1_wrt_2", "rotations_1_wrt_2", "translations_2_wrt_1",
                                                          "rotations_2_wrt_1", "intrinsics"))
        flows_1 = mask_mul(flow_layer([scaled_1, b, t12, r12, k]), b)
        flows_2 = mask_mul(flow_layer([scaled_2, b, t21, r21, k]), b)
        warped_21, inter_1 = warping([scaled_1, scaled_2, b, t12, r12, k])
        warped_12, inter_2 = warping([scaled_2, scaled_1, b, t21, r21, k])
        out = display.validation_panels(colors_1, colors_2, b, scaled_1, scaled_2, batch["sparse_depths_1"], batch["sparse_depths_2"],
                                        batch["sparse_depth_masks_1"], batch["sparse_depth_masks_2"], warped_21, warped_12, sparse_flows_1,
                                        sparse_flows_2, flows_1, flows_2, k, epsilon=eps, point_cloud_downsampling=point_cloud_downsampling)
        out["offsets"] = out["offsets"].cpu().tolist()          # the batch's one read back (it waits for the stream)
    out.update({"colors_1": colors_1, "colors_2": colors_2, "sparse_flows_1": sparse_flows_1, "sparse_flows_2": sparse_flows_2,
                "predictions_1": pred_1, "predictions_2": pred_2, "scaled_depths_1": scaled_1, "scaled_depths_2": scaled_2,
                "flows_1": flows_1, "flows_2": flows_2, "warped_depths_2_to_1": warped_21, "warped_depths_1_to_2": warped_12,
                "intersect_masks_1": inter_1, "intersect_masks_2": inter_2})
    return out


def _write_validation_batch(ready, index, panel, points, offsets, samples, out_dir, ply_text):
    """One batch's files, on a writer thread, once the device-to-host copies have landed."""
    ready.synchronize()
    if points is not None:
        for i in samples:
            name = "{}.ply".format(index) if i == 0 else "{}_{}.ply".format(index, i)
            utils.write_point_cloud(os.path.join(out_dir, name), points[offsets[i]:offsets[i + 1]].numpy(), text=ply_text)
    if panel is not None:
        utils.write_png(os.path.join(out_dir, "{}.png".format(index)), panel.numpy()[:, :, ::-1])          # write_png takes B, G, R


def run_validation_phase(model, batches, out_dir, write_png=True, write_ply=True, ply_text=True, all_samples=False, writer=None, step=0,
                         writers=4):
    """evaluate.py:167-274: every batch of ``batches`` (a dataset.TrainingBatches(transform=None, shuffle=False)) through
    validation_outputs, then ``<batch>.png`` (the 12-section R, G, B panel) and ``<batch>.ply`` (the point cloud of sample 0's frame 1,
    as the reference writes it; all_samples=True adds ``<batch>_<i>.ply`` for the samples i >= 1) in ``out_dir``, on run_test_phase's
    writer pool.  writer: any object with tensorboardX's add_image; it receives stack_and_display's call (utils.py:894-896) per batch.
    The per-pair measures stay on the device and are read once at the end.  Returns a dictionary: pairs (the number of frame pairs),
    metrics (the (pairs, 2, 4) float32 array of [abs rel, sigma 1, 2, 3] per pair and frame), mean_metrics ((2, 4) float64: per frame
    the means over the pairs whose four numbers are finite; NaN where there is none) and non_finite (the number of (pair, frame) rows
    left out of them: pairs without sparse points in that frame)."""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    collected = []
    with _WriterPool(writers) as pool:
        for index, batch in enumerate(batches):
            out = validation_outputs(model, batch, is_hsv=getattr(batches, "is_hsv", False))
            collected.append(out["metrics"])
            if writer is not None:
                display.stack_and_display("validation", VALIDATION_TITLE, step, writer, out["panel"])
            if not (write_png or write_ply):
                continue
            offsets = out["offsets"]
            samples = range(len(offsets) - 1) if all_samples else range(1)
            panel = out["panel"].to("cpu", non_blocking=True) if write_png else None
            points = out["points"][:offsets[samples[-1] + 1]].to("cpu", non_blocking=True) if write_ply else None
            pool.submit(_write_validation_batch, index, panel, points, offsets, samples, out_dir, ply_text)
    if collected:
        metrics = torch.cat(collected, dim=0).cpu().numpy()          # the pass's one read of the measures
    else:
        metrics = np.zeros((0, 2, 4), np.float32)
    finite = np.all(np.isfinite(metrics), axis=2)
    means = np.full((2, 4), np.nan, np.float64)
    for side in range(2):
        if finite[:, side].any():
            means[side] = metrics[finite[:, side], side].astype(np.float64).mean(axis=0)
    return {"pairs": int(metrics.shape[0]), "metrics": metrics, "mean_metrics": means, "non_finite": int((~finite).sum())}


def _initial_transform(initial):
    """(scale, rotation, translation) of a start given as None (the identity), a registration.Registration, a 4 x 4 matrix whose upper
    left block is scale * R, or a (scale, rotation, translation) tuple."""
    if initial is None:
        return 1.0, np.eye(3), np.zeros(3)
    if isinstance(initial, registration.Registration):
        return initial.scale, initial.rotation, initial.translation
    if isinstance(initial, (tuple, list)) and len(initial) == 3:
        return float(initial[0]), np.asarray(initial[1], np.float64).reshape(3, 3), np.asarray(initial[2], np.float64).reshape(3)
    matrix = np.asarray(initial, np.float64)
    if matrix.shape != (4, 4):
        raise ValueError("initial is None, a Registration, a 4 x 4 matrix or (scale, rotation, translation)")
    det = float(np.linalg.det(matrix[:3, :3]))
    if not det > 0.0:
        raise ValueError("initial's 3 x 3 block must be scale * rotation with a positive determinant")
    scale = det ** (1.0 / 3.0)
    return scale, matrix[:3, :3] / scale, matrix[:3, 3].copy()


def registration_errors(points, offsets, target, initial=None, merged=False, **register_kwargs):
    """The residual errors of point clouds against a model (the reference's README, step 4): ``points`` / ``offsets`` as test_outputs,
    posed_test_outputs and validation_outputs return them (rows of x, y, z, r, g, b on the device; the host list of row offsets), target
    a registration.TargetModel (or rows to make one of, prepared once here), initial the start of every frame (_initial_transform;
    None: the identity), register_kwargs those of registration.register.  Returns a list with one registration.Registration per frame,
    None for a frame without points; merged=True: one Registration of all rows together.  A frame whose matches do not determine a
    similarity raises registration.register's ValueError."""
    if not isinstance(target, registration.TargetModel):
        target = registration.TargetModel(target)
    scale, rotation, translation = _initial_transform(initial)
    offsets = [int(v) for v in offsets]
    if merged:
        if offsets[-1] == offsets[0]:
            return None
        return registration.register(points[offsets[0]:offsets[-1]], target, scale, rotation, translation, **register_kwargs)
    return [registration.register(points[a:b], target, scale, rotation, translation, **register_kwargs) if b > a else None
            for a, b in zip(offsets[:-1], offsets[1:])]


REGISTRATION_COLUMNS = ("name", "points", "inliers", "scale", "mean", "rms", "max", "iterations", "converged")


def _write_registered(ready, path, rows, ply_text):
    ready.synchronize()
    utils.write_point_cloud(path, rows.numpy(), text=ply_text)


def run_registration_phase(model, frames, translation_dict, rotation_dict, target, out_dir, initial=None, write_ply=True, ply_text=True,
                           point_cloud_downsampling=1, min_threshold=None, max_threshold=None, writers=4, **register_kwargs):
    """The posed test outputs of a sequence (posed_test_outputs per batch, as run_posed_test_phase runs them: clouds in the tracker's
    frame), then every frame's cloud registered to ``target`` (a registration.TargetModel, e.g. TargetModel.from_ply of the CT model)
    from ``initial`` (the tracker-to-model start, _initial_transform) with registration.register(**register_kwargs).  Writes
    ``registration_errors.csv`` in ``out_dir``: one line per frame of name, points, inliers (the rows within the last distance cap),
    scale, mean, rms and max of their distances, iterations, converged; a frame without kept pixels, with non-finite coordinates (equal
    kept depths) or whose matches do not determine a similarity has points and empty fields.  write_ply: ``registered_<name>.ply``, the
    frame's cloud under its registration (endo_similarity_apply; colours kept), on run_test_phase's writer pool.
    Returns a dictionary: frames, registered (their number), failed (the names of the other frames), rows (the table's rows) and rms
    (the root mean square of the inliers' distances over all registered frames; NaN without one)."""
    names_ahead = getattr(frames, "image_file_names", None)
    if names_ahead is not None:
        for name in names_ahead:
            key = os.path.basename(str(name))[-12:-4]
            translation_dict[key], rotation_dict[key]          # KeyError before anything runs
    if not isinstance(target, registration.TargetModel):
        target = registration.TargetModel(target)
    scale, rotation, translation = _initial_transform(initial)
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    rows, failed = [], []
    count, squares, inliers = 0, 0.0, 0
    with _WriterPool(writers) as pool:
        for batch in frames:
            names = list(batch["names"])
            out = posed_test_outputs(model, batch, [rotation_dict[name] for name in names], [translation_dict[name] for name in names],
                                     is_hsv=getattr(frames, "is_hsv", False), point_cloud_downsampling=point_cloud_downsampling,
                                     min_threshold=min_threshold, max_threshold=max_threshold)
            count += len(names)
            offsets, ranges = out["offsets"], out["ranges"]
            for f, name in enumerate(names):
                cloud = out["points"][offsets[f]:offsets[f + 1]]
                result = None
                if ranges[f, 0] < ranges[f, 1]:          # neither empty nor of equal kept depths (non-finite coordinates)
                    try:
                        result = registration.register(cloud, target, scale, rotation, translation, **register_kwargs)
                    except ValueError:
                        result = None
                if result is None:
                    failed.append(name)
                    rows.append((name, int(cloud.shape[0]), "", "", "", "", "", "", ""))
                    continue
                rows.append((name, int(cloud.shape[0]), result.count, repr(result.scale), repr(result.mean), repr(result.rms),
                             repr(result.max), result.iterations, int(result.converged)))
                squares += result.rms * result.rms * result.count
                inliers += result.count
                if write_ply:
                    moved = registration.similarity_apply(cloud, result.scale, result.rotation, result.translation)
                    pool.submit(_write_registered, os.path.join(out_dir, "registered_{}.ply".format(name)),
                                moved.to("cpu", non_blocking=True), ply_text)
    with open(os.path.join(out_dir, "registration_errors.csv"), "w") as f:
        f.write(",".join(REGISTRATION_COLUMNS) + "\n")
        for row in rows:
            f.write(",".join(str(v) for v in row) + "\n")
    return {"frames": count, "registered": count - len(failed), "failed": failed, "rows": rows,
            "rms": float(np.sqrt(squares / inliers)) if inliers else float("nan")}


def _write_fused(ready, path, rows, ply_text):
    ready.synchronize()
    utils.write_point_cloud(path, rows.numpy(), text=ply_text)


def _write_fused_mesh(ready, path, vertices, normals, faces, ply_text):
    ready.synchronize()
    utils.write_mesh(path, vertices.numpy(), normals.numpy(), faces.numpy(), text=ply_text)


CONSISTENCY_COLUMNS = ("name", "pixels", "abs_rel", "sigma_1", "sigma_2", "sigma_3")


def _write_fused_color(ready, path, image):
    ready.synchronize()
    utils.write_png(path, image.numpy())


def _write_consistency(ready, path, names, metrics, pixels, rows):
    ready.synchronize()
    for name, m, p in zip(names, torch.cat(metrics).numpy().astype(np.float64), torch.cat(pixels).numpy()):
        rows.append((name, int(p), float(m[0]), float(m[1]), float(m[2]), float(m[3])))
    with open(path, "w") as f:
        f.write(",".join(CONSISTENCY_COLUMNS) + "\n")
        for row in rows:
            f.write(",".join([row[0], str(row[1])] + [repr(v) for v in row[2:]]) + "\n")


TRACKING_COLUMNS = ("name", "status", "iterations", "count", "rms_before", "rms_after", "rotation_degrees", "translation", "scale_ratio")


def _write_tracking(path, rows):
    with open(path, "w") as f:
        f.write(",".join(TRACKING_COLUMNS) + "\n")
        for row in rows:
            f.write(",".join([row[0], row[1], str(row[2]), str(row[3])] + [repr(v) for v in row[4:]]) + "\n")


def _refine_poses(volume, kept, poses, names, rounds, min_weight):
    """run_fusion_phase's refine: ``rounds`` times, every kept batch tracked against the volume (fusion.TSDFVolume.track), the volume
    cleared and the batches integrated again under the poses and scales found.  ``poses``: per batch (rotations, translations,
    scales) as host fp64 arrays, updated in place.  A frame whose tracking does not end "ok" keeps the pose and scale it entered the
    round with: the tracker's own in the first.  Returns the rows of TRACKING_COLUMNS, one per frame: status, count and rms after of the
    last round, the iterations of all rounds, rms before of the first, and the change from the tracker's pose and the frame's own scale."""
    first = [tuple(a.copy() for a in pose) for pose in poses]
    state = [[{"iterations": 0, "before": None} for _ in batch_names] for batch_names in names]
    fits = []
    for _ in range(rounds):
        fits = [volume.track(depth, boundaries, intrinsics, pose[0], pose[1], scales=pose[2], min_weight=min_weight)
                for (depth, boundaries, _, intrinsics, _, _), pose in zip(kept, poses)]          # every batch against the same model
        for pose, batch_fits, batch_state in zip(poses, fits, state):
            for f, (fit, frame) in enumerate(zip(batch_fits, batch_state)):
                frame["iterations"] += fit.iterations
                if frame["before"] is None:
                    frame["before"] = fit.initial_rms
                if fit.status == "ok":
                    pose[0][f], pose[1][f], pose[2][f] = fit.rotation, fit.translation, fit.scale
        volume.clear()
        for (depth, boundaries, colors, intrinsics, _, _), pose in zip(kept, poses):
            volume.integrate(depth, boundaries, colors, intrinsics, pose[0], pose[1], scales=pose[2].astype(np.float32))
    rows = []
    for pose, start, batch_fits, batch_state, batch_names in zip(poses, first, fits, state, names):
        for f, (fit, frame, name) in enumerate(zip(batch_fits, batch_state, batch_names)):
            cosine = (float(np.trace(pose[0][f] @ start[0][f].T)) - 1.0) / 2.0
            rows.append((name, fit.status, frame["iterations"], fit.count, float(frame["before"]), float(fit.rms),
                         float(np.degrees(np.arccos(min(1.0, max(-1.0, cosine))))), float(np.linalg.norm(pose[1][f] - start[1][f])),
                         float(pose[2][f] / start[2][f])))
    return rows


def run_fusion_phase(model, frames, translation_dict, rotation_dict, out_dir, voxel_size=None, resolution=256, truncation_voxels=4,
                     min_weight=2.0, max_weight=64.0, target=None, initial=None, ply_text=False, mesh=False, render=False, refine=0,
                     **register_kwargs):
    """One model of a sequence: every batch of ``frames`` (a dataset.TestFrames) through posed_test_outputs with the poses
    ``translation_dict[name]`` / ``rotation_dict[name]`` (the network's forward runs once); each batch's depth, colour images,
    boundaries, intrinsics and poses stay on the device, with the bounding box of its posed rows.  Then a fusion.TSDFVolume around
    that box (its longest side in ``resolution`` voxels, or voxels of ``voxel_size``; truncation ``truncation_voxels`` voxels), the
    batches integrated in order, the surface extracted at ``min_weight`` and written as ``fused_surface.ply`` in ``out_dir`` on
    run_test_phase's writer pool.  Frames without kept pixels or with equal kept depths take no part, neither in the box nor in the
    volume; their names are reported.  A frame whose name is missing from either dictionary raises KeyError before anything runs.
    With ``target`` (a registration.TargetModel, or rows to make one of): the fused rows registered once with
    registration.register(**register_kwargs) from ``initial`` (_initial_transform), ``fused_registered.ply`` (the rows under that
    registration, colours kept) and a one-row ``fused_registration.csv`` with REGISTRATION_COLUMNS.
    mesh=True: the surface comes from volume.extract_mesh -- the same rows, with normals and faces -- and ``fused_mesh.ply``
    (utils.write_mesh) is written on the same pool; every other file is what it is without it.
    render=True: after the last batch is integrated, every frame that took part is rendered from its own pose (volume.render with the
    frame's own scale 20 / (z_max - z_min), its boundaries and ``min_weight``): ``fused_color_<name>.png``, the model's colours as that
    frame sees them, comparable with run_posed_test_phase's test_color_<name>.png, and ``fused_consistency.csv``, one row per such
    frame of CONSISTENCY_COLUMNS: the hit pixels and losses.depth_metrics(the frame's predicted depth, the rendered depth, the hit
    mask), the frame's AbsRel and sigma 1, 2, 3 against what the whole sequence agrees the surface is (NaN without a hit pixel); both on
    the same pool.  Every other file is what it is without it.
    refine=K > 0: after the sequence is integrated, K times: every frame that took part is tracked against the volume
    (fusion.TSDFVolume.track(min_weight=min_weight), a similarity per frame, each frame starting from the tracker's pose
    and its own scale 20 / (z_max - z_min)), the volume is cleared and the batches are integrated again under the refined poses and
    explicit scales; a frame whose tracking does not end "ok" keeps the pose it had.  The surface, the mesh, the renders and the
    registration then come from the final volume and the final poses.  ``fused_tracking.csv`` has one row per such frame of
    TRACKING_COLUMNS: status, iterations, count, the rms of the signed distances before and after, and how far the pose moved:
    the rotation in degrees, the translation, the ratio of the scales.  A known bias: a frame is tracked against a model that
    contains the frame itself, with 1 / weight of every voxel it saw, which pulls it towards where it already is; tracking a frame
    before it is integrated, or taking it out first, is not done here.  With refine=0 every file and the dictionary are what they are
    without it.
    Returns a dictionary: frames (their number), empty and zero_range (names), voxel_size, dims and origin of the volume (None when no
    frame took part), points (the surface's rows), observed_voxels, registration (a registration.Registration, or None), with mesh=True triangles
    (the mesh's faces), with render=True consistency (the table's rows), and with refine > 0 tracking (fused_tracking.csv's rows) and poses (name -> the final rotation, translation and scale)."""
    names_ahead = getattr(frames, "image_file_names", None)
    if names_ahead is not None:
        for name in names_ahead:
            key = os.path.basename(str(name))[-12:-4]
            translation_dict[key], rotation_dict[key]          # KeyError before anything runs
    out_dir = str(out_dir)
    refine = int(refine)
    if refine < 0:
        raise ValueError("refine must not be negative, not %d" % refine)
    count = 0
    empty, zero_range, kept, boxes, views, consistency, tracking = [], [], [], [], [], [], []
    for batch in frames:
        names = list(batch["names"])
        rotations = [rotation_dict[name] for name in names]
        translations = [translation_dict[name] for name in names]
        out = posed_test_outputs(model, batch, rotations, translations, is_hsv=getattr(frames, "is_hsv", False))
        count += len(names)
        offsets, ranges = out["offsets"], out["ranges"]
        good = []
        for f, name in enumerate(names):
            if ranges[f, 0] > ranges[f, 1]:
                empty.append(name)
            elif ranges[f, 0] == ranges[f, 1]:
                zero_range.append(name)
            else:
                good.append(f)
        for f in good:
            rows = out["points"][offsets[f]:offsets[f + 1], :3]
            if rows.shape[0]:
                boxes.append(torch.stack([rows.amin(dim=0), rows.amax(dim=0)]))
        if good:
            dev = out["depth"].device
            rot, tr = _poses_f64(rotations, translations, len(names), dev)
            pick = torch.tensor(good, dtype=torch.int64, device=dev)
            kept.append((out["depth"][pick], batch["boundaries"].to(dev)[pick], out["color_images"][pick], batch["intrinsics"].to(dev)[pick],
                         rot[pick], tr[pick]))
            if render or refine:          # the posed output's own scale of each frame: evaluate_posed.hip:150-151
                views.append(([names[f] for f in good], np.float32(20.0) / (ranges[good, 1] - ranges[good, 0])))
    os.makedirs(out_dir, exist_ok=True)
    result = {"frames": count, "empty": empty, "zero_range": zero_range, "voxel_size": None, "dims": None, "origin": None, "points": 0,
              "observed_voxels": 0, "registration": None}
    with _WriterPool(1) as pool:
        if boxes:
            both = torch.stack(boxes).to(torch.float64)
            bounds = torch.stack([both[:, 0].amin(dim=0), both[:, 1].amax(dim=0)]).cpu().numpy()          # the box's one read
            volume = fusion.TSDFVolume.around_bounds(bounds[0], bounds[1], voxel_size, resolution, device=kept[0][0].device,
                                                     truncation_voxels=truncation_voxels, max_weight=max_weight)
            for depth, boundaries, colors, intrinsics, rot, tr in kept:
                volume.integrate(depth, boundaries, colors, intrinsics, rot, tr)
            if refine:
                poses = [(rot.cpu().numpy(), tr.cpu().numpy(), scales.astype(np.float64)) for (_, _, _, _, rot, tr), (_, scales) in zip(kept, views)]
                tracking += _refine_poses(volume, kept, poses, [names for names, _ in views], refine, min_weight)
                result["poses"] = {name: (pose[0][f].copy(), pose[1][f].copy(), float(pose[2][f]))
                                   for (names, _), pose in zip(views, poses) for f, name in enumerate(names)}
                kept = [batch[:4] + (rot, tr) for batch, (rot, tr, _) in zip(kept, poses)]
                views = [(names, scales.astype(np.float32)) for (names, _), (_, _, scales) in zip(views, poses)]
            if mesh:
                surface, normals, faces = volume.extract_mesh(min_weight)
            else:
                surface = volume.extract(min_weight)
            result.update({"voxel_size": volume.voxel_size, "dims": volume.dims, "origin": volume.origin.copy(),
                           "observed_voxels": volume.observed_voxels()})
            if render:
                shown, metrics, pixels = [], [], []
                for (depth, boundaries, _, intrinsics, rot, tr), (names, scales) in zip(kept, views):
                    height, width = int(depth.shape[-2]), int(depth.shape[-1])
                    seen = volume.render(intrinsics, rot, tr, height, width, scales=scales, boundaries=boundaries, min_weight=min_weight)
                    metrics.append(losses.depth_metrics(depth.reshape(-1, 1, height, width), seen["depth"], seen["mask"]).to("cpu", non_blocking=True))
                    pixels.append(seen["mask"].sum(dim=(1, 2, 3)).to("cpu", non_blocking=True))
                    images = seen["colors"].to("cpu", non_blocking=True)
                    shown += names
                    for f, name in enumerate(names):
                        pool.submit(_write_fused_color, os.path.join(out_dir, "fused_color_{}.png".format(name)), images[f])
                pool.submit(_write_consistency, os.path.join(out_dir, "fused_consistency.csv"), shown, metrics, pixels, consistency)
        else:
            surface = torch.zeros((0, 6), dtype=torch.float32)
            normals, faces = torch.zeros((0, 3), dtype=torch.float32), torch.zeros((0, 3), dtype=torch.int32)
        result["points"] = int(surface.shape[0])
        pool.submit(_write_fused, os.path.join(out_dir, "fused_surface.ply"), surface.to("cpu", non_blocking=True), ply_text)
        if mesh:
            result["triangles"] = int(faces.shape[0])
            pool.submit(_write_fused_mesh, os.path.join(out_dir, "fused_mesh.ply"), surface.to("cpu", non_blocking=True),
                        normals.to("cpu", non_blocking=True), faces.to("cpu", non_blocking=True), ply_text)
        if target is not None:
            if not isinstance(target, registration.TargetModel):
                target = registration.TargetModel(target)
            scale, rotation, translation = _initial_transform(initial)
            fit = registration.register(surface, target, scale, rotation, translation, **register_kwargs)
            moved = registration.similarity_apply(surface, fit.scale, fit.rotation, fit.translation)
            pool.submit(_write_fused, os.path.join(out_dir, "fused_registered.ply"), moved.to("cpu", non_blocking=True), ply_text)
            with open(os.path.join(out_dir, "fused_registration.csv"), "w") as f:
                f.write(",".join(REGISTRATION_COLUMNS) + "\n")
                f.write(",".join(str(v) for v in ("fused", int(surface.shape[0]), fit.count, repr(fit.scale), repr(fit.mean), repr(fit.rms),
                                                  repr(fit.max), fit.iterations, int(fit.converged))) + "\n")
            result["registration"] = fit
    if refine:
        result["tracking"] = tracking
        result.setdefault("poses", {})
        _write_tracking(os.path.join(out_dir, "fused_tracking.csv"), tracking)
    if render:
        result["consistency"] = consistency
        if not boxes:          # no frame took part: the table has its header alone
            _write_consistency(torch.cuda.Event(), os.path.join(out_dir, "fused_consistency.csv"), [], [torch.zeros((0, 4))], [torch.zeros(0)], consistency)
    return result


MODEL_DEPTH_COLUMNS = ("name", "pixels", "scale", "abs_rel", "sigma_1", "sigma_2", "sigma_3")


def _model_poses(rotations, translations, transforms, n):
    """Each frame's camera in the model's frame: with the tracker-to-model similarity (sigma, Q, tau) of the frame, the rotation Q R_f
    and the centre sigma Q t_f + tau, host fp64.  transforms: one start (_initial_transform) for all frames or a list of N."""
    rot, tr = _poses_f64(rotations, translations, n, torch.device("cpu"))
    rot, tr = rot.numpy(), tr.numpy()
    if not (isinstance(transforms, list) and len(transforms) == n and not np.isscalar(transforms[0])):          # ([scale, R, t] is one)
        transforms = [transforms] * n
    out_rot, out_tr = np.empty((n, 3, 3)), np.empty((n, 3))
    for f, transform in enumerate(transforms):
        sigma, q, tau = _initial_transform(transform)
        out_rot[f] = np.asarray(q, np.float64) @ rot[f]
        out_tr[f] = float(sigma) * (np.asarray(q, np.float64) @ tr[f]) + np.asarray(tau, np.float64)
    return out_rot, out_tr


def model_depth_errors(predictions, boundaries, intrinsics, rotations, translations, mesh, transform=None, cull=None):
    """Predicted depth against the depth of a model's surface, per frame.  predictions and boundaries (N, 1, H, W) and intrinsics
    (N, 3, 3), fp32 on the device; rotations (N, 3, 3) and translations (N, 3): each frame's pose in the tracker's frame
    (reader.read_initial_pose_file); mesh: a mesh.TriangleMesh in the model's frame; transform: the tracker-to-model similarity
    (_initial_transform: None, a registration.Registration, a 4 x 4 matrix or (scale, rotation, translation)), or a list of N of
    them, one per frame.  The camera of frame f stands in the model's frame with rotation Q R_f at sigma Q t_f + tau -- no scale of the
    prediction enters, which is why the scale can be taken from the render afterwards.  The mesh is rendered from there at scale 1
    (mesh.render with the frame's boundaries and ``cull``), so its depth is in the model's units; each prediction is scaled to it over
    the rendered mask as the reference scales to sparse depth (models.DepthScalingLayer), and losses.depth_metrics compares the two.
    Returns the render's dictionary (depth, mask, normals, colors, triangle, barycentric, flags) plus ``scaled`` (N, 1, H, W), the
    scaled predictions, ``metrics`` (N, 4) fp32 [abs rel, sigma 1, 2, 3] (NaN for a frame the model does not cover), ``pixels`` (N,)
    fp32, the covered pixels, and ``scale`` (N,) fp64, the factor each prediction was multiplied by (NaN likewise): device tensors."""
    if not isinstance(mesh, mesh_module.TriangleMesh):
        raise ValueError("mesh must be a mesh.TriangleMesh")
    if not torch.is_tensor(predictions) or predictions.dim() != 4 or predictions.shape[1] != 1:
        raise ValueError("predictions must be an (N, 1, H, W) device tensor")
    n, _, height, width = (int(v) for v in predictions.shape)
    predictions = _device_f32(predictions, (n, 1, height, width), "predictions")
    boundaries = _device_f32(boundaries, (n, 1, height, width), "boundaries")
    intrinsics = _device_f32(intrinsics, (n, 3, 3), "intrinsics")
    model_rot, model_tr = _model_poses(rotations, translations, transform, n)
    with torch.no_grad(), torch.cuda.device(predictions.device):
        seen = mesh.render(intrinsics, model_rot, model_tr, height, width, boundaries=boundaries, cull=cull)
        scaled, _ = models.DepthScalingLayer()([predictions, seen["depth"], seen["mask"]])
        metrics = losses.depth_metrics(scaled, seen["depth"], seen["mask"])
        mask = seen["mask"].to(torch.float64)
        scale = (scaled.to(torch.float64) * mask).sum(dim=(1, 2, 3)) / (predictions.to(torch.float64) * mask).sum(dim=(1, 2, 3))
        pixels = seen["mask"].sum(dim=(1, 2, 3))
    out = dict(seen)
    out.update({"scaled": scaled, "metrics": metrics, "pixels": pixels, "scale": scale})
    return out


def _cloud_start(start, translation, model_scale, z_range):
    """Where ICP starts for one frame's posed cloud.  The cloud is ``R (s d ray) + t`` with the posed output's own
    s = 20 / (z_max - z_min), not the tracker's metric: it is the frame's surface scaled about the camera centre t by an unknown lambda.
    The render from ``start`` = (sigma, Q, tau) tells lambda: ``model_scale`` times the prediction is the model's depth there, so
    lambda = s sigma / model_scale, and the start is x -> sigma Q ((x - t) / lambda + t) + tau: scale model_scale / s, rotation Q,
    translation tau + (sigma - model_scale / s) Q t."""
    sigma, q, tau = start
    own = 20.0 / (float(z_range[1]) - float(z_range[0]))
    scale = float(model_scale) / own
    return scale, q, np.asarray(tau, np.float64) + (float(sigma) - scale) * (np.asarray(q, np.float64) @ np.asarray(translation, np.float64).reshape(3))


def _write_model_depth_images(ready, names, left, right, out_dir):
    ready.synchronize()
    for f, name in enumerate(names):
        utils.write_png(os.path.join(out_dir, "model_depth_{}.png".format(name)), np.concatenate([left[f].numpy(), right[f].numpy()], axis=1))


def _depth_images(depth, boundaries):
    """utils.display_depth_map's colours for a batch of (N, 1, H, W) maps: endo_evaluate_posed's depth images, (N, H, W, 3) B, G, R."""
    n, _, height, width = (int(v) for v in depth.shape)
    dev = depth.device
    zeros = torch.zeros((n, 3, height, width), dtype=torch.float32, device=dev)
    k = torch.eye(3, dtype=torch.float32, device=dev).reshape(1, 3, 3).repeat(n, 1, 1)
    return posed_outputs_from_predictions(zeros, boundaries, depth, k, np.stack([np.eye(3)] * n), np.zeros((n, 3)))["depth_images"]


def run_model_depth_phase(model, frames, translation_dict, rotation_dict, mesh, out_dir, initial=None, refine=False, write_images=True,
                          writers=4, **register_kwargs):
    """Dense depth errors of a sequence against a model: every batch of ``frames`` (a dataset.TestFrames) through the network in eval
    mode on ``boundaries * colors``, as run_registration_phase runs it, then model_depth_errors with the poses
    ``translation_dict[name]`` / ``rotation_dict[name]`` and ``initial``, the tracker-to-model similarity (_initial_transform).
    refine=True: each frame's posed cloud (posed_outputs_from_predictions) is first registered to ``mesh.target()`` with
    registration.register(**register_kwargs) and the frame uses its own similarity.  The cloud has the posed output's own scale about
    its camera centre, so its start is ``initial`` with that scale taken out by a first render from ``initial`` (_cloud_start).  A
    frame that fails -- no kept pixels, equal kept depths, no pixel the model covers from ``initial`` or matches that do not
    determine a similarity -- falls back to ``initial`` and is named in ``failed``.
    Writes ``model_depth_errors.csv`` in ``out_dir``: one line per frame of MODEL_DEPTH_COLUMNS -- the pixels the model covers, the
    factor the prediction was scaled by, AbsRel and sigma 1, 2, 3 of the scaled prediction against the model's depth there (NaN
    without such a pixel); and with write_images ``model_depth_<name>.png``: prediction | rendered depth, each in
    utils.display_depth_map's colours over its own range, on run_test_phase's writer pool.  A frame whose name is missing from either
    dictionary raises KeyError before anything runs.
    Returns a dictionary: frames (their number), failed (names; empty without refine), rows (the table's rows), covered (the frames
    with at least one covered pixel) and mean_metrics ((4,) float64 over those frames; NaN without one)."""
    names_ahead = getattr(frames, "image_file_names", None)
    if names_ahead is not None:
        for name in names_ahead:
            key = os.path.basename(str(name))[-12:-4]
            translation_dict[key], rotation_dict[key]          # KeyError before anything runs
    if not isinstance(mesh, mesh_module.TriangleMesh):
        raise ValueError("mesh must be a mesh.TriangleMesh")
    start = _initial_transform(initial)
    target = mesh.target() if refine else None
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    count, failed, all_names, collected = 0, [], [], []
    with _WriterPool(writers) as pool:
        for batch in frames:
            names = list(batch["names"])
            rotations = [rotation_dict[name] for name in names]
            translations = [translation_dict[name] for name in names]
            masked, boundaries, pred, intrinsics = _masked_forward(model, batch, "run_model_depth_phase")
            transforms = [start] * len(names)
            if refine:
                posed = posed_outputs_from_predictions(masked, boundaries, pred, intrinsics, rotations, translations,
                                                       is_hsv=getattr(frames, "is_hsv", False))
                offsets, ranges = posed["offsets"], posed["ranges"]
                first = model_depth_errors(pred, boundaries, intrinsics, rotations, translations, mesh, start)["scale"].cpu().numpy()
                for f, name in enumerate(names):
                    fit = None
                    if ranges[f, 0] < ranges[f, 1] and np.isfinite(first[f]) and first[f] > 0.0:
                        try:
                            fit = registration.register(posed["points"][offsets[f]:offsets[f + 1]], target,
                                                        *_cloud_start(start, translations[f], first[f], ranges[f]), **register_kwargs)
                        except ValueError:
                            fit = None
                    if fit is None:
                        failed.append(name)
                    else:
                        transforms[f] = (fit.scale, fit.rotation, fit.translation)
            out = model_depth_errors(pred, boundaries, intrinsics, rotations, translations, mesh, transforms)
            count += len(names)
            all_names += names
            collected.append(torch.cat([out["pixels"].to(torch.float64)[:, None], out["scale"][:, None], out["metrics"].to(torch.float64)], dim=1))
            if write_images:
                left = _depth_images(pred, boundaries).to("cpu", non_blocking=True)
                right = _depth_images(out["depth"], boundaries).to("cpu", non_blocking=True)
                pool.submit(_write_model_depth_images, names, left, right, out_dir)
    table = torch.cat(collected, dim=0).cpu().numpy() if collected else np.zeros((0, 6))          # the phase's one read of the measures
    rows = [(name, int(row[0])) + tuple(float(v) for v in row[1:]) for name, row in zip(all_names, table)]
    with open(os.path.join(out_dir, "model_depth_errors.csv"), "w") as f:
        f.write(",".join(MODEL_DEPTH_COLUMNS) + "\n")
        for row in rows:
            f.write(",".join([row[0], str(row[1])] + [repr(v) for v in row[2:]]) + "\n")
    covered = table[:, 0] > 0
    return {"frames": count, "failed": failed, "rows": rows, "covered": int(covered.sum()),
            "mean_metrics": table[covered, 2:].mean(axis=0) if covered.any() else np.full(4, np.nan)}
