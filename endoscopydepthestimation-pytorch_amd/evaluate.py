"""The test phase of the reference's evaluate.py (279-346): per frame one masked depth map, one colour|depth PNG panel and one
coloured PLY point cloud, for batches of frames (dataset.TestFrames) on the device.

    per batch   boundaries * colors -> the network in eval mode -> endo_evaluate (csrc/evaluate.hip: three launches whatever the batch
                size): masked depth, the (N, H, 2W, 3) BGR panels, the point clouds of all frames and their offsets; one host read
    per frame   utils.write_png / utils.write_point_cloud on a small writer pool, while the next batch is decoded and run

The reference needs cv2 and plyfile here and runs one frame per batch with all per-pixel work on the host (evaluate.py:292, 329-345).
"""

import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import torch

from . import _lib, utils


def _device_f32(t, shape, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a float32 device tensor of shape %s" % (name, tuple(shape)))
    return t.contiguous()


def test_outputs(model, batch, is_hsv=False, point_cloud_downsampling=1):
    """evaluate.py:323-344 for a TestFrames batch: the network on ``boundaries * colors`` and the per-frame outputs, on the device.
    Returns a dictionary: colors (the masked network input), predictions, depth (N, 1, H, W) fp32, panels (N, H, 2W, 3) uint8 B, G, R
    (what evaluate.py:345 hands to cv2.imwrite), points (capacity N * H * W rows of x, y, z, r, g, b) and offsets: the host list of N + 1
    row offsets, frame f's points being points[offsets[f]:offsets[f + 1]] -- the batch's one read back to the host."""
    if model.training:
        raise RuntimeError("test_outputs runs the network in eval mode: call model.eval() first (evaluate.py:313)")
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
    out = outputs_from_predictions(masked, boundaries, pred, intrinsics, is_hsv, point_cloud_downsampling)
    out["colors"], out["predictions"] = masked, pred
    return out


def outputs_from_predictions(colors, boundaries, predictions, intrinsics, is_hsv=False, point_cloud_downsampling=1):
    """endo_evaluate on a batch: colors (N, 3, H, W) the masked network input, boundaries (N, 1, H, W) in {0, 1}, predictions
    (N, 1, H, W) the network's output, intrinsics (N, 3, 3), all fp32 on the device.  Returns depth, panels, points and the host list
    of offsets as test_outputs does."""
    n, _, height, width = (int(v) for v in colors.shape)
    colors = _device_f32(colors, (n, 3, height, width), "colors")
    boundaries = _device_f32(boundaries, (n, 1, height, width), "boundaries")
    predictions = _device_f32(predictions, (n, 1, height, width), "predictions")
    intrinsics = _device_f32(intrinsics, (n, 3, 3), "intrinsics")
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
    pending = deque()
    with ThreadPoolExecutor(max(1, int(writers))) as pool:
        try:
            for batch in frames:
                out = test_outputs(model, batch, is_hsv=frames.is_hsv, point_cloud_downsampling=point_cloud_downsampling)
                names = list(batch["names"])
                count += len(names)
                if not (write_png or write_ply):
                    continue
                offsets = out["offsets"]
                panels = out["panels"].to("cpu", non_blocking=True) if write_png else None
                points = out["points"][:offsets[-1]].to("cpu", non_blocking=True) if write_ply else None
                ready = torch.cuda.Event()
                ready.record()
                pending.append(pool.submit(_write_frames, ready, names, panels, points, offsets, out_dir, write_png, write_ply, ply_text))
                while len(pending) > 2 * max(1, int(writers)):          # bound the host copies in flight
                    pending.popleft().result()
        finally:
            while pending:
                pending.popleft().result()
    return count
