"""The display panels of train.py's epoch loop (353-371 during training, 460-478 during validation) on the device.

    panels(...)              endo_display (csrc/display.hip: two launches whatever the batch size): the uint8 (8 Hg, Wg, 3) R, G, B panel
                             of c1, d1, sf1, df1, c2, d2, sf2, df2 stacked top to bottom, each section the make_grid of the batch -- what
                             utils.display_color_depth_sparse_flow_dense_flow (twice), draw_flow and stack_and_display build on the host
                             with torchvision and cv2 (utils.py:868-900, 965-994) and a tensorboardX writer stores
    validation_panels(...)   endo_evaluate_validation (csrc/evaluate_validation.hip: three launches whatever the batch size): the uint8
                             (12 Hg, Wg, 3) panel of c1 sd1 d1 wd1 sf1 df1 c2 sd2 d2 wd2 sf2 df2 that evaluate.py's validation phase
                             builds (utils.py:903-954) and writes, with the batch's error measures and point clouds
    grid_shape(n, h, w)      (Hg, Wg) of one section: make_grid(nrow=8, padding=2) of n frames; n = 1 is the frame itself
    stack_and_display(...)   utils.stack_and_display's writer call for a device panel

TrainingStep.display_panels() renders the latest training or validation call from the fused loss head's workspace; panels() takes
tensors from any path, the module path's ``losses()`` extras included.  The TensorBoard writer stays the caller's: any object with an
``add_image(tag, img_tensor, global_step)`` method.
"""

import math

import torch

from . import _lib


def grid_shape(n, h, w):
    """(Hg, Wg) of torchvision's make_grid(nrow=8, padding=2) over n frames of h x w: min(8, n) frames across, ceil(n / 8) down, two pixels
    of padding around and between them; n = 1 gives (h, w) (make_grid returns the frame itself)."""
    n, h, w = int(n), int(h), int(w)
    if n <= 0 or h <= 0 or w <= 0:
        raise ValueError("grid_shape needs n, h, w >= 1 (got %d, %d, %d)" % (n, h, w))
    if n == 1:
        return h, w
    xmaps = min(8, n)
    ymaps = int(math.ceil(float(n) / xmaps))
    return (h + 2) * ymaps + 2, (w + 2) * xmaps + 2


def panel_shape(n, h, w):
    """(8 Hg, Wg, 3): the eight sections of a panel stacked top to bottom."""
    gh, gw = grid_shape(n, h, w)
    return 8 * gh, gw, 3


def _device_f32(t, shape, name, device):
    if not torch.is_tensor(t) or not t.is_cuda or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a device tensor of shape %s" % (name, tuple(shape)))
    if t.device != device:
        raise ValueError("%s is on %s, the batch on %s" % (name, t.device, device))
    return _lib.dev_f32(t, name)


def panels(colors_1, colors_2, depths_1, depths_2, boundaries, sparse_flows_1, sparse_flows_2, flows_1, flows_2, is_hsv=False):
    """train.py:353-371 for one batch: colors_k (N, 3, H, W) the masked network input (train.py:272-273), depths_k (N, 1, H, W) the scaled
    depth (multiplied by ``boundaries`` (N, 1, H, W) inside, as train.py:356 does), sparse_flows_k / flows_k (N, 2, H, W) the masked sparse
    flows and flows from depth (train.py:295-298).  Returns the device uint8 (8 Hg, Wg, 3) R, G, B panel, on the current stream.
    is_hsv=True (train.py --use_hsv_colorspace) is not implemented: the reference converts its float colour grid with cv2's float HSV
    path."""
    if is_hsv:
        raise NotImplementedError("HSV display panels: the reference converts the float colour grid with cv2.COLOR_HSV2RGB_FULL's float path, "
                                  "which is not implemented")
    if not torch.is_tensor(colors_1) or colors_1.dim() != 4 or colors_1.shape[1] != 3:
        raise ValueError("colors_1 must be an (N, 3, H, W) tensor")
    n, _, h, w = (int(v) for v in colors_1.shape)
    device = colors_1.device
    args = []
    for t, c, name in ((colors_1, 3, "colors_1"), (colors_2, 3, "colors_2"), (depths_1, 1, "depths_1"), (depths_2, 1, "depths_2"),
                       (boundaries, 1, "boundaries"), (sparse_flows_1, 2, "sparse_flows_1"), (sparse_flows_2, 2, "sparse_flows_2"),
                       (flows_1, 2, "flows_1"), (flows_2, 2, "flows_2")):
        args.append(_device_f32(t, (n, c, h, w), name, device))
    lib = _lib.load()
    need = int(lib.endo_display_workspace_bytes(n, h, w))
    if need < 0:
        raise ValueError("a batch of %d pairs of %d x %d is outside endo_display's sizes" % (n, h, w))
    with torch.cuda.device(device):
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        out = torch.empty(panel_shape(n, h, w), dtype=torch.uint8, device=device)
        _lib.check(lib.endo_display(*[_lib.ptr(a) for a in args], n, h, w, _lib.ptr(out), _lib.ptr(workspace), need, _lib.stream()),
                   "endo_display")
    return out


def _on_gpu(t, name):
    """a host tensor is the usual RuntimeError of the boundary contract (no CPU fallback), not a shape error"""
    if torch.is_tensor(t) and not t.is_cuda:
        _lib.dev_f32(t, name)
    return t


def validation_panel_shape(n, h, w):
    """(12 Hg, Wg, 3): the twelve sections of evaluate.py's validation panel stacked top to bottom."""
    gh, gw = grid_shape(n, h, w)
    return 12 * gh, gw, 3


def validation_panels(colors_1, colors_2, boundaries, depths_1, depths_2, sparse_depths_1, sparse_depths_2, sparse_depth_masks_1,
                      sparse_depth_masks_2, warped_depths_2_to_1, warped_depths_1_to_2, sparse_flows_1, sparse_flows_2, flows_1, flows_2,
                      intrinsics, epsilon=1.0e-8, is_hsv=False, point_cloud_downsampling=1):
    """evaluate.py:201-274 for one batch: colors_k (N, 3, H, W) the masked network input, boundaries (N, 1, H, W), depths_k the scaled
    depths (unmasked), sparse_depths_k / sparse_depth_masks_k, warped_depths_2_to_1 / _1_to_2 (N, 1, H, W), sparse_flows_k / flows_k
    (N, 2, H, W) the masked sparse flows and flows from depth, intrinsics (N, 3, 3).  Returns a dictionary of device tensors on the
    current stream: panel uint8 (12 Hg, Wg, 3) R, G, B; metrics (N, 2, 4) float32 [abs rel, sigma 1, 2, 3] per sample and frame;
    points (capacity N H W rows of x, y, z, r, g, b: frame 1 of every pair) and offsets int64 (N + 1).
    is_hsv=True is not implemented, for the reason panels() gives."""
    if is_hsv:
        raise NotImplementedError("HSV display panels: the reference converts the float colour grid with cv2.COLOR_HSV2RGB_FULL's float path, "
                                  "which is not implemented")
    if not torch.is_tensor(_on_gpu(colors_1, "colors_1")) or colors_1.dim() != 4 or colors_1.shape[1] != 3:
        raise ValueError("colors_1 must be an (N, 3, H, W) tensor")
    n, _, h, w = (int(v) for v in colors_1.shape)
    device = colors_1.device
    args = []
    for t, c, name in ((colors_1, 3, "colors_1"), (colors_2, 3, "colors_2"), (boundaries, 1, "boundaries"), (depths_1, 1, "depths_1"),
                       (depths_2, 1, "depths_2"), (sparse_depths_1, 1, "sparse_depths_1"), (sparse_depths_2, 1, "sparse_depths_2"),
                       (sparse_depth_masks_1, 1, "sparse_depth_masks_1"), (sparse_depth_masks_2, 1, "sparse_depth_masks_2"),
                       (warped_depths_2_to_1, 1, "warped_depths_2_to_1"), (warped_depths_1_to_2, 1, "warped_depths_1_to_2"),
                       (sparse_flows_1, 2, "sparse_flows_1"), (sparse_flows_2, 2, "sparse_flows_2"), (flows_1, 2, "flows_1"),
                       (flows_2, 2, "flows_2")):
        args.append(_device_f32(_on_gpu(t, name), (n, c, h, w), name, device))
    args.append(_device_f32(_on_gpu(intrinsics, "intrinsics"), (n, 3, 3), "intrinsics", device))
    if int(point_cloud_downsampling) < 1:
        raise ValueError("point_cloud_downsampling must be >= 1")
    lib = _lib.load()
    need = int(lib.endo_evaluate_validation_workspace_bytes(n, h, w))
    if need < 0:
        raise ValueError("a batch of %d pairs of %d x %d is outside endo_evaluate_validation's sizes" % (n, h, w))
    with torch.cuda.device(device):
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        panel = torch.empty(validation_panel_shape(n, h, w), dtype=torch.uint8, device=device)
        metrics = torch.empty((n, 2, 4), dtype=torch.float32, device=device)
        points = torch.empty((n * h * w, 6), dtype=torch.float32, device=device)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=device)
        _lib.check(lib.endo_evaluate_validation(*[_lib.ptr(a) for a in args], n, h, w, float(epsilon), 0, int(point_cloud_downsampling),
                                                _lib.ptr(panel), _lib.ptr(metrics), _lib.ptr(points), _lib.ptr(offsets),
                                                _lib.ptr(workspace), need, _lib.stream()), "endo_evaluate_validation")
    return {"panel": panel, "metrics": metrics, "points": points, "offsets": offsets}


def stack_and_display(phase, title, step, writer, panel):
    """utils.stack_and_display (utils.py:894-900) for a panel of ``panels()`` / ``TrainingStep.display_panels()``:
    ``writer.add_image(phase + '/Images/' + title, <the (3, 8 Hg, Wg) uint8 host array>, step)``.  One device-to-host copy."""
    if not torch.is_tensor(panel) or panel.dim() != 3 or panel.shape[2] != 3 or panel.dtype != torch.uint8:
        raise ValueError("panel must be an (H, W, 3) uint8 tensor")
    chw = panel.permute(2, 0, 1).contiguous().cpu().numpy()
    writer.add_image(phase + '/Images/' + title, chw, step)
    return chw
