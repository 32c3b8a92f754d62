"""numpy restatement of the test-phase outputs (reference evaluate.py:329-345 with utils.py:825-852; csrc/evaluate.hip): what the
device outputs are checked against.  Arithmetic as the reference's float32 numpy evaluates it, each operation rounded on its own;
cv2.COLOR_HSV2BGR_FULL and COLORMAP_JET restated from OpenCV's formulas (PARITY UNPINNED against cv2 itself: it is not installed).
Colour images are uint8 (H, W, 3) in cv2's B, G, R order."""

import numpy as np

from augment_restate import _SECTORS


def jet():
    """COLORMAP_JET as a (256, 3) uint8 table, B, G, R: x = i / 255, r = clip(min(4x - 1.5, 4.5 - 4x)), g = clip(min(4x - 0.5, 3.5 - 4x)),
    b = clip(min(4x + 0.5, 2.5 - 4x)), each x 255 rounded half to even (fp64).  cv2 first interpolates its table in float32, so it may
    differ from this on entries within a float32 rounding of .5."""
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(np.minimum(4.0 * x - 1.5, 4.5 - 4.0 * x), 0.0, 1.0)
    g = np.clip(np.minimum(4.0 * x - 0.5, 3.5 - 4.0 * x), 0.0, 1.0)
    b = np.clip(np.minimum(4.0 * x + 0.5, 2.5 - 4.0 * x), 0.0, 1.0)
    return np.rint(255.0 * np.stack([b, g, r], axis=-1)).astype(np.uint8)


JET = jet()


def hsv_full_to_bgr(hsv):
    """cv2.COLOR_HSV2BGR_FULL on uint8 (color_hsv HSV2RGB_b -> HSV2RGB_native, hscale = 6 / 256): augment_restate.hsv180_to_rgb with
    hue range 256, blue first."""
    hsv = np.asarray(hsv, np.uint8)
    f32 = np.float32
    s = hsv[..., 1].astype(f32) * f32(1.0 / 255.0)
    v = hsv[..., 2].astype(f32) * f32(1.0 / 255.0)
    h = hsv[..., 0].astype(f32) * f32(6.0 / 256.0)
    h = np.fmod(h, f32(6.0))
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f32(0), h).astype(f32)
    one = f32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    bgr = np.take_along_axis(tab, _SECTORS[sector], axis=-1)
    bgr = np.where((s == 0)[..., None], v[..., None], bgr) * f32(255.0)
    return np.clip(np.rint(bgr), 0, 255).astype(np.uint8)


def display_u8(c):
    """np.uint8(255 * (0.5 * c + 0.5)) of the (3, H, W) float32 masked input, as (H, W, 3) in its own channel order (evaluate.py:329-330)."""
    x = np.asarray(c, np.float32).transpose(1, 2, 0)
    return (np.float32(255) * (np.float32(0.5) * x + np.float32(0.5))).astype(np.uint8)


def color_display(c, b, is_hsv=False):
    """evaluate.py:329-337: (H, W, 3) uint8 B, G, R of the masked input c (3, H, W) and the boundary b (H, W)."""
    u = display_u8(c)
    u = hsv_full_to_bgr(u) if is_hsv else u[..., ::-1]
    return (np.asarray(b, np.float32).reshape(b.shape[-2], b.shape[-1], 1) * u).astype(np.uint8)


def depth_index(d):
    """np.uint8(255 * d / np.max(d)) of the masked depth (H, W) (evaluate.py:339); a frame whose maximum is 0 gives 0 everywhere."""
    d = np.asarray(d, np.float32)
    m = d.max()
    if not m > 0:
        return np.zeros(d.shape, np.uint8)
    return ((np.float32(255) * d) / m).astype(np.uint8)


def depth_display(d):
    return JET[depth_index(d)]


def panel(c, b, d, is_hsv=False):
    """cv2.hconcat([colour display, depth display]) (evaluate.py:345): (H, 2W, 3) uint8 B, G, R."""
    return np.concatenate([color_display(c, b, is_hsv), depth_display(d)], axis=1)


def point_cloud(d, color_bgr, b, k, downsampling=1):
    """utils.point_cloud_from_depth (utils.py:825-852) without thresholds, vectorised: (P, 6) float32 rows (x, y, z, r, g, b) of every
    kept pixel in row-major order, x = (w - cx) / fx * z in float32."""
    d = np.asarray(d, np.float32)
    height, width = d.shape
    k = np.asarray(k, np.float32).reshape(3, 3)
    hh, ww = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    keep = (hh % downsampling == 0) & (ww % downsampling == 0) & (np.asarray(b, np.float32).reshape(height, width) > 0.5)
    z = d[keep]
    x = (ww[keep].astype(np.float32) - k[0, 2]) / k[0, 0] * z
    y = (hh[keep].astype(np.float32) - k[1, 2]) / k[1, 1] * z
    col = np.asarray(color_bgr)[keep].astype(np.float32)
    return np.stack([x, y, z, col[:, 2], col[:, 1], col[:, 0]], axis=1).astype(np.float32).reshape(-1, 6)


def batch_outputs(colors, boundaries, predictions, intrinsics, is_hsv=False, downsampling=1):
    """Everything endo_evaluate writes for a batch, as numpy: depth (N, 1, H, W), panels (N, H, 2W, 3), the per-frame point clouds."""
    colors = np.asarray(colors, np.float32)
    boundaries = np.asarray(boundaries, np.float32)
    depth = boundaries * np.asarray(predictions, np.float32)
    panels, clouds = [], []
    for f in range(colors.shape[0]):
        b = boundaries[f, 0]
        disp = color_display(colors[f], b, is_hsv)
        panels.append(np.concatenate([disp, depth_display(depth[f, 0])], axis=1))
        clouds.append(point_cloud(depth[f, 0], disp, b, intrinsics[f], downsampling))
    return depth, np.stack(panels), clouds
