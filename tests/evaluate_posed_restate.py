"""numpy restatement of the posed test output (reference utils.py:1316-1355 write_test_output_with_initial_pose, utils.py:1246-1295
point_cloud_from_depth_and_initial_pose, utils.py:773-781 display_depth_map; csrc/evaluate_posed.hip): what the device outputs are
checked against.  tests/golden/make_evaluate_posed_golden.py asserts that it equals the reference's own functions bit for bit.

The arithmetic is numpy 2's (weak Python scalars): float32 throughout, each operation rounded on its own, up to the position
p = (x, y, z) * scale; then float64 for R p + t in the order ((R_i0 p_x + R_i1 p_y) + R_i2 p_z) + t_i, without contraction, and one
rounding to float32.  Colour images keep the reference's channel order: an RGB input stays R, G, B (there is no swap before cv2.imwrite),
an HSV input becomes B, G, R through COLOR_HSV2BGR_FULL; a point's (r, g, b) are channels (2, 1, 0) either way."""

import numpy as np

import evaluate_restate as er

F32 = np.float32


def color_image(c, is_hsv=False):
    """utils.py:1330-1336: (H, W, 3) uint8 of the (3, H, W) float32 network input; not multiplied by the boundary."""
    x = np.asarray(c, F32).transpose(1, 2, 0)
    v = x * F32(0.5) + F32(0.5)
    v = np.where(v < 0, F32(0), v)
    v = np.where(v > 1, F32(1), v).astype(F32)
    u = (F32(255) * v).astype(np.uint8)
    return er.hsv_full_to_bgr(u) if is_hsv else u


def depth_index(d, min_value=None, max_value=None):
    """display_depth_map before applyColorMap (utils.py:774-780) on an (H, W) float32 map; max == min (0 / 0 in the reference) gives 0."""
    d = np.asarray(d, F32)
    if min_value is None or max_value is None:
        min_value, max_value = d.min(), d.max()
    min_value, max_value = F32(min_value), F32(max_value)
    span = max_value - min_value
    if not span > 0:
        return np.zeros(d.shape, np.uint8)
    v = np.abs((d - min_value) / span * F32(255))
    v = np.where(v > 255, F32(255), v)
    v = np.where(v <= 0, F32(0), v)
    return v.astype(np.uint8)


def depth_image(d, min_value=None, max_value=None):
    """(H, W, 3) uint8 B, G, R: COLORMAP_JET of depth_index."""
    return er.JET[depth_index(d, min_value, max_value)]


def kept(b, downsampling):
    """utils.py:1262: the pixels whose depth enters the z range."""
    b = np.asarray(b, F32)
    height, width = b.shape
    hh, ww = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return (hh % downsampling == 0) & (ww % downsampling == 0) & (b > 0.5)


def frame_range(d, b, downsampling):
    """(z_min, z_max) over the kept pixels as float32; (+inf, -inf) when there is none."""
    z = np.asarray(d, F32)[kept(b, downsampling)]
    if z.size == 0:
        return F32(np.inf), F32(-np.inf)
    return z.min(), z.max()


def point_cloud(d, color_img, b, k, translation, rotation, downsampling=1, min_threshold=None, max_threshold=None):
    """utils.py:1246-1295 vectorised: (P, 6) float32 rows (x, y, z, r, g, b) in row-major order.  d, b (H, W); color_img (H, W, 3) uint8;
    k (3, 3) float32; translation (3,) and rotation (3, 3) float64.  Raises ZeroDivisionError when no pixel is kept, as the reference
    does (its z_min / z_max sentinels are Python ints)."""
    d = np.asarray(d, F32)
    height, width = d.shape
    k = np.asarray(k, F32).reshape(3, 3)
    rot = np.asarray(rotation, np.float64).reshape(3, 3)
    t = np.asarray(translation, np.float64).reshape(3)
    keep = kept(np.asarray(b, F32).reshape(height, width), downsampling)
    if not keep.any():
        raise ZeroDivisionError("float division by zero")
    hh, ww = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    z = d[keep]
    with np.errstate(all="ignore"):
        scale = F32(20.0) / (z.max() - z.min())
        x = (ww[keep].astype(F32) - k[0, 2]) / k[0, 0] * z
        y = (hh[keep].astype(F32) - k[1, 2]) / k[1, 1] * z
        px, py, pz = ((v * scale).astype(np.float64) for v in (x, y, z))
        xyz = [(((rot[i, 0] * px + rot[i, 1] * py) + rot[i, 2] * pz) + t[i]).astype(F32) for i in range(3)]
    col = np.asarray(color_img, np.uint8).reshape(height, width, 3)[keep]
    rows = np.stack(xyz + [col[:, 2].astype(F32), col[:, 1].astype(F32), col[:, 0].astype(F32)], axis=1).astype(F32).reshape(-1, 6)
    if max_threshold is not None and min_threshold is not None:
        rows = rows[(col.max(axis=1).astype(F32) >= F32(max_threshold)) & (col.min(axis=1).astype(F32) <= F32(min_threshold))]
    return rows


def batch_outputs(colors, boundaries, predictions, intrinsics, rotations, translations, is_hsv=False, downsampling=1, min_threshold=None,
                  max_threshold=None):
    """Everything endo_evaluate_posed writes for a batch, as numpy: depth (N, 1, H, W), colour images and depth images (N, H, W, 3), the
    per-frame point clouds (a frame without kept pixels: an empty cloud) and the (N, 2) frame ranges."""
    colors = np.asarray(colors, F32)
    boundaries = np.asarray(boundaries, F32)
    depth = boundaries * np.asarray(predictions, F32)
    color_images, depth_images, clouds, ranges = [], [], [], []
    for f in range(colors.shape[0]):
        b = boundaries[f, 0]
        img = color_image(colors[f], is_hsv)
        color_images.append(img)
        depth_images.append(depth_image(depth[f, 0]))
        ranges.append(frame_range(depth[f, 0], b, downsampling))
        if kept(b, downsampling).any():
            clouds.append(point_cloud(depth[f, 0], img, b, intrinsics[f], translations[f], rotations[f], downsampling, min_threshold,
                                      max_threshold))
        else:
            clouds.append(np.zeros((0, 6), F32))
    return depth, np.stack(color_images), np.stack(depth_images), clouds, np.array(ranges, F32).reshape(-1, 2)
