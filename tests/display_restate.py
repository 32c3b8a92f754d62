"""numpy restatement of the training / validation display panel (reference train.py:353-371 and 460-478: utils.display_color_depth_sparse_
flow_dense_flow for both frames, draw_flow and stack_and_display, utils.py:868-900, 965-994, over torchvision 0.7-era make_grid; csrc/
display.hip): what the device panel is checked against, bit for bit.  float32 arithmetic as torch and numpy evaluate it, each operation
rounded on its own.  COLORMAP_JET and cv2's 8-bit COLOR_HSV2BGR are the restatements of evaluate_restate.jet and
augment_restate.hsv180_to_rgb (PARITY UNPINNED against cv2 itself: it is not installed).  Images are uint8 (H, W, 3) R, G, B: what a
tensorboardX writer stores for the reference's float image (trunc(clip(255 x)) of u / 255 gives u back for every uint8 u)."""

import math

import numpy as np

from augment_restate import hsv180_to_rgb
from evaluate_restate import JET

F32 = np.float32


def grid_shape(n, h, w):
    """(Hg, Wg) of make_grid(nrow=8, padding=2) over n frames; n = 1: the frame itself."""
    if n == 1:
        return h, w
    xmaps = min(8, n)
    ymaps = int(math.ceil(float(n) / xmaps))
    return (h + 2) * ymaps + 2, (w + 2) * xmaps + 2


def make_grid(frames, pad_value=0.0):
    """torchvision make_grid(frames, nrow=8, padding=2, pad_value) of an (N, C, H, W) array, without normalisation: (C, Hg, Wg)."""
    frames = np.asarray(frames)
    n, c, h, w = frames.shape
    if n == 1:
        return frames[0].copy()
    gh, gw = grid_shape(n, h, w)
    xmaps = min(8, n)
    grid = np.full((c, gh, gw), pad_value, dtype=frames.dtype)
    for k in range(n):
        y, x = divmod(k, xmaps)
        grid[:, y * (h + 2) + 2:y * (h + 2) + 2 + h, x * (w + 2) + 2:x * (w + 2) + 2 + w] = frames[k]
    return grid


def to_u8(x):
    """tensorboardX's float image -> uint8: trunc(clip(255 x, 0, 255)) in float32."""
    return np.clip(np.asarray(x, F32) * F32(255), 0, 255).astype(np.uint8)


def color_section(colors):
    """make_grid(colors * 0.5 + 0.5) (utils.py:968), as the writer stores it: (Hg, Wg, 3); padding 0 = black."""
    x = (np.asarray(colors, F32) * F32(0.5) + F32(0.5)).astype(F32)
    return to_u8(make_grid(x).transpose(1, 2, 0))


def normalize_each(depth):
    """make_grid(normalize=True, scale_each=True)'s 0.7-era norm_ip on every frame of (N, 1, H, W): clamp to [min, max], subtract min,
    divide by the float32 of the Python float max - min + 1e-5."""
    out = np.empty_like(np.asarray(depth, F32))
    for f in range(out.shape[0]):
        t = np.asarray(depth[f], F32)
        lo, hi = float(t.min()), float(t.max())
        out[f] = (np.clip(t, F32(lo), F32(hi)) - F32(lo)) / F32(hi - lo + 1e-5)
    return out


def depth_section(depths, boundaries):
    """COLORMAP_JET of np.uint8(255 * make_grid(depth * boundary, normalize=True, scale_each=True)), B, G, R -> R, G, B (utils.py:972-975,
    982): (Hg, Wg, 3).  The padding is 0 before the colormap: JET entry 0."""
    d = (np.asarray(depths, F32) * np.asarray(boundaries, F32)).astype(F32)
    grid = make_grid(normalize_each(d))[0]
    idx = (F32(255) * grid).astype(np.uint8)
    return JET[idx][..., ::-1]


def flow_hsv(flows, max_v=None, literal=False):
    """draw_flow (utils.py:868-891) up to the HSV image: returns (hsv uint8 (Hg, Wg, 3), np.max(v)).  fx = x, fy = y * Hg / Wg, ang =
    arctan2(fy, fx) + pi, v = sqrt(fx^2 + fy^2), H = ang * (180 / pi / 2), S = 255, V = min(v / max_v, 1) * 255, all float32, truncated;
    V = 0 where v / max_v is NaN (0 / 0).  The angle is arctan2 in float64 rounded once to float32 (literal=False: the correctly rounded
    float32 the device forms) or numpy's float32 arctan2 (literal=True: the reference's own line, libm's atan2f)."""
    flows = np.asarray(flows, F32)
    gx = make_grid(flows[:, 0:1])[0]
    gy = make_grid(flows[:, 1:2])[0]
    h, w = gx.shape
    fx, fy = gx, gy * h / w
    if literal:
        ang = np.arctan2(fy, fx) + np.pi
    else:
        ang = np.arctan2(fy.astype(np.float64), fx.astype(np.float64)).astype(F32) + np.pi
    v = np.sqrt(fx * fx + fy * fy)
    hsv = np.zeros((h, w, 3), np.uint8)
    hsv[..., 0] = ang * (180 / np.pi / 2)
    hsv[..., 1] = 255
    top = np.max(v) if max_v is None else max_v
    with np.errstate(divide="ignore", invalid="ignore"):
        t = v / top
    val = np.minimum(np.where(np.isnan(t), F32(0), t), 1.0) * 255
    hsv[..., 2] = val.astype(np.uint8)
    return hsv, np.max(v)


def flow_section(flows, max_v=None):
    """draw_flow -> cv2.COLOR_HSV2BGR -> cv2.COLOR_BGR2RGB: (rgb uint8 (Hg, Wg, 3), np.max(v)).  The padding is black."""
    hsv, top = flow_hsv(flows, max_v)
    return hsv180_to_rgb(hsv), top


def half_sections(colors, depths, boundaries, sparse_flows, flows):
    """display_color_depth_sparse_flow_dense_flow(color_reverse=True) of one frame of the pair: [c, d, sf, df], the dense flows scaled by
    the sparse flows' max_v (utils.py:979-980)."""
    sf, top = flow_section(sparse_flows)
    df, _ = flow_section(flows, max_v=top)
    return [color_section(colors), depth_section(depths, boundaries), sf, df]


def panel(colors_1, colors_2, depths_1, depths_2, boundaries, sparse_flows_1, sparse_flows_2, flows_1, flows_2):
    """stack_and_display's np.vstack of c1, d1, sf1, df1, c2, d2, sf2, df2 (train.py:366-371): (8 Hg, Wg, 3) uint8 R, G, B."""
    return np.vstack(half_sections(colors_1, depths_1, boundaries, sparse_flows_1, flows_1) +
                     half_sections(colors_2, depths_2, boundaries, sparse_flows_2, flows_2))
