"""numpy restatement of evaluate.py's validation phase (reference evaluate.py:201-274): the 12-section panel of utils.display_color_sparse_
depth_dense_depth_warped_depth_sparse_flow_dense_flow for both frames and stack_and_display (utils.py:894-954) over torchvision 0.7-era
make_grid, and the two error measures AbsRelError and Threshold (losses.py:189-227); csrc/evaluate_validation.hip is checked against it, the
panel bit for bit.  float32 arithmetic as torch and numpy evaluate it, each operation rounded on its own.  The pieces shared with the
training panel (make_grid, COLORMAP_JET, draw_flow, the uint8 conversion) are display_restate's."""

import numpy as np

import display_restate as dr
from evaluate_restate import JET

F32 = np.float32


def color_section(colors, boundaries):
    """make_grid((colors * 0.5 + 0.5) * boundaries) (utils.py:912), as evaluate.py:270 and the writer store it: (Hg, Wg, 3)."""
    x = ((np.asarray(colors, F32) * F32(0.5) + F32(0.5)).astype(F32) * np.asarray(boundaries, F32)).astype(F32)
    return dr.to_u8(dr.make_grid(x).transpose(1, 2, 0))


def depth_range(depths, boundaries):
    """(min, max) of scaled_depth * boundaries over the whole batch, as Python floats (utils.py:921-922 on evaluate.py:230's product)."""
    d = (np.asarray(depths, F32) * np.asarray(boundaries, F32)).astype(F32)
    return float(d.min()), float(d.max())


def ranged_depth_section(values, lo, hi):
    """COLORMAP_JET of np.uint8(255 * make_grid(values, normalize=True, scale_each=False, range=(lo, hi))), B, G, R -> R, G, B
    (utils.py:924-940, 946-948): 0.7-era norm_ip on the whole batch -- clamp to [lo, hi], subtract lo, divide by the float32 of the Python
    float hi - lo + 1e-5 -- then the grid, whose padding is 0 before the colormap: JET entry 0."""
    t = np.asarray(values, F32)
    x = ((np.clip(t, F32(lo), F32(hi)) - F32(lo)) / F32(hi - lo + 1e-5)).astype(F32)
    idx = (F32(255) * dr.make_grid(x)[0]).astype(np.uint8)
    return JET[idx][..., ::-1]


def half_sections(colors, sparse_depths, depths, warped, sparse_flows, flows, boundaries):
    """One frame of the pair: [c, sd, d, wd, sf, df]; the dense flows set draw_flow's max_v, which the sparse flows reuse
    (utils.py:942-943)."""
    lo, hi = depth_range(depths, boundaries)
    masked = (np.asarray(depths, F32) * np.asarray(boundaries, F32)).astype(F32)
    df, top = dr.flow_section(flows)
    sf, _ = dr.flow_section(sparse_flows, max_v=top)
    return [color_section(colors, boundaries), ranged_depth_section(sparse_depths, lo, hi), ranged_depth_section(masked, lo, hi),
            ranged_depth_section(warped, lo, hi), sf, df]


def panel(colors_1, colors_2, boundaries, depths_1, depths_2, sparse_depths_1, sparse_depths_2, warped_2_to_1, warped_1_to_2,
          sparse_flows_1, sparse_flows_2, flows_1, flows_2):
    """stack_and_display's np.vstack of c1 sd1 d1 wd1 sf1 df1 c2 sd2 d2 wd2 sf2 df2 (evaluate.py:257-268): (12 Hg, Wg, 3) uint8 R, G, B."""
    return np.vstack(half_sections(colors_1, sparse_depths_1, depths_1, warped_2_to_1, sparse_flows_1, flows_1, boundaries) +
                     half_sections(colors_2, sparse_depths_2, depths_2, warped_1_to_2, sparse_flows_2, flows_2, boundaries))


def cloud_colors(colors):
    """np.uint8(255 * (0.5 * c + 0.5)) of one (3, H, W) masked frame as (H, W, 3) B, G, R: the point colours (evaluate.py:329-334)."""
    x = np.asarray(colors, F32).transpose(1, 2, 0)
    return (F32(255) * (F32(0.5) * x + F32(0.5))).astype(np.uint8)[..., ::-1]


def _terms(depths, sparse, masks, eps):
    d, s, m = (np.asarray(a, F32) for a in (depths, sparse, masks))
    eps = F32(eps)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rel = (m * np.abs(d - s)) / (eps + s)
        dm = d * m
        ratio = np.maximum(dm / (eps + s), s / (eps + dm))          # np.maximum keeps a NaN, as torch.max does
        thr = m * ratio + (F32(1.0) - m) * F32(10.0)
    assert rel.dtype == F32 and thr.dtype == F32
    return rel, thr, m


def abs_rel_error(depths, sparse, masks, eps=1.0e-8):
    """AbsRelError.forward (losses.py:194-199) on (N, 1, H, W) arrays: (N,) float32.  The per-pixel terms are float32; their sum is
    exact up to one rounding (fp64 accumulation, as the device forms it), the quotient float32.  An empty mask: NaN."""
    rel, _, m = _terms(depths, sparse, masks, eps)
    n = rel.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return rel.reshape(n, -1).sum(axis=1, dtype=np.float64).astype(F32) / m.reshape(n, -1).sum(axis=1, dtype=np.float64).astype(F32)


def threshold(depths, sparse, masks, eps=1.0e-8):
    """Threshold.forward (losses.py:207-227): [sigma_1, sigma_2, sigma_3], each (N,) float32: the count of threshold_map < 1.25^k over the
    mask sum.  An empty mask: NaN."""
    _, thr, m = _terms(depths, sparse, masks, eps)
    n = thr.shape[0]
    den = m.reshape(n, -1).sum(axis=1, dtype=np.float64).astype(F32)
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for bound in (1.25, 1.25 * 1.25, 1.25 * 1.25 * 1.25):
            out.append((thr < F32(bound)).reshape(n, -1).sum(axis=1).astype(F32) / den)
    return out


def metrics(depths, sparse, masks, eps=1.0e-8):
    """(N, 4) float32: [abs rel, sigma 1, sigma 2, sigma 3] per sample, as endo_depth_metrics lays them out."""
    return np.stack([abs_rel_error(depths, sparse, masks, eps)] + threshold(depths, sparse, masks, eps), axis=1)
