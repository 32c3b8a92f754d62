"""The numpy float32 statement of csrc/fusion.hip and fusion.py: what a TSDF volume holds after posed depth maps have been integrated
into it, and the surface rows extracted from it.  Every operation is done on np.float32 values, one rounding each, in the order the
header (include/endo_hip.h, endo_fusion_integrate / endo_fusion_extract) states, so the device planes and rows are compared with it
byte for byte.  There is no reference code for this step.  A plain module: it reads nothing outside the repository.

    Volume            the five planes and the grid's numbers
    frame_scales      the pre-pass: each frame's scale and flag
    integrate         frames into a Volume, in order; returns the flags
    extract           the surface rows of a Volume
    render_plane      fp64 helper: the exact depth maps of a plane seen by posed pinhole cameras
    intrinsics        a (3, 3) pinhole matrix
    rotation_about    a rotation matrix from an axis and degrees
"""
import numpy as np

F = np.float32
FLAGS = ("ok", "empty", "zero_range", "bad_scale")


class Volume(object):
    def __init__(self, origin, voxel_size, dims, truncation=None, max_weight=64.0):
        self.nx, self.ny, self.nz = (int(v) for v in dims)
        self.origin = np.asarray(origin, np.float64).astype(F)
        self.vs = F(voxel_size)
        self.trunc = F(4.0 * float(voxel_size) if truncation is None else truncation)
        self.max_weight = F(max_weight)
        shape = (self.nz, self.ny, self.nx)
        self.tsdf = np.ones(shape, F)
        self.weight = np.zeros(shape, F)
        self.color = np.zeros((3,) + shape, F)

    def centres(self):
        """The voxel centres per axis: o + (float(index) + 0.5) * vs, each operation rounded."""
        return [self.origin[a] + (np.arange(n, dtype=F) + F(0.5)) * self.vs for a, n in enumerate((self.nx, self.ny, self.nz))]

    def copy(self):
        other = Volume(self.origin, self.vs, (self.nx, self.ny, self.nz), self.trunc, self.max_weight)
        other.tsdf, other.weight, other.color = self.tsdf.copy(), self.weight.copy(), self.color.copy()
        return other


def frame_scales(depth, boundaries, scales=None):
    """The pre-pass.  depth, boundaries: (N, H, W) float32.  Returns (scales float32 (N,), flags list): the caller's scales, or
    20.0f / (z_max - z_min) over the pixels with boundaries > 0.5 of boundaries * depth (minimum and maximum skip NaN, as fminf /
    fmaxf do)."""
    depth, boundaries = np.asarray(depth, F), np.asarray(boundaries, F)
    n = depth.shape[0]
    out, flags = np.zeros(n, F), []
    for f in range(n):
        kept = boundaries[f] > F(0.5)
        d = (boundaries[f] * depth[f])[kept]
        zmin = np.fmin.reduce(d, initial=F(np.inf)) if d.size else F(np.inf)
        zmax = np.fmax.reduce(d, initial=F(-np.inf)) if d.size else F(-np.inf)
        flag, s = "ok", F(0.0)
        with np.errstate(all="ignore"):
            if zmin > zmax:
                flag = "empty"
            elif scales is not None:
                s = F(np.asarray(scales, F).reshape(-1)[f])
            elif zmin == zmax:
                flag = "zero_range"
            else:
                s = F(20.0) / (F(zmax) - F(zmin))
        if flag == "ok" and not (s > 0 and np.isfinite(s)):
            flag = "bad_scale"
        out[f] = s
        flags.append(flag)
    return out, flags


def integrate(volume, depth, boundaries, colors_u8, intrinsics, rotations, translations, scales=None):
    """endo_fusion_integrate.  depth, boundaries (N, H, W) float32; colors_u8 (N, H, W, 3) uint8; intrinsics (N, 3, 3) float32;
    rotations (N, 3, 3), translations (N, 3) float64.  Updates ``volume`` in place, returns the flags."""
    depth, boundaries = np.asarray(depth, F), np.asarray(boundaries, F)
    n, height, width = depth.shape
    colors_u8 = np.asarray(colors_u8, np.uint8).reshape(n, height, width, 3)
    intrinsics = np.asarray(intrinsics, F).reshape(n, 3, 3)
    rotations = np.asarray(rotations, np.float64).reshape(n, 3, 3)
    translations = np.asarray(translations, np.float64).reshape(n, 3)
    frame_s, flags = frame_scales(depth, boundaries, scales)
    cx, cy, cz = volume.centres()
    c = [cx[None, None, :], cy[None, :, None], cz[:, None, None]]
    shape = volume.tsdf.shape
    for f in range(n):
        if flags[f] != "ok":
            continue
        rt = rotations[f].T.astype(F)
        t = translations[f].astype(F)
        d = [np.broadcast_to(c[a] - t[a], shape) for a in range(3)]
        p = [(rt[r, 0] * d[0] + rt[r, 1] * d[1]) + rt[r, 2] * d[2] for r in range(3)]
        fx, ccx, fy, ccy = intrinsics[f, 0, 0], intrinsics[f, 0, 2], intrinsics[f, 1, 1], intrinsics[f, 1, 2]
        with np.errstate(all="ignore"):
            u = np.rint(fx * (p[0] / p[2]) + ccx)
            v = np.rint(fy * (p[1] / p[2]) + ccy)
            valid = (p[2] > 0) & (u >= 0) & (u <= F(width - 1)) & (v >= 0) & (v <= F(height - 1))
        ui = np.where(valid, u, F(0)).astype(np.int64)
        vi = np.where(valid, v, F(0)).astype(np.int64)
        z = depth[f][vi, ui]
        with np.errstate(all="ignore"):
            valid &= boundaries[f][vi, ui] > F(0.5)
            valid &= np.isfinite(z) & (z > 0)
            sdf = frame_s[f] * z - p[2]
            valid &= ~(sdf < -volume.trunc)
            val = np.minimum(F(1.0), sdf / volume.trunc)
            w0 = volume.weight
            w1 = w0 + F(1.0)
            tsdf = (volume.tsdf * w0 + val) / w1
            volume.tsdf = np.where(valid, tsdf, volume.tsdf).astype(F)
            for ch in range(3):
                col = (volume.color[ch] * w0 + colors_u8[f][vi, ui, ch].astype(F)) / w1
                volume.color[ch] = np.where(valid, col, volume.color[ch]).astype(F)
            volume.weight = np.where(valid, np.minimum(w1, volume.max_weight), w0).astype(F)
    assert volume.tsdf.dtype == F and volume.weight.dtype == F and volume.color.dtype == F
    return flags


def extract(volume, min_weight=1.0):
    """endo_fusion_count / endo_fusion_extract: (P, 6) float32 rows."""
    t, w = volume.tsdf, volume.weight
    ok = w >= F(min_weight)
    neg = t < 0
    has = np.zeros(t.shape + (3,), bool)
    has[:, :, :-1, 0] = ok[:, :, :-1] & ok[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    has[:, :-1, :, 1] = ok[:, :-1, :] & ok[:, 1:, :] & (neg[:, :-1, :] != neg[:, 1:, :])
    has[:-1, :, :, 2] = ok[:-1] & ok[1:] & (neg[:-1] != neg[1:])
    k, j, i, e = np.nonzero(has)          # (k, j, i) order, the edges +x, +y, +z inside a voxel
    rows = np.zeros((k.shape[0], 6), F)
    if not k.shape[0]:
        return rows
    kb, jb, ib = k + (e == 2), j + (e == 1), i + (e == 0)
    ta, tb = t[k, j, i], t[kb, jb, ib]
    lam = ta / (ta - tb)
    cx, cy, cz = volume.centres()
    step = lam * volume.vs
    rows[:, 0] = np.where(e == 0, cx[i] + step, cx[i])
    rows[:, 1] = np.where(e == 1, cy[j] + step, cy[j])
    rows[:, 2] = np.where(e == 2, cz[k] + step, cz[k])
    for out, ch in ((3, 2), (4, 1), (5, 0)):          # r, g, b = channels 2, 1, 0
        ca, cb = volume.color[ch][k, j, i], volume.color[ch][kb, jb, ib]
        rows[:, out] = np.rint(ca + lam * (cb - ca))
    return rows


def intrinsics(focal, height, width):
    return np.array([[focal, 0.0, 0.5 * (width - 1)], [0.0, focal, 0.5 * (height - 1)], [0.0, 0.0, 1.0]], F)


def rotation_about(axis, degrees):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    a = np.radians(degrees)
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(a) * k + (1.0 - np.cos(a)) * (k @ k)


def render_plane(normal, offset, rotations, translations, k, height, width, scale=1.0):
    """fp64: the depth maps (N, H, W) float32 of the plane normal . x = offset seen by cameras posed x = R (scale * x_cam) + t with the
    pinhole matrix k; 0 where the pixel's ray does not meet the plane in front of the camera."""
    normal = np.asarray(normal, np.float64)
    k = np.asarray(k, np.float64)
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    rays = np.stack([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], np.ones_like(u)], axis=-1)
    maps = []
    for rot, tr in zip(rotations, translations):
        rot, tr = np.asarray(rot, np.float64), np.asarray(tr, np.float64)
        along = (rays @ rot.T) @ normal
        with np.errstate(all="ignore"):
            z = (offset - normal @ tr) / along / scale
        maps.append(np.where(np.isfinite(z) & (z > 0), z, 0.0))
    return np.stack(maps).astype(F)
