"""The numpy float32 statement of csrc/fusion_render.hip and fusion.TSDFVolume.render: a fusion_restate.Volume seen from posed pinhole
cameras, one ray per pixel marched to the first zero crossing of the trilinear tsdf.  Every operation is done on np.float32 values, one
rounding each, in the order include/endo_hip.h (endo_fusion_render) states, so the device's depth, mask, colours and normals are
compared with it byte for byte.  There is no reference code for this step.  A plain module: it reads nothing outside the repository.

    brick_marks       the marks of the empty-space skipping
    sample_times      t_k of every ray: the sample grid, which no skipping changes
    render            the four outputs, and what happened on the way (``stats``)

Which samples are evaluated is not part of the contract (the device clips k to the grid by slabs, this file by the distance of the
volume's corners from the camera); which sample ends a ray, and everything computed from it, is.
"""
import numpy as np

import fusion_restate as fr

F = fr.F
MAX_SAMPLES = 1 << 20
NO_RAY, HIT, ENDED, MISS = 0, 1, 2, 3          # stats["outcome"]


def _lerp(a, b, r):
    return a + r * (b - a)


def brick_marks(volume, min_weight, brick):
    """(nbz, nby, nbx) bool: brick b covers voxels b * brick .. b * brick + brick on every axis (the cells whose base voxel lies in it)
    and is marked when it holds a voxel with weight >= min_weight and tsdf <= 0."""
    with np.errstate(all="ignore"):
        q = (volume.weight >= F(min_weight)) & (volume.tsdf <= 0)
    for axis in (2, 1, 0):
        count = (q.shape[axis] + brick - 1) // brick
        q = np.stack([np.take(q, range(b * brick, min(b * brick + brick + 1, q.shape[axis])), axis=axis).any(axis=axis) for b in range(count)],
                     axis=axis)
    return q


def _frame_rays(k, rot, tr, height, width, step_length):
    rf, tf = np.asarray(rot, np.float64).astype(F), np.asarray(tr, np.float64).astype(F)
    fx, cx, fy, cy = k[0, 0], k[0, 2], k[1, 1], k[1, 2]
    with np.errstate(all="ignore"):
        dx = np.broadcast_to(((np.arange(width, dtype=F) - cx) / fx)[None, :], (height, width)).reshape(-1)
        dy = np.broadcast_to(((np.arange(height, dtype=F) - cy) / fy)[:, None], (height, width)).reshape(-1)
        w = [(rf[r, 0] * dx + rf[r, 1] * dy) + rf[r, 2] for r in range(3)]
        dt = step_length / np.sqrt((dx * dx + dy * dy) + F(1.0))
    assert dt.dtype == F and all(x.dtype == F for x in w)
    return tf, w, dt


def sample_times(k, rot, tr, height, width, voxel_size, step, samples):
    """(samples, H * W) float32: t_1 .. t_samples of every pixel's ray."""
    _, _, dt = _frame_rays(np.asarray(k, F), rot, tr, height, width, F(step) * F(voxel_size))
    return np.arange(1, samples + 1, dtype=F)[:, None] * dt[None, :]


def _locate(volume, inv, tf, w, dt, k):
    """The cells of sample k (a number or one per ray): inside, (i, j, k) of the base voxel (0 outside), the three fractions."""
    with np.errstate(all="ignore"):
        tk = np.asarray(k).astype(F) * dt
        inside = np.ones(dt.shape, bool)
        base, frac = [], []
        for a, n in enumerate((volume.nx, volume.ny, volume.nz)):
            x = tf[a] + tk * w[a][...]
            g = (x - volume.origin[a]) * inv - F(0.5)
            b = np.floor(g)
            frac.append(g - b)
            inside &= (b >= 0) & (b <= F(n - 2))
            base.append(b)
        assert all(x.dtype == F for x in frac)
        idx = [np.where(inside, b, F(0)).astype(np.int64) for b in base]
    return inside, idx, frac


def _corners(plane, idx):
    i, j, k = idx
    nz, ny, nx = plane.shape          # (a ray outside the grid has base 0 and is not looked at: its +1 stays inside a one-voxel axis)
    return [[[plane[np.minimum(k + z, nz - 1), np.minimum(j + y, ny - 1), np.minimum(i + x, nx - 1)] for x in (0, 1)] for y in (0, 1)]
            for z in (0, 1)]          # [z][y][x]


def _value(plane, idx, frac):
    c = _corners(plane, idx)
    with np.errstate(all="ignore"):
        b = [_lerp(_lerp(c[z][0][0], c[z][0][1], frac[0]), _lerp(c[z][1][0], c[z][1][1], frac[0]), frac[1]) for z in (0, 1)]
        return _lerp(b[0], b[1], frac[2])


def _value_gradient(plane, idx, frac):
    c = _corners(plane, idx)
    rx, ry, rz = frac
    with np.errstate(all="ignore"):
        d = [[c[z][y][1] - c[z][y][0] for y in (0, 1)] for z in (0, 1)]
        a = [[c[z][y][0] + rx * d[z][y] for y in (0, 1)] for z in (0, 1)]
        gx = _lerp(_lerp(d[0][0], d[0][1], ry), _lerp(d[1][0], d[1][1], ry), rz)
        e = [a[z][1] - a[z][0] for z in (0, 1)]
        b = [a[z][0] + ry * e[z] for z in (0, 1)]
        gy = _lerp(e[0], e[1], rz)
        gz = b[1] - b[0]
        return b[0] + rz * gz, [gx, gy, gz]


def _weights_ok(volume, idx, min_weight):
    ok = np.ones(idx[0].shape, bool)
    with np.errstate(all="ignore"):
        for plane in _corners(volume.weight, idx):
            for row in plane:
                for value in row:
                    ok &= value >= F(min_weight)
    return ok


def _sample_range(volume, rot, tr, step_length):
    """fp64, conservative: the first and last k at which any ray of a camera at ``tr`` can be inside the grid."""
    lo = volume.origin.astype(np.float64)
    hi = lo + float(volume.vs) * np.array([volume.nx, volume.ny, volume.nz])
    tr = np.asarray(tr, np.float64)
    nearest = np.linalg.norm(tr - np.clip(tr, lo, hi))
    farthest = np.linalg.norm(np.maximum(np.abs(tr - lo), np.abs(tr - hi)))
    sigma = np.linalg.svd(np.asarray(rot, np.float64), compute_uv=False)          # a sample advances sigma_min .. sigma_max steps
    if not (np.isfinite(sigma).all() and sigma.min() > 0 and np.isfinite(farthest)):
        return 1, MAX_SAMPLES
    first = int(max(1.0, np.floor(nearest / (sigma.max() * float(step_length))) - 2.0))
    last = int(min(float(MAX_SAMPLES), np.ceil(farthest / (sigma.min() * float(step_length))) + 2.0))
    return first, last


def render(volume, intrinsics, rotations, translations, height, width, scales=None, boundaries=None, min_weight=1.0, step=0.5, skip=True,
           brick=8, stats=None):
    """endo_fusion_render.  intrinsics (N, 3, 3) float32; rotations (N, 3, 3), translations (N, 3) float64; scales (N,) or None;
    boundaries (N, H, W) float32 or None.  Returns {"depth", "mask"} (N, 1, H, W) float32, {"colors"} (N, H, W, 3) uint8 and
    {"normals"} (N, H, W, 3) float32.  ``stats``, a dictionary, receives: outcome (N, H, W) of NO_RAY / HIT / ENDED / MISS; evaluated and
    skipped, the numbers of samples inside the grid that were and were not evaluated; skipped_before_end, the rays whose ending sample
    follows a skipped one; end (N, H, W), the ending sample's k or 0; and with skip=False: unsafe, the ending samples that lie in an
    unmarked brick (the brick rule holds when it is 0), and observed_miss, the misses that met a valid sample."""
    intrinsics = np.asarray(intrinsics, F).reshape(-1, 3, 3)
    n = intrinsics.shape[0]
    rotations = np.asarray(rotations, np.float64).reshape(n, 3, 3)
    translations = np.asarray(translations, np.float64).reshape(n, 3)
    scales = np.ones(n, F) if scales is None else np.asarray(scales, F).reshape(n)
    if boundaries is not None:
        boundaries = np.asarray(boundaries, F).reshape(n, height * width)
    step_length = F(step) * volume.vs
    assert F(step) > 0 and step_length <= volume.trunc and (volume.nx + volume.ny + volume.nz + 6.0) / float(F(step)) <= MAX_SAMPLES
    inv = F(1.0) / volume.vs
    marks = brick_marks(volume, min_weight, brick)
    pixels = height * width
    depth, mask = np.zeros((n, pixels), F), np.zeros((n, pixels), F)
    colors, normals = np.zeros((n, pixels, 3), np.uint8), np.zeros((n, pixels, 3), F)
    outcome, ends = np.zeros((n, pixels), np.int64), np.zeros((n, pixels), np.int64)
    count = {"evaluated": 0, "skipped": 0, "skipped_before_end": 0, "unsafe": 0, "observed_miss": 0}
    for f in range(n):
        s = scales[f]
        if not (s > 0 and np.isfinite(s)):
            continue
        tf, w, dt = _frame_rays(intrinsics[f], rotations[f], translations[f], height, width, step_length)
        with np.errstate(all="ignore"):
            cast = (dt > 0) & np.isfinite(dt)
            if boundaries is not None:
                cast &= boundaries[f] > F(0.5)
        outcome[f][cast] = MISS
        alive = cast.copy()
        end = np.zeros(pixels, np.int64)
        observed = np.zeros(pixels, bool)
        first, last = _sample_range(volume, rotations[f], translations[f], step_length)
        for k in range(first, last + 1):
            sel = np.nonzero(alive)[0]
            if not sel.size:
                break
            inside, idx, frac = _locate(volume, inv, tf, [x[sel] for x in w], dt[sel], k)
            marked = inside & marks[idx[2] // brick, idx[1] // brick, idx[0] // brick]
            consider = marked if skip else inside
            count["evaluated"] += int(consider.sum())
            count["skipped"] += int((inside & ~consider).sum())
            with np.errstate(all="ignore"):
                ending = consider & (_value(volume.tsdf, idx, frac) <= 0)
            if skip:
                ending[ending] = _weights_ok(volume, [x[ending] for x in idx], min_weight)
            else:
                ok = inside & _weights_ok(volume, idx, min_weight)
                observed[sel] |= ok
                ending &= ok
                count["unsafe"] += int((ending & ~marked).sum())
            end[sel[ending]] = k
            alive[sel[ending]] = False
        ends[f] = end
        outcome[f][end > 0] = ENDED
        count["observed_miss"] += int((observed & (end == 0)).sum())
        sel = np.nonzero(end > 1)[0]
        if not sel.size:
            continue
        ws, dts = [x[sel] for x in w], dt[sel]
        inside, ia, ra = _locate(volume, inv, tf, ws, dts, end[sel] - 1)
        count["skipped_before_end"] += int((inside & ~marks[ia[2] // brick, ia[1] // brick, ia[0] // brick]).sum())
        fa, ga = _value_gradient(volume.tsdf, ia, ra)
        with np.errstate(all="ignore"):
            hit = inside & _weights_ok(volume, ia, min_weight) & (fa > 0)
        if not hit.any():
            continue
        sel, ws, dts = sel[hit], [x[hit] for x in ws], dts[hit]
        ia, ra, fa, ga = [x[hit] for x in ia], [x[hit] for x in ra], fa[hit], [x[hit] for x in ga]
        inside, ib, rb = _locate(volume, inv, tf, ws, dts, end[sel])
        assert inside.all()
        fb, gb = _value_gradient(volume.tsdf, ib, rb)
        with np.errstate(all="ignore"):
            lam = fa / (fa - fb)
            ts = (end[sel] - 1).astype(F) * dts + lam * dts
            depth[f][sel] = ts / s
            mask[f][sel] = F(1.0)
            outcome[f][sel] = HIT
            for c in range(3):
                blended = np.rint(_lerp(_value(volume.color[c], ia, ra), _value(volume.color[c], ib, rb), lam))
                colors[f][sel, c] = np.fmin(np.fmax(blended, F(0.0)), F(255.0)).astype(np.uint8)
            v = [_lerp(ga[a], gb[a], lam) for a in range(3)]
            length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            unit = np.isfinite(length) & (length > 0)
            for a in range(3):
                normals[f][sel, a] = np.where(unit, v[a] / length, F(0.0))
            assert lam.dtype == F and ts.dtype == F and length.dtype == F
    if stats is not None:
        stats.update(count)
        stats["outcome"] = outcome.reshape(n, height, width)
        stats["end"] = ends.reshape(n, height, width)
    return {"depth": depth.reshape(n, 1, height, width), "mask": mask.reshape(n, 1, height, width),
            "colors": colors.reshape(n, height, width, 3), "normals": normals.reshape(n, height, width, 3)}
