"""The numpy statement of csrc/fusion_track.hip and fusion.TSDFVolume.residuals / .track: the signed distance of every pixel of posed
depth maps to a fusion_restate.Volume, the normal equations of a similarity's Gauss-Newton step, and the loop around them.  The
per-pixel numbers are np.float32, one rounding per operation, in the order include/endo_hip.h (endo_fusion_track) states, and are
compared with the device's byte for byte; the 40 sums per frame are fp64 and differ from the device's by their order of addition alone.
There is no reference code for this step.  A plain module: it reads nothing outside the repository.

    pixels            per frame: which pixels are samples, their r, n, y, J (float32)
    sums_of           the 40 fp64 sums of one frame's samples (forward or reversed order of addition)
    residuals         endo_fusion_track: the three per-pixel outputs, the sums and the flags
    step_of, rodrigues, track   the Gauss-Newton loop of fusion.TSDFVolume.track
    height, render_height_field, curved_scene   the curved test scene: an analytic height field ray-cast by bisection in fp64
    mapped_rms        how far a pose maps a frame's points from where the true pose maps them
"""
import math

import numpy as np

import fusion_render_restate as rr
import fusion_restate as fr

F = fr.F
SUMS = 40          # count, sum r^2, sum |r|, max |r|, sum |y|^2, Jt r (7), the upper triangle of JtJ row by row (28)
UPPER = np.triu_indices(7)
SAMPLE, MASKED, BAD_DEPTH, OUTSIDE, UNOBSERVED, BAD_SCALE = range(6)          # pixels()' kind


def pixels(volume, depth, boundaries, k, rot, tr, scale, min_weight=1.0):
    """One frame.  Returns sample (H * W bool) and, for every pixel (meaningless outside the samples), r (float32), n, y (3 float32
    arrays each), J (7 float32 arrays), q = |y|^2 (float32), and kind: why a pixel is no sample (SAMPLE for one that is)."""
    height, width = depth.shape
    inv = F(1.0) / volume.vs
    per_unit = volume.trunc * inv
    tf, w, _ = rr._frame_rays(np.asarray(k, F), rot, tr, height, width, F(1.0))
    d, b, s = np.asarray(depth, F).reshape(-1), np.asarray(boundaries, F).reshape(-1), F(scale)
    with np.errstate(all="ignore"):
        scaled = bool(s > 0 and np.isfinite(s))
        ok = (b > F(0.5)) & np.isfinite(d) & (d > 0) & scaled
        sd = s * d
        y = [sd * w[a] for a in range(3)]
        inside = ok.copy()
        base, frac = [], []
        for a, n in enumerate((volume.nx, volume.ny, volume.nz)):
            x = tf[a] + y[a]
            g = (x - volume.origin[a]) * inv - F(0.5)
            c = np.floor(g)
            frac.append(g - c)
            inside &= (c >= 0) & (c <= F(n - 2))
            base.append(c)
        idx = [np.where(inside, c, F(0)).astype(np.int64) for c in base]
        sample = inside & rr._weights_ok(volume, idx, min_weight)
        phi, grad = rr._value_gradient(volume.tsdf, idx, frac)
        r = phi * volume.trunc
        n = [grad[a] * per_unit for a in range(3)]
        j = [y[1] * n[2] - y[2] * n[1], y[2] * n[0] - y[0] * n[2], y[0] * n[1] - y[1] * n[0], n[0], n[1], n[2],
             (n[0] * y[0] + n[1] * y[1]) + n[2] * y[2]]
        q = (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]
        kind = np.where(sample, SAMPLE, np.where(inside, UNOBSERVED, np.where(ok, OUTSIDE, np.where(b > F(0.5), BAD_DEPTH, MASKED))))
        if not scaled:
            kind[:] = BAD_SCALE
    assert r.dtype == F and q.dtype == F and all(v.dtype == F for v in n + y + j)
    return sample, r, n, y, j, q, kind


def terms_of(sample, r, j, q):
    """(S, 40) fp64: what each of the S samples adds to the sums (column 3 holds |r|, of which the sum takes the maximum)."""
    rd = r[sample].astype(np.float64)
    jd = np.stack([v[sample].astype(np.float64) for v in j], axis=1)
    out = np.zeros((rd.shape[0], SUMS))
    out[:, 0] = 1.0
    out[:, 1] = rd * rd
    out[:, 2] = np.abs(rd)
    out[:, 3] = np.abs(rd)
    out[:, 4] = q[sample].astype(np.float64)
    out[:, 5:12] = jd * rd[:, None]
    out[:, 12:] = jd[:, UPPER[0]] * jd[:, UPPER[1]]
    return out


def sums_of(terms, reverse=False):
    """The 40 sums of terms_of's rows, added one after the other in pixel order, or in the reversed order."""
    if reverse:
        terms = terms[::-1]
    out = np.zeros(SUMS)
    if terms.shape[0]:
        out[:] = np.cumsum(terms, axis=0)[-1]          # (cumsum adds sequentially; sum() adds pairwise)
        out[3] = terms[:, 3].max()
    return out


def residuals(volume, depth, boundaries, intrinsics, rotations, translations, scales=None, min_weight=1.0, reverse=False, detail=None):
    """endo_fusion_track.  depth, boundaries (N, H, W) float32; intrinsics (N, 3, 3) float32; rotations (N, 3, 3), translations (N, 3)
    float64; scales (N,) or None for ones.  Returns {"residual", "valid"} (N, 1, H, W) and {"gradient"} (N, H, W, 3) float32, {"sums"}
    (N, 40) fp64, {"flags"}.  ``detail``, a list, receives each frame's (terms_of, kind)."""
    depth, boundaries = np.asarray(depth, F), np.asarray(boundaries, F)
    n, height, width = depth.shape
    intrinsics = np.asarray(intrinsics, F).reshape(n, 3, 3)
    rotations = np.asarray(rotations, np.float64).reshape(n, 3, 3)
    translations = np.asarray(translations, np.float64).reshape(n, 3)
    scales = np.ones(n, F) if scales is None else np.asarray(scales, np.float64).astype(F).reshape(n)
    residual, valid = np.zeros((n, height * width), F), np.zeros((n, height * width), F)
    gradient = np.zeros((n, height * width, 3), F)
    sums, flags = np.zeros((n, SUMS)), []
    for f in range(n):
        with np.errstate(all="ignore"):
            flags.append("ok" if scales[f] > 0 and np.isfinite(scales[f]) else "bad_scale")
        sample, r, nrm, _, j, q, kind = pixels(volume, depth[f], boundaries[f], intrinsics[f], rotations[f], translations[f], scales[f], min_weight)
        residual[f][sample] = r[sample]
        valid[f][sample] = F(1.0)
        for a in range(3):
            gradient[f][sample, a] = nrm[a][sample]
        terms = terms_of(sample, r, j, q)
        sums[f] = sums_of(terms, reverse)
        if detail is not None:
            detail.append((terms, kind))
    return {"residual": residual.reshape(n, 1, height, width), "valid": valid.reshape(n, 1, height, width),
            "gradient": gradient.reshape(n, height, width, 3), "sums": sums, "flags": flags}


def rms_of(sums):
    return math.sqrt(sums[1] / sums[0]) if sums[0] > 0 else float("nan")


def rodrigues(omega):
    omega = np.asarray(omega, np.float64)
    angle = float(np.linalg.norm(omega))
    k = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if angle < 1.0e-12:
        return np.eye(3) + k
    return np.eye(3) + (math.sin(angle) / angle) * k + ((1.0 - math.cos(angle)) / (angle * angle)) * (k @ k)


def normal_matrix(sums):
    a = np.zeros((7, 7))
    a[UPPER] = sums[12:40]
    return a + np.triu(a, 1).T


def step_of(sums, with_scale=True, damping=0.0):
    """(omega, tau, sigma) as 7 fp64 numbers from (JtJ + damping diag(JtJ)) delta = -Jt r, or None where the Cholesky factorisation fails."""
    m = 7 if with_scale else 6
    a, b = normal_matrix(sums)[:m, :m], sums[5:5 + m]
    a = a + damping * np.diag(np.diag(a))
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return None
    try:
        lower = np.linalg.cholesky(a)
    except np.linalg.LinAlgError:
        return None
    delta = np.zeros(7)
    delta[:m] = -np.linalg.solve(lower.T, np.linalg.solve(lower, b))
    return delta if np.isfinite(delta).all() else None


def track(volume, depth, boundaries, intrinsics, rotations, translations, scales=None, with_scale=True, iterations=20, tolerance=None,
          min_weight=1.0, min_count=64, damping=0.0, reverse=False):
    """fusion.TSDFVolume.track: a list of one dictionary per frame with rotation, translation, scale, iterations, converged, status,
    count, rms, initial_rms and history."""
    n = np.asarray(depth).shape[0]
    rot = np.array(rotations, np.float64).reshape(n, 3, 3)
    tr = np.array(translations, np.float64).reshape(n, 3)
    scales = np.ones(n) if scales is None else np.array(scales, np.float64).reshape(n)
    tolerance = 1.0e-3 * float(volume.vs) if tolerance is None else float(tolerance)
    start = (rot.copy(), tr.copy(), scales.copy())
    status, steps, converged = ["ok"] * n, [0] * n, [False] * n
    history, initial = [[] for _ in range(n)], [float("nan")] * n
    active = list(range(n))

    def call(frames):          # (only the frames still moving: the others' sums are not looked at)
        out = residuals(volume, np.asarray(depth, F)[frames], np.asarray(boundaries, F)[frames], np.asarray(intrinsics, F)[frames], rot[frames],
                        tr[frames], scales[frames], min_weight, reverse)
        return dict(zip(frames, out["sums"])), dict(zip(frames, out["flags"]))

    for it in range(int(iterations)):
        if not active:
            break
        sums, flags = call(list(active))
        for f in list(active):
            history[f].append(rms_of(sums[f]))
            if it == 0:
                initial[f] = history[f][0]
            delta = None
            if flags[f] != "ok":
                status[f] = flags[f]
            elif sums[f][0] < min_count:
                status[f] = "too_few"
            else:
                delta = step_of(sums[f], with_scale, damping)
                if delta is None:
                    status[f] = "singular"
            if delta is None:
                rot[f], tr[f], scales[f] = start[0][f], start[1][f], start[2][f]
                active.remove(f)
                continue
            rot[f] = rodrigues(delta[:3]) @ rot[f]
            tr[f] = tr[f] + delta[3:6]
            scales[f] = scales[f] * math.exp(delta[6])
            steps[f] += 1
            rho = math.sqrt(sums[f][4] / sums[f][0])
            if max(np.linalg.norm(delta[:3]) * rho, np.linalg.norm(delta[3:6]), abs(delta[6]) * rho) <= tolerance:
                converged[f] = True
                active.remove(f)
    sums, flags = call(list(range(n)))
    out = []
    for f in range(n):
        if status[f] == "ok" and flags[f] != "ok":
            status[f] = flags[f]
        if not history[f]:
            initial[f] = rms_of(sums[f])
        out.append({"rotation": rot[f].copy(), "translation": tr[f].copy(), "scale": float(scales[f]), "iterations": steps[f],
                    "converged": converged[f], "status": status[f], "count": int(round(sums[f][0])), "rms": rms_of(sums[f]),
                    "initial_rms": initial[f], "history": history[f]})
    return out


# ---- the curved scene: z = height(x, y), seen from cameras near the origin looking along +z

SCENE_FRAMES, SCENE_H, SCENE_W = 6, 48, 64
SCENE_DIMS, SCENE_VS, SCENE_TRUNC = (64, 56, 40), 0.5, 1.5
SCENE_ORIGIN = (-0.5 * SCENE_DIMS[0] * SCENE_VS, -0.5 * SCENE_DIMS[1] * SCENE_VS, 30.0 - 0.5 * SCENE_DIMS[2] * SCENE_VS)


def height(x, y):
    """Curved in both directions and twisted: a plane would leave scale and the translation along its normal indistinguishable, a
    sphere the rotation free."""
    return 30.0 + 1.5 * np.sin(x / 2.0) + 1.2 * np.cos(y / 1.7) + 0.04 * x * y


def render_height_field(rot, tr, k, h, w):
    """fp64: the z-depth map (h, w) float32 of the height field seen by the camera x = R x_cam + t, by 60 bisections of [5, 60]."""
    k = np.asarray(k, np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dx, dy = (u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1]
    ray = np.stack([rot[a, 0] * dx + rot[a, 1] * dy + rot[a, 2] for a in range(3)])
    lo, hi = np.full((h, w), 5.0), np.full((h, w), 60.0)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        p = np.asarray(tr, np.float64)[:, None, None] + mid * ray
        below = p[2] < height(p[0], p[1])
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return (0.5 * (lo + hi)).astype(F)


_curved = {}


def curved_scene(seed=0, true_scales=None):
    """Six 48 x 64 frames of the height field from random poses (up to 6 degrees, +-2, +-2, +-1 units), integrated into 64 x 56 x 40
    voxels of 0.5 with truncation 1.5.  Frame f's depth map is the true one divided by true_scales[f] (None: ones), so its true scale
    is true_scales[f].  Returns a dictionary (made once per key and left unchanged): volume, depth, boundaries, colors, intrinsics,
    rotations, translations, scales."""
    key = (seed, None if true_scales is None else tuple(float(s) for s in true_scales))
    if key in _curved:
        return _curved[key]
    rng = np.random.default_rng(seed)
    k = fr.intrinsics(60.0, SCENE_H, SCENE_W)
    rotations = np.stack([fr.rotation_about(rng.normal(size=3), rng.uniform(0.0, 6.0)) for _ in range(SCENE_FRAMES)])
    translations = np.stack([np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-1, 1)]) for _ in range(SCENE_FRAMES)])
    scales = np.ones(SCENE_FRAMES, F) if true_scales is None else np.asarray(true_scales, F)
    depth = np.stack([render_height_field(rotations[f], translations[f], k, SCENE_H, SCENE_W) for f in range(SCENE_FRAMES)]) / scales[:, None, None]
    boundaries = np.ones_like(depth)
    colors = rng.integers(0, 256, (SCENE_FRAMES, SCENE_H, SCENE_W, 3), dtype=np.uint8)
    intrinsics = np.stack([k] * SCENE_FRAMES)
    volume = fr.Volume(SCENE_ORIGIN, SCENE_VS, SCENE_DIMS, truncation=SCENE_TRUNC)
    assert fr.integrate(volume, depth, boundaries, colors, intrinsics, rotations, translations, scales=scales) == ["ok"] * SCENE_FRAMES
    _curved[key] = {"volume": volume, "depth": depth.astype(F), "boundaries": boundaries, "colors": colors, "intrinsics": intrinsics,
                    "rotations": rotations, "translations": translations, "scales": scales.astype(np.float64)}
    return _curved[key]


def perturbed(scene, seed, degrees=1.5, shift=0.3, scale=1.03):
    """The prototype's start: every frame's pose ``degrees`` about a random axis, a normal ``shift`` per coordinate and ``scale`` away."""
    rng = np.random.default_rng(1000 + seed)
    n = scene["rotations"].shape[0]
    rotations = np.stack([fr.rotation_about(rng.normal(size=3), degrees) @ scene["rotations"][f] for f in range(n)])
    translations = scene["translations"] + rng.normal(size=(n, 3)) * shift
    return rotations, translations, scene["scales"] * scale


POINTS = np.random.default_rng(7).uniform(-1, 1, (100, 3)) * [8.0, 6.0, 0.0] + [0.0, 0.0, 30.0]


def mapped_rms(pose, other):
    """The rms distance between where two poses (rotation, translation, scale) map the same camera points: the points are POINTS, a
    patch of the surface's neighbourhood, taken into the camera by ``other``."""
    (ra, ta, sa), (rb, tb, sb) = pose, other
    cam = (POINTS - tb) @ rb / sb
    moved = (sa * cam) @ np.asarray(ra).T + ta
    return float(np.sqrt(((moved - POINTS) ** 2).sum(axis=1).mean()))


# ---- evaluate.run_fusion_phase(refine=K) on a synthetic sequence of the curved scene

def jittered_sequence(seed=3, degrees=1.0, shift=0.2, scale_jitter=0.02):
    """The curved scene as a sequence with a tracker's errors: every pose ``degrees`` about a random axis and a normal ``shift`` per
    coordinate off, and every frame's own scale 20 / (z_max - z_min) up to ``scale_jitter`` off 1.  The mask keeps the image's centre,
    where the surface spans less than 20 units of depth, and one kept pixel per frame is pinned 20 / (1 + e_f) below the frame's
    largest kept depth, so that the frame's own scale is 1 + e_f.  Returns a dictionary: depth (the predictions), boundaries, colors,
    intrinsics, rotations and translations (the tracker's), true_rotations, true_translations (the true scale is 1)."""
    scene = curved_scene(0)
    rng = np.random.default_rng(seed)
    n = SCENE_FRAMES
    depth = scene["depth"].copy()
    boundaries = np.zeros_like(depth)
    boundaries[:, 6:42, 8:56] = 1.0
    off = rng.uniform(-scale_jitter, scale_jitter, n)
    for f in range(n):
        kept = depth[f][boundaries[f] > 0]
        assert kept.max() - kept.min() < 19.0
        depth[f, 6, 8] = F(kept.max() - 20.0 / (1.0 + off[f]))
    rotations = np.stack([fr.rotation_about(rng.normal(size=3), degrees) @ scene["rotations"][f] for f in range(n)])
    translations = scene["translations"] + rng.normal(size=(n, 3)) * shift
    return {"depth": depth, "boundaries": boundaries, "colors": scene["colors"], "intrinsics": scene["intrinsics"], "rotations": rotations,
            "translations": translations, "true_rotations": scene["rotations"], "true_translations": scene["translations"]}


def errors_to_truth(sequence, rotations, translations, scales):
    return np.array([mapped_rms((rotations[f], translations[f], scales[f]), (sequence["true_rotations"][f], sequence["true_translations"][f], 1.0))
                     for f in range(len(scales))])


def around_bounds(low, high, resolution, margin=8, truncation_voxels=4):
    """fusion.TSDFVolume.around_bounds: origin, voxel size, dims and truncation."""
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    voxel = float((high - low).max()) / int(resolution)
    dims = [int(math.ceil(float(side) / voxel)) + 1 + 2 * margin for side in (high - low)]
    dims[0] = (dims[0] + 3) // 4 * 4
    return low - margin * voxel, voxel, dims, truncation_voxels * voxel


def refine(sequence, rounds, resolution=64, min_weight=2.0):
    """run_fusion_phase(refine=rounds) restated: the volume around the posed points, the frames integrated under the tracker's poses
    and their own scales, then ``rounds`` times tracked, cleared and integrated again.  Returns (the frames' mapped-point errors to
    the truth before, after, the final rotations, translations, scales, the last round's fits)."""
    depth, boundaries, k = sequence["depth"], sequence["boundaries"], sequence["intrinsics"]
    n, height, width = depth.shape
    own, flags = fr.frame_scales(depth, boundaries)
    assert flags == ["ok"] * n
    rot, tra, scales = sequence["rotations"].copy(), sequence["translations"].copy(), own.astype(np.float64)
    low, high = np.full(3, np.inf), np.full(3, -np.inf)
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    for f in range(n):
        ray = np.stack([(u - k[f, 0, 2]) / k[f, 0, 0], (v - k[f, 1, 2]) / k[f, 1, 1], np.ones_like(u)], axis=-1)
        points = ((scales[f] * depth[f].astype(np.float64))[..., None] * ray)[boundaries[f] > 0.5] @ rot[f].T + tra[f]
        low, high = np.minimum(low, points.min(axis=0)), np.maximum(high, points.max(axis=0))
    origin, voxel, dims, truncation = around_bounds(low, high, resolution)

    def fused():
        volume = fr.Volume(origin, voxel, dims, truncation=truncation)
        fr.integrate(volume, depth, boundaries, sequence["colors"], k, rot, tra, scales=scales.astype(F))
        return volume

    before = errors_to_truth(sequence, rot, tra, scales)
    volume, fits = fused(), []
    for _ in range(rounds):
        fits = track(volume, depth, boundaries, k, rot, tra, scales, min_weight=min_weight)
        for f, fit in enumerate(fits):
            if fit["status"] == "ok":
                rot[f], tra[f], scales[f] = fit["rotation"], fit["translation"], fit["scale"]
        volume = fused()
    return before, errors_to_truth(sequence, rot, tra, scales), rot, tra, scales, fits
