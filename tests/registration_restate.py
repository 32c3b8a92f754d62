"""numpy fp64 restatement of the similarity registration (registration.py over csrc/registration.hip): a brute-force nearest neighbour,
Umeyama's closed form, the ICP loop with the product's cap rule and stop rule, and the fixture the tests register.  Nothing here
imports the product."""
import math

import numpy as np

FIXTURE_K, FIXTURE_M = 1500, 400
FIXTURE_SCALE = 1.25
FIXTURE_TRANSLATION = np.array([0.3, -0.2, 0.4])


def rotation_about(axis, degrees):
    """Rodrigues' formula."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * k + (1.0 - math.cos(th)) * (k @ k)


FIXTURE_ROTATION = rotation_about((1.0, 2.0, 3.0), 8.0)


def fixture(seed, sigma=0.0, junk=0, k=FIXTURE_K, m=FIXTURE_M):
    """A wavy tube offset from the origin (the target) and m of its rows, noisy by sigma, the first `junk` of them pushed 2-4 units
    away, moved by the inverse of the similarity to recover.  Returns (source, target) as float32 and the true (scale, R, t) source ->
    target about the target's fp64 mean: y = c0 R0 (x - ctr) + ctr + t0."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 2.0 * np.pi, k)
    z = rng.uniform(0.0, 12.0, k)
    r = 4.0 + 0.8 * np.sin(3.0 * u + 0.5 * z) + 0.5 * np.cos(u) * np.sin(0.9 * z) + 0.15 * z
    target = np.stack([r * np.cos(u), 1.3 * r * np.sin(u), z + 0.6 * np.sin(2.0 * u)], axis=1) + np.array([150.0, -80.0, 60.0])
    sel = rng.choice(k, m, replace=False)
    y = target[sel] + sigma * rng.standard_normal((m, 3))          # drawn when sigma = 0 too: the later draws stay the same
    if junk > 0:
        push = rng.uniform(2.0, 4.0, junk)
        direction = rng.standard_normal((junk, 3))
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        y[:junk] += push[:, None] * direction
    ctr = target.mean(axis=0)
    source = (y - ctr - FIXTURE_TRANSLATION) @ FIXTURE_ROTATION / FIXTURE_SCALE + ctr
    true_t = ctr + FIXTURE_TRANSLATION - FIXTURE_SCALE * (FIXTURE_ROTATION @ ctr)
    return source.astype(np.float32), target.astype(np.float32), (FIXTURE_SCALE, FIXTURE_ROTATION.copy(), true_t)


def apply(points, scale, rotation, translation):
    """scale * R x + t for rows x, in fp64."""
    return scale * (np.asarray(points, np.float64)[:, :3] @ np.asarray(rotation, np.float64).T) + np.asarray(translation, np.float64)


def squared_distances(moved, target, chunk=2048):
    """(M, K) squared distances by direct differences in fp64, in chunks of rows."""
    moved = np.asarray(moved, np.float64)[:, :3]
    target = np.asarray(target, np.float64)[:, :3]
    out = np.empty((moved.shape[0], target.shape[0]))
    for at in range(0, moved.shape[0], chunk):
        diff = moved[at:at + chunk, None, :] - target[None, :, :]
        out[at:at + chunk] = (diff * diff).sum(axis=2)
    return out


def nearest(moved, target, fp32_score=False):
    """Index (argmin: the lowest of equal ones) and fp64 distance of the nearest target row.  fp32_score=True orders the targets as the
    matrix-unit kernel does: coordinates relative to the target's fp64 mean rounded to float32, score = |t|^2 - 2 x.t as a float32
    fmaf chain; the distance is still the fp64 one to the chosen row."""
    moved = np.asarray(moved, np.float64)[:, :3]
    target64 = np.asarray(target, np.float64)[:, :3]
    if fp32_score:
        ctr = target64.mean(axis=0)
        t = (target64 - ctr).astype(np.float32)
        x = (moved - ctr).astype(np.float32)
        def fma(a, b, c):
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)          # exact product, one rounding
        norm = fma(t[:, 2], t[:, 2], fma(t[:, 1], t[:, 1], (t[:, 0] * t[:, 0]).astype(np.float32)))
        a = np.float32(-2.0) * t
        score = fma(a[None, :, 0], x[:, None, 0], np.zeros((1, 1), np.float32))
        score = fma(a[None, :, 1], x[:, None, 1], score)
        score = fma(a[None, :, 2], x[:, None, 2], score)
        score = fma(norm[None, :], np.ones((1, 1), np.float32), score)
        index = score.argmin(axis=1)
    else:
        index = squared_distances(moved, target64).argmin(axis=1)
    diff = moved - target64[index]
    return index, np.sqrt((diff * diff).sum(axis=1))


def sums_of(source, target, index, distance, cap, source_centre, target_centre):
    """The 20 sums of endo_registration_match over the rows with distance <= cap."""
    keep = distance <= cap
    s = np.asarray(source, np.float64)[keep, :3] - source_centre
    t = np.asarray(target, np.float64)[index[keep], :3] - target_centre
    d = distance[keep]
    out = np.zeros(20)
    out[0] = keep.sum()
    out[1], out[2] = d.sum(), (d * d).sum()
    out[3] = d.max() if d.size else 0.0
    out[4:7], out[7:10] = s.sum(axis=0), t.sum(axis=0)
    out[10] = (s * s).sum()
    out[11:20] = (t.T @ s).reshape(9)
    return out


def umeyama(source, target, with_scale=True):
    """Least-squares similarity target ~ c R source + t over corresponding rows (Umeyama 1991), det R = +1."""
    source = np.asarray(source, np.float64)
    target = np.asarray(target, np.float64)
    n = source.shape[0]
    ms, mt = source.mean(axis=0), target.mean(axis=0)
    s, t = source - ms, target - mt
    var = (s * s).sum() / n
    if n < 3 or var <= 0.0:
        raise ValueError("%d rows do not determine a similarity" % n)
    u, d, vt = np.linalg.svd(t.T @ s / n)
    sign = np.ones(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        sign[2] = -1.0
    rot = (u * sign) @ vt
    c = float((d * sign).sum() / var) if with_scale else 1.0
    return c, rot, mt - c * (rot @ ms)


def register(source, target, scale=1.0, rotation=None, translation=None, with_scale=True, iterations=50, tolerance=1e-9,
             max_distance=None, reject_factor=3.0, fp32_score=False):
    """The product's loop: match under the cap, Umeyama on the kept rows, cap = min(max_distance, reject_factor * rms), stop when
    |rms_prev - rms| <= tolerance * rms; one more match at the end.  Returns a dictionary."""
    rot = np.eye(3) if rotation is None else np.asarray(rotation, np.float64)
    tr = np.zeros(3) if translation is None else np.asarray(translation, np.float64)
    c = float(scale)
    top = np.inf if max_distance is None else float(max_distance)
    cap = top
    history, converged, previous = [], False, None
    for _ in range(iterations):
        index, dist = nearest(apply(source, c, rot, tr), target, fp32_score)
        keep = dist <= cap
        if keep.sum() < 3:
            raise ValueError("%d rows are within the distance cap" % keep.sum())
        rms = math.sqrt(float((dist[keep] ** 2).sum() / keep.sum()))
        history.append(rms)
        c, rot, tr = umeyama(np.asarray(source, np.float64)[keep, :3], np.asarray(target, np.float64)[index[keep], :3], with_scale)
        if reject_factor is not None:
            cap = min(top, reject_factor * rms)
        if previous is not None and abs(previous - rms) <= tolerance * rms:
            converged = True
            break
        previous = rms
    index, dist = nearest(apply(source, c, rot, tr), target, fp32_score)
    keep = dist <= cap
    return {"scale": c, "rotation": rot, "translation": tr, "index": index, "distance": dist, "count": int(keep.sum()),
            "rms": math.sqrt(float((dist[keep] ** 2).sum() / max(1, keep.sum()))), "iterations": len(history), "converged": converged,
            "history": history}
