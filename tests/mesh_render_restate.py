"""The numpy float32 statement of csrc/mesh_render.hip and mesh.TriangleMesh.render: a triangle mesh seen from posed pinhole cameras,
the ray through every pixel centre against every triangle, the nearest hit kept.  Every operation is done on np.float32 values, one
rounding each, in the order include/endo_hip.h (endo_mesh_render) states, so the device's outputs are compared with it byte for byte.
There is no reference code for this step.  A plain module: it reads nothing outside the repository.

    render       every pixel against every triangle (in chunks of triangles), np.argmin for the tie rule: the outputs
    icosphere, tube, pixel_grid, mixed_mesh, look_at, intrinsics       the meshes and cameras the tests share

There is no pixel box here: the device's box only has to be conservative, and its bytes are held to this file with the box and without.
"""
import numpy as np

F = np.float32
CULL_BACK, CULL_FRONT, BRUTE = 1, 2, 4          # ENDO_MESH_* of include/endo_hip.h
FRAME_OK, FRAME_BAD_SCALE = 0, 3                # ENDO_FUSION_FRAME_*
CHUNK = 256


def _edge(px, py, qx, qy):
    return px * qy - py * qx          # two products, each rounded, then the difference: f(Q, P) = -f(P, Q) exactly


def _camera_vertices(xyz, rf, tf):
    q = [xyz[:, a] - tf[a] for a in range(3)]
    return [(rf[0, a] * q[0] + rf[1, a] * q[1]) + rf[2, a] * q[2] for a in range(3)]


def render(vertices, faces, intrinsics, rotations, translations, height, width, scales=None, boundaries=None, cull=0):
    """endo_mesh_render.  vertices (V, 3 or 6) float32, faces (T, 3) int32, intrinsics (N, 3, 3) float32, rotations (N, 3, 3) and
    translations (N, 3) float64, scales (N,) or None, boundaries (N, H, W) or None, cull 0, CULL_BACK or CULL_FRONT.  Returns depth and
    mask (N, 1, H, W) float32, triangle (N, H, W) int32, barycentric and normals (N, H, W, 3) float32, colors (N, H, W, 3) uint8 (None
    without colour columns) and flags (N,) int32."""
    vertices = np.asarray(vertices, F)
    vertices = vertices.reshape(-1, vertices.shape[-1] if vertices.ndim == 2 else 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    count, triangles = vertices.shape[0], faces.shape[0]
    intrinsics = np.asarray(intrinsics, F).reshape(-1, 3, 3)
    n = intrinsics.shape[0]
    rotations = np.asarray(rotations, np.float64).reshape(n, 3, 3)
    translations = np.asarray(translations, np.float64).reshape(n, 3)
    scales = np.ones(n, F) if scales is None else np.asarray(scales, F).reshape(n)
    pixels = height * width
    with_colors = vertices.shape[1] >= 6
    depth, mask = np.zeros((n, pixels), F), np.zeros((n, pixels), F)
    triangle = np.full((n, pixels), -1, np.int32)
    bary, normals = np.zeros((n, pixels, 3), F), np.zeros((n, pixels, 3), F)
    colors = np.zeros((n, pixels, 3), np.uint8) if with_colors else None
    flags = np.zeros(n, np.int32)
    usable = np.nonzero(((faces >= 0) & (faces < count)).all(axis=1))[0]
    for f in range(n):
        s = scales[f]
        if not (s > 0 and np.isfinite(s)):
            flags[f] = FRAME_BAD_SCALE
            continue
        if not usable.size:
            continue
        k = intrinsics[f]
        rf, tf = rotations[f].astype(F), translations[f].astype(F)
        with np.errstate(all="ignore"):
            dx = np.broadcast_to(((np.arange(width, dtype=F) - k[0, 2]) / k[0, 0])[None, :], (height, width)).reshape(-1)
            dy = np.broadcast_to(((np.arange(height, dtype=F) - k[1, 2]) / k[1, 1])[:, None], (height, width)).reshape(-1)
            cam = _camera_vertices(vertices, rf, tf)
        best_t = np.full(pixels, np.inf, F)
        best = {name: np.zeros(pixels, F) for name in ("u", "v", "w", "det")}
        best_face = np.full(pixels, -1, np.int64)
        for start in range(0, usable.size, CHUNK):
            ids = usable[start:start + CHUNK]
            corner = [[cam[a][faces[ids, c]][:, None] for a in range(3)] for c in range(3)]          # [corner][axis] (t, 1)
            with np.errstate(all="ignore"):
                sx = [corner[c][0] - dx[None, :] * corner[c][2] for c in range(3)]
                sy = [corner[c][1] - dy[None, :] * corner[c][2] for c in range(3)]
                u = _edge(sx[2], sy[2], sx[1], sy[1])
                v = _edge(sx[0], sy[0], sx[2], sy[2])
                w = _edge(sx[1], sy[1], sx[0], sy[0])
                det = (u + v) + w
                t = ((u * corner[0][2] + v * corner[1][2]) + w * corner[2][2]) / det
                assert t.dtype == F and det.dtype == F
                inside = ((u >= 0) & (v >= 0) & (w >= 0)) | ((u <= 0) & (v <= 0) & (w <= 0))
                for side in (sx, sy):          # the span rule: the ray lies inside the three sheared vertices' box
                    inside &= ~((side[0] > 0) & (side[1] > 0) & (side[2] > 0)) & ~((side[0] < 0) & (side[1] < 0) & (side[2] < 0))
                ok = inside & (det != 0) & np.isfinite(t) & (t > 0)
                if cull == CULL_BACK:
                    ok &= ~(det < 0)
                elif cull == CULL_FRONT:
                    ok &= ~(det > 0)
            t = np.where(ok, t, F(np.inf))
            row = np.argmin(t, axis=0)          # the first of equal values: the lowest face index
            cols = np.arange(pixels)
            better = t[row, cols] < best_t          # strictly: an earlier chunk's equal t has the lower index
            best_t = np.where(better, t[row, cols], best_t)
            best_face = np.where(better, ids[row], best_face)
            for name, values in (("u", u), ("v", v), ("w", w), ("det", det)):
                best[name] = np.where(better, values[row, cols], best[name])
        hit = best_face >= 0
        if boundaries is not None:
            hit &= np.asarray(boundaries, F).reshape(n, pixels)[f] > F(0.5)
        sel = np.nonzero(hit)[0]
        if not sel.size:
            continue
        face = faces[best_face[sel]]
        u, v, w, det = (best[name][sel] for name in ("u", "v", "w", "det"))
        with np.errstate(all="ignore"):
            depth[f, sel] = best_t[sel] / s
            mask[f, sel] = F(1.0)
            triangle[f, sel] = best_face[sel]
            beta = [u / det, v / det, w / det]
            for c in range(3):
                bary[f, sel, c] = beta[c]
            a, b, c = (vertices[face[:, i], :3] for i in range(3))
            e1, e2 = b - a, c - a
            nv = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
            length = np.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
            unit = np.isfinite(length) & (length > 0)
            for i in range(3):
                value = np.where(unit, nv[i] / length, F(0.0))
                normals[f, sel, i] = np.where(det < 0, -value, value)          # towards the camera: det > 0 is the front
            if with_colors:
                for byte in range(3):
                    col = 5 - byte          # rows hold r, g, b = planes 2, 1, 0 (endo_fusion_extract); byte c is plane c
                    mixed = (beta[0] * vertices[face[:, 0], col] + beta[1] * vertices[face[:, 1], col]) + beta[2] * vertices[face[:, 2], col]
                    colors[f, sel, byte] = np.fmin(np.fmax(np.rint(mixed), F(0.0)), F(255.0)).astype(np.uint8)
            assert length.dtype == F and beta[0].dtype == F
    return {"depth": depth.reshape(n, 1, height, width), "mask": mask.reshape(n, 1, height, width),
            "triangle": triangle.reshape(n, height, width), "barycentric": bary.reshape(n, height, width, 3),
            "normals": normals.reshape(n, height, width, 3),
            "colors": colors.reshape(n, height, width, 3) if with_colors else None, "flags": flags}


# ---- the meshes and cameras the tests share ------------------------------------------------------------------------------------------
def intrinsics(focal, height, width):
    return np.array([[focal, 0.0, (width - 1) / 2.0], [0.0, focal, (height - 1) / 2.0], [0.0, 0.0, 1.0]], F)


def icosphere(subdivisions=2, radius=1.0):
    """A closed sphere of 20 * 4^subdivisions triangles, counter-clockwise as seen from outside: (V, 3) float32 and (T, 3) int32."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    points = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
              (-g, 0, -1), (-g, 0, 1)]
    points = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in points]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        middle, out = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in middle:
                p = points[i] + points[j]
                points.append(p / np.linalg.norm(p))
                middle[key] = len(points) - 1
            return middle[key]

        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return (np.asarray(points) * radius).astype(F), np.asarray(faces, np.int32)


def tube(rings=8, sectors=12, radius=1.0, length=4.0, bend=0.3):
    """An open, gently bent tube along z of rings x sectors quads (two triangles each), normals towards the axis: the endoscope's view
    from inside.  (V, 3) float32 and (T, 3) int32."""
    points, faces = [], []
    for r in range(rings + 1):
        z = length * r / rings
        for s in range(sectors):
            angle = 2.0 * np.pi * s / sectors
            rad = radius * (1.0 + 0.15 * np.sin(3.0 * angle + z))
            points.append((rad * np.cos(angle) + bend * np.sin(z), rad * np.sin(angle), z))
    for r in range(rings):
        for s in range(sectors):
            a, b = r * sectors + s, r * sectors + (s + 1) % sectors
            c, d = a + sectors, b + sectors
            faces += [(a, c, b), (b, c, d)]
    return np.asarray(points, F), np.asarray(faces, np.int32)


def pixel_grid(k, height, width, depth=2.0, every=3):
    """A planar grid of quads at z = depth whose vertices lie exactly on the rays of pixel centres (every ``every``-th pixel and the
    last one), for a camera at the origin with identity rotation.  The vertex of pixel (u, v) is (d_x depth, d_y depth, depth) in
    float32, d as the kernel computes it: with depth a power of two the products are exact."""
    k = np.asarray(k, F)
    us = sorted(set(list(range(0, width, every)) + [width - 1]))
    vs = sorted(set(list(range(0, height, every)) + [height - 1]))
    dx = (np.asarray(us, F) - k[0, 2]) / k[0, 0]
    dy = (np.asarray(vs, F) - k[1, 2]) / k[1, 1]
    z = F(depth)
    points = [(dx[i] * z, dy[j] * z, z) for j in range(len(vs)) for i in range(len(us))]
    faces = []
    for j in range(len(vs) - 1):
        for i in range(len(us) - 1):
            a = j * len(us) + i
            b, c, d = a + 1, a + len(us), a + len(us) + 1
            faces += [(a, b, c), (b, d, c)]
    return np.asarray(points, F), np.asarray(faces, np.int32)


def mixed_mesh(seed=0, small=150):
    """``small`` triangles far smaller than a pixel of the test cameras, scattered in front of the origin, then one triangle that
    covers any image from there, behind them."""
    rng = np.random.default_rng(seed)
    centres = np.stack([rng.uniform(-0.8, 0.8, small), rng.uniform(-0.6, 0.6, small), rng.uniform(1.5, 3.0, small)], axis=1)
    points = (centres[:, None, :] + rng.normal(scale=0.004, size=(small, 3, 3))).reshape(-1, 3)
    faces = np.arange(3 * small).reshape(small, 3)
    big = np.array([[-40.0, -30.0, 4.0], [40.0, -30.0, 4.5], [0.0, 60.0, 5.0]])
    return np.concatenate([points, big]).astype(F), np.concatenate([faces, [[3 * small, 3 * small + 1, 3 * small + 2]]]).astype(np.int32)


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """The rotation (camera to model, columns x right, y down, z forward) of a camera at ``eye`` looking at ``target``."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(-np.asarray(up, np.float64), z)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross((1.0, 0.0, 0.0), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q
