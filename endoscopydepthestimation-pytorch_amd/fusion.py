"""Volumetric fusion of a sequence's posed depth maps into one surface: a truncated signed distance function (TSDF) on a voxel grid,
averaged over the frames that saw a voxel, with its zero crossings as one coloured cloud.  evaluate.run_posed_test_phase ends at one
cloud per frame, every surface patch once per frame that saw it; what a user registers, measures and looks at is one model.  The
reference has no code for this step; tests/fusion_restate.py is the numpy float32 statement of what is computed here, bit for bit.

    per volume   TSDFVolume: five fp32 planes of nz x ny x nx voxels on the device (tsdf, weight, colour x 3), cleared once
    per batch    volume.integrate (csrc/fusion.hip, two launches whatever the batch size): the per-frame table, then every voxel
                 against every frame of the batch in order; a wave whose box of voxels no frame can see loads and stores nothing;
                 one read of the per-frame flags
    at the end   volume.extract (three launches): the surface points on the grid's edges as (P, 6) rows of x, y, z, r, g, b, which
                 registration.register and utils.write_point_cloud take as they are; one 8-byte read of the count in between;
                 or volume.extract_mesh (csrc/fusion_mesh.hip, four launches): the same rows as vertices, a unit normal per row and
                 the (T, 3) faces of marching cubes, which utils.write_mesh takes; tests/fusion_mesh_restate.py states them
    at any time  volume.render (csrc/fusion_render.hip, two launches whatever the batch, no read): the volume seen from posed cameras,
                 a ray per pixel to the first zero crossing of the trilinear tsdf: depth, mask, colours and normals on the device;
                 tests/fusion_render_restate.py states them
    at any time  volume.residuals / volume.track (csrc/fusion_track.hip, two launches per call whatever the batch, one read of 40
                 doubles per frame): each predicted pixel's signed distance to the model under its frame's scale and pose, and
                 Gauss-Newton on those distances over a similarity per frame, solved on the host; tests/fusion_track_restate.py
                 states them

Depth maps, masks, colour images, intrinsics and poses are the ones evaluate.posed_outputs_from_predictions takes and returns: a pose
maps scaled camera coordinates to the tracker's frame, ``x = R (s x_cam) + t``, and without explicit scales ``s`` is the posed
output's own 20 / (z_max - z_min), so the fused surface lies on the posed clouds.
"""

import ctypes
import math

import numpy as np
import torch

from . import _lib

FLAGS = ("ok", "empty", "zero_range", "bad_scale")          # ENDO_FUSION_FRAME_* of include/endo_hip.h
NO_CULL = 1                                                 # ENDO_FUSION_NO_CULL
NO_SKIP = 2                                                 # ENDO_FUSION_NO_SKIP
TRACK_SUMS = 40                                             # endo_fusion_track's doubles per frame


def __getattr__(name):
    # the box of voxels one wave of the integrate kernel owns, asked of the library itself (tests take their edge sizes from here)
    if name == "WAVE_BOX":
        lib = _lib.load()
        return tuple(int(lib.endo_fusion_tile(which)) for which in range(3))
    # the render kernel's: the pixel tile of one wave (x, y), and the cells of a brick of the empty-space marks (x, y, z)
    if name in ("RENDER_TILE", "RENDER_BRICK"):
        lib = _lib.load()
        return tuple(int(lib.endo_fusion_render_tile(which)) for which in (range(2) if name == "RENDER_TILE" else range(2, 5)))
    # the track kernel's: the pixel tile of one block (x, y) and the consecutive tiles of a frame a block walks
    if name == "TRACK_TILE":
        lib = _lib.load()
        return tuple(int(lib.endo_fusion_track_tile(which)) for which in range(3))
    raise AttributeError(name)


def _host_doubles(values):
    values = [float(v) for v in values]
    return (ctypes.c_double * len(values))(*values)


def _device_tensor(t, dtype, shape, name):
    if not torch.is_tensor(t):
        raise ValueError("%s must be a device tensor of shape %s" % (name, tuple(shape)))
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: the MI355X path has no CPU fallback" % name)
    if t.dtype != dtype or int(t.numel()) != int(np.prod(shape)):
        raise ValueError("%s must be a %s tensor of shape %s, not %s of %s" % (
            name, str(dtype).replace("torch.", ""), tuple(shape), str(t.dtype).replace("torch.", ""), tuple(t.shape)))
    return t.contiguous()


def _poses(rotations, translations, n, dev):
    from . import evaluate          # (evaluate imports this module)
    return evaluate._poses_f64(rotations, translations, n, dev)


def _track_rms(sums):
    return math.sqrt(float(sums[1] / sums[0])) if sums[0] > 0 else float("nan")


def rodrigues(omega):
    """exp([omega]x) in fp64: the rotation about ``omega`` by its length in radians."""
    omega = np.asarray(omega, np.float64).reshape(3)
    angle = float(np.linalg.norm(omega))
    k = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if angle < 1.0e-12:
        return np.eye(3) + k
    return np.eye(3) + (math.sin(angle) / angle) * k + ((1.0 - math.cos(angle)) / (angle * angle)) * (k @ k)


def gauss_newton_step(sums, with_scale=True, damping=0.0):
    """One frame's 40 sums of endo_fusion_track to its step (omega, tau, sigma), 7 fp64 numbers (sigma 0 without the scale): the
    solution of ``(JtJ + damping diag(JtJ)) delta = -Jt r`` through a Cholesky factorisation; None where that fails (a system that is
    not positive definite, or not finite)."""
    m = 7 if with_scale else 6
    full = np.zeros((7, 7))
    full[np.triu_indices(7)] = np.asarray(sums, np.float64)[12:40]
    full = full + np.triu(full, 1).T
    a, b = full[:m, :m], np.asarray(sums, np.float64)[5:5 + m]
    a = a + float(damping) * np.diag(np.diag(a))
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return None
    try:
        lower = np.linalg.cholesky(a)
    except np.linalg.LinAlgError:
        return None
    delta = np.zeros(7)
    delta[:m] = -np.linalg.solve(lower.T, np.linalg.solve(lower, b))
    return delta if np.isfinite(delta).all() else None


class Tracking(object):
    """One frame's result of TSDFVolume.track: rotation (3 x 3), translation and scale of the refined pose ``x = R (s x_cam) + t`` (the
    input's for a frame that failed); status, "ok", "bad_scale", "too_few" or "singular"; iterations (the steps taken), converged;
    count and rms of the signed distances under the returned pose; initial_rms (under the input pose) and history (the rms of every
    iteration, before its update)."""

    def __init__(self, rotation, translation, scale, iterations, converged, status, count, rms, initial_rms, history):
        self.rotation, self.translation, self.scale = np.array(rotation, np.float64), np.array(translation, np.float64), float(scale)
        self.iterations, self.converged, self.status = int(iterations), bool(converged), str(status)
        self.count, self.rms, self.initial_rms, self.history = int(count), float(rms), float(initial_rms), list(history)

    def __repr__(self):
        return "Tracking(status=%s, scale=%.6g, count=%d, rms=%.6g, iterations=%d, converged=%s)" % (
            self.status, self.scale, self.count, self.rms, self.iterations, self.converged)


class TSDFVolume(object):
    """A voxel grid in the tracker's frame.  origin: the corner of voxel (0, 0, 0) (its centre is half a voxel further on every
    axis); voxel_size: the edge of a voxel; dims: (nx, ny, nz) with nx a multiple of 4; truncation: the distance at which the signed
    distance saturates (None: 4 voxels); max_weight: the cap of a voxel's frame count, after which the average becomes a moving one.
    The planes are ``tsdf`` and ``weight`` (nz, ny, nx) and ``color`` (3, nz, ny, nx), fp32 on ``device``: tsdf 1, weight 0, colour 0
    until a frame sees the voxel."""

    def __init__(self, origin, voxel_size, dims, truncation=None, max_weight=64.0, device=None):
        origin = np.asarray(origin, np.float64).reshape(-1)
        if origin.shape[0] != 3 or not np.all(np.isfinite(origin)) or not np.all(np.isfinite(origin.astype(np.float32))):
            raise ValueError("origin must be three finite coordinates, not %r" % (origin.tolist(),))
        voxel_size = float(voxel_size)
        if not (voxel_size > 0.0 and math.isfinite(voxel_size) and float(np.float32(voxel_size)) > 0.0 and np.isfinite(np.float32(voxel_size))):
            raise ValueError("voxel_size must be positive and finite, not %r" % voxel_size)
        try:
            nx, ny, nz = (int(v) for v in dims)
        except (TypeError, ValueError):
            raise ValueError("dims must be (nx, ny, nz), not %r" % (dims,))
        if nx <= 0 or ny <= 0 or nz <= 0:
            raise ValueError("dims must be positive, not %r" % ((nx, ny, nz),))
        if nx % 4:
            raise ValueError("nx must be a multiple of 4 (a thread owns 4 consecutive x voxels), not %d" % nx)
        truncation = 4.0 * voxel_size if truncation is None else float(truncation)
        if not (truncation > 0.0 and math.isfinite(truncation)):
            raise ValueError("truncation must be positive and finite, not %r" % truncation)
        max_weight = float(max_weight)
        if not (max_weight >= 1.0 and math.isfinite(max_weight)):
            raise ValueError("max_weight must be finite and at least 1, not %r" % max_weight)
        lib = _lib.load()
        self._extract_bytes = int(lib.endo_fusion_extract_workspace_bytes(nx, ny, nz))
        if self._extract_bytes < 0:
            raise ValueError("a volume of %d x %d x %d voxels is outside endo_fusion_integrate's sizes" % (nx, ny, nz))
        self.origin, self.voxel_size, self.dims = origin, voxel_size, (nx, ny, nz)
        self.truncation, self.max_weight = truncation, max_weight
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError("a TSDFVolume lives on the GPU: the MI355X path has no CPU fallback")
        with torch.cuda.device(self.device):
            self._planes = torch.empty((5, nz, ny, nx), dtype=torch.float32, device=self.device)
        self.tsdf, self.weight, self.color = self._planes[0], self._planes[1], self._planes[2:5]
        self.device = self._planes.device
        self.clear()

    @classmethod
    def around(cls, points, voxel_size=None, resolution=256, margin_voxels=8, **kw):
        """A volume around the bounding box of (P, >= 3) device rows of x, y, z, ...: the box's longest side divided into ``resolution``
        voxels (or voxels of ``voxel_size``), ``margin_voxels`` more on every side, nx rounded up to a multiple of 4.  One read of the
        six bounds."""
        if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] < 3:
            raise ValueError("points must be (P, C) device rows of x, y, z, ... with C >= 3")
        if not points.is_cuda:
            raise RuntimeError("points must live on the GPU: the MI355X path has no CPU fallback")
        if points.shape[0] == 0:
            raise ValueError("points is empty: there is no bounding box")
        xyz = points[:, :3].float()
        bounds = torch.stack([xyz.amin(dim=0), xyz.amax(dim=0)]).to(torch.float64).cpu().numpy()
        return cls.around_bounds(bounds[0], bounds[1], voxel_size, resolution, margin_voxels, device=points.device, **kw)

    @classmethod
    def around_bounds(cls, low, high, voxel_size=None, resolution=256, margin_voxels=8, truncation_voxels=None, **kw):
        """around() from the box's corners as host numbers.  truncation_voxels: the truncation in voxels of the size found here."""
        low, high = np.asarray(low, np.float64).reshape(3), np.asarray(high, np.float64).reshape(3)
        if not (np.all(np.isfinite(low)) and np.all(np.isfinite(high))) or np.any(high < low):
            raise ValueError("the bounding box %r .. %r is not finite" % (low.tolist(), high.tolist()))
        margin = int(margin_voxels)
        if margin < 0:
            raise ValueError("margin_voxels must not be negative")
        if voxel_size is None:
            if int(resolution) <= 0:
                raise ValueError("resolution must be positive, not %r" % resolution)
            voxel_size = float((high - low).max()) / int(resolution)
            if not voxel_size > 0.0:
                raise ValueError("the bounding box has no extent: give voxel_size")
        voxel_size = float(voxel_size)
        if not (voxel_size > 0.0 and math.isfinite(voxel_size)):
            raise ValueError("voxel_size must be positive and finite, not %r" % voxel_size)
        dims = [int(math.ceil(float(side) / voxel_size)) + 1 + 2 * margin for side in (high - low)]
        dims[0] = (dims[0] + 3) // 4 * 4
        if truncation_voxels is not None:
            kw["truncation"] = float(truncation_voxels) * voxel_size
        return cls(low - margin * voxel_size, voxel_size, dims, **kw)

    def clear(self):
        """tsdf 1, weight 0, colour 0 (endo_fusion_clear)."""
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().endo_fusion_clear(nx, ny, nz, _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color),
                                                     _lib.stream()), "endo_fusion_clear")

    def integrate(self, depth, boundaries, colors_u8, intrinsics, rotations, translations, scales=None, cull=True):
        """endo_fusion_integrate on a batch of N frames, in order: depth and boundaries (N, 1, H, W) or (N, H, W) fp32, colors_u8
        (N, H, W, 3) uint8, intrinsics (N, 3, 3) fp32, as evaluate.posed_outputs_from_predictions takes and returns them (its
        ``depth``, its ``boundaries`` argument, its ``color_images``); rotations (N, 3, 3) and translations (N, 3) as it takes them.
        scales: N per-frame scales (a tensor or an array), or None for the posed output's own 20 / (z_max - z_min).  cull=False
        integrates without the per-wave visibility test: same bytes, more traffic.  Returns the host list of N flags -- "ok",
        "empty" (no pixel inside the mask), "zero_range" (equal kept depths under the default scale), "bad_scale" (a scale that is
        not finite and positive) -- the call's one read back; only "ok" frames touch the volume."""
        if not torch.is_tensor(depth) or depth.dim() not in (3, 4):
            raise ValueError("depth must be an (N, 1, H, W) or (N, H, W) device tensor")
        n, height, width = int(depth.shape[0]), int(depth.shape[-2]), int(depth.shape[-1])
        depth = _device_tensor(depth, torch.float32, (n, height, width), "depth")
        boundaries = _device_tensor(boundaries, torch.float32, (n, height, width), "boundaries")
        colors_u8 = _device_tensor(colors_u8, torch.uint8, (n, height, width, 3), "colors_u8")
        intrinsics = _device_tensor(intrinsics, torch.float32, (n, 3, 3), "intrinsics")
        for name, t in (("depth", depth), ("boundaries", boundaries), ("colors_u8", colors_u8), ("intrinsics", intrinsics)):
            if t.device != self.device:
                raise ValueError("%s lives on %s, the volume on %s" % (name, t.device, self.device))
        lib = _lib.load()
        need = int(lib.endo_fusion_workspace_bytes(n, height, width))
        if need < 0:
            raise ValueError("a batch of %d frames of %d x %d is outside endo_fusion_integrate's sizes" % (n, height, width))
        rotations, translations = _poses(rotations, translations, n, self.device)
        if scales is not None:
            if not torch.is_tensor(scales):
                scales = torch.from_numpy(np.ascontiguousarray(np.asarray(scales, np.float32).reshape(-1)))
            if int(scales.numel()) != n:
                raise ValueError("scales must hold one value per frame: %d, not %d" % (n, int(scales.numel())))
            scales = scales.detach().to(device=self.device, dtype=torch.float32).reshape(n).contiguous()
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            flags = torch.empty(n, dtype=torch.int32, device=self.device)
            _lib.check(lib.endo_fusion_integrate(_lib.ptr(depth), _lib.ptr(boundaries), _lib.ptr(colors_u8), _lib.ptr(intrinsics),
                                                 _lib.ptr(rotations), _lib.ptr(translations), _lib.ptr(scales), n, height, width,
                                                 _host_doubles(self.origin), self.voxel_size, self.truncation, self.max_weight, nx, ny,
                                                 nz, _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color), _lib.ptr(flags),
                                                 0 if cull else NO_CULL, _lib.ptr(workspace), need, _lib.stream()),
                       "endo_fusion_integrate")
            host = flags.cpu().tolist()          # the call's one read back (it waits for the stream)
        return [FLAGS[v] for v in host]

    def extract(self, min_weight=1.0):
        """The surface as a (P, 6) fp32 device tensor of x, y, z, r, g, b: one row per grid edge whose two voxels both have
        weight >= min_weight and signed distances of different sign, at the linear zero crossing, coloured by the same interpolation;
        voxels in (k, j, i) order, the edges +x, +y, +z inside a voxel.  P = 0 is a valid result."""
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError("min_weight is NaN")
        lib = _lib.load()
        nx, ny, nz = self.dims
        origin = _host_doubles(self.origin)
        with torch.cuda.device(self.device):
            workspace = torch.empty(self._extract_bytes, dtype=torch.uint8, device=self.device)
            total = torch.empty(2, dtype=torch.int64, device=self.device)
            _lib.check(lib.endo_fusion_count(origin, self.voxel_size, nx, ny, nz, _lib.ptr(self.tsdf), _lib.ptr(self.weight),
                                             _lib.ptr(self.color), min_weight, _lib.ptr(total), _lib.ptr(workspace), self._extract_bytes,
                                             _lib.stream()), "endo_fusion_count")
            count = int(total[1:].cpu()[0])          # the one 8-byte read between the scan and the write pass
            rows = torch.empty((count, 6), dtype=torch.float32, device=self.device)
            _lib.check(lib.endo_fusion_extract(origin, self.voxel_size, nx, ny, nz, _lib.ptr(self.tsdf), _lib.ptr(self.weight),
                                               _lib.ptr(self.color), min_weight, _lib.ptr(rows) if count else None, count,
                                               _lib.ptr(total), _lib.ptr(workspace), self._extract_bytes, _lib.stream()),
                       "endo_fusion_extract")
        return rows

    def extract_mesh(self, min_weight=1.0):
        """The surface as a triangle mesh (csrc/fusion_mesh.hip, four launches): ``(vertices, normals, faces)`` on the device.
        vertices (P, 6) fp32: the rows of ``extract(min_weight)``, byte for byte.  normals (P, 3) fp32: the unit gradient of the signed
        distance at each row, from the surface towards the cameras; (0, 0, 0) where the gradient vanishes.  faces (T, 3) int32: the
        rows of each triangle, counter-clockwise as seen from outside; marching cubes over the cells whose eight voxels all have
        weight >= min_weight, cells in (k, j, i) order.  A row on the rim of the observed part that no such cell touches stays
        unreferenced.  One 32-byte read of the two counts between the count and the write launches; P = 0 or T = 0 is valid."""
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError("min_weight is NaN")
        lib = _lib.load()
        nx, ny, nz = self.dims
        origin = _host_doubles(self.origin)
        need = int(lib.endo_fusion_mesh_workspace_bytes(nx, ny, nz))
        with torch.cuda.device(self.device):
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            totals = torch.empty(4, dtype=torch.int64, device=self.device)
            volume = (origin, self.voxel_size, nx, ny, nz, _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color), min_weight)
            state = (_lib.ptr(totals), _lib.ptr(workspace), need, _lib.stream())
            _lib.check(lib.endo_fusion_mesh_count(*(volume + state)), "endo_fusion_mesh_count")
            _, points, _, triangles = totals.cpu().tolist()          # the one read between the scan and the write launches
            if max(points, triangles) > 2 ** 31 - 1:
                raise ValueError("a mesh of %d vertices and %d triangles does not fit int32 faces: extract a smaller volume" % (points, triangles))
            vertices = torch.empty((points, 6), dtype=torch.float32, device=self.device)
            normals = torch.empty((points, 3), dtype=torch.float32, device=self.device)
            faces = torch.empty((triangles, 3), dtype=torch.int32, device=self.device)
            _lib.check(lib.endo_fusion_mesh_vertices(*(volume + (_lib.ptr(vertices) if points else None, _lib.ptr(normals) if points else None,
                                                                 points) + state)), "endo_fusion_mesh_vertices")
            _lib.check(lib.endo_fusion_mesh_faces(*(volume + (_lib.ptr(faces) if triangles else None, triangles) + state)),
                       "endo_fusion_mesh_faces")
        return vertices, normals, faces

    def render(self, intrinsics, rotations, translations, height, width, scales=None, boundaries=None, min_weight=1.0, step=0.5, skip=True):
        """The volume seen by N posed cameras (csrc/fusion_render.hip, two launches whatever N is, no read back): one ray per pixel,
        sampled every ``step`` voxels of distance, to the first zero crossing of the trilinear tsdf between two samples whose eight
        voxels all have weight >= min_weight (extract_mesh's cell rule).  intrinsics (N, 3, 3) fp32 on the device; rotations
        (N, 3, 3) and translations (N, 3) as integrate takes them; scales: N per-frame scales or None for ones -- with a frame's own
        scale the depth is in the units of that frame's prediction; boundaries (N, 1, H, W) or (N, H, W) fp32 or None: a pixel that is
        not > 0.5 casts no ray.  0 < step <= truncation / voxel_size.  skip=False marches without the empty-space marks: same bytes,
        more traffic.  Returns a dictionary of device tensors, all 0 where a ray meets no surface: ``depth`` and ``mask`` (N, 1, H, W)
        fp32, ``colors`` (N, H, W, 3) uint8 in the byte order integrate took, ``normals`` (N, H, W, 3) fp32 unit vectors in the
        tracker's frame, from the surface towards free space.  tests/fusion_render_restate.py states all four, bit for bit."""
        n, height, width = (int(intrinsics.shape[0]) if torch.is_tensor(intrinsics) and intrinsics.dim() == 3 else 0), int(height), int(width)
        min_weight, step = float(min_weight), float(step)
        if math.isnan(min_weight):
            raise ValueError("min_weight is NaN")
        if not (step > 0.0 and float(np.float32(step) * np.float32(self.voxel_size)) <= float(np.float32(self.truncation))):
            raise ValueError("step must be positive and at most truncation / voxel_size = %g voxels, not %r" % (
                self.truncation / self.voxel_size, step))
        if n <= 0:
            raise ValueError("intrinsics must be an (N, 3, 3) device tensor")
        intrinsics = _device_tensor(intrinsics, torch.float32, (n, 3, 3), "intrinsics")
        if boundaries is not None:
            boundaries = _device_tensor(boundaries, torch.float32, (n, height, width), "boundaries")
        for name, t in (("intrinsics", intrinsics), ("boundaries", boundaries)):
            if t is not None and t.device != self.device:
                raise ValueError("%s lives on %s, the volume on %s" % (name, t.device, self.device))
        lib = _lib.load()
        nx, ny, nz = self.dims
        need = int(lib.endo_fusion_render_workspace_bytes(n, height, width, nx, ny, nz))
        if need < 0:
            raise ValueError("%d frames of %d x %d from %d x %d x %d voxels are outside endo_fusion_render's sizes" % (n, height, width, nx, ny, nz))
        rotations, translations = _poses(rotations, translations, n, self.device)
        if scales is not None:
            if not torch.is_tensor(scales):
                scales = torch.from_numpy(np.ascontiguousarray(np.asarray(scales, np.float32).reshape(-1)))
            if int(scales.numel()) != n:
                raise ValueError("scales must hold one value per frame: %d, not %d" % (n, int(scales.numel())))
            scales = scales.detach().to(device=self.device, dtype=torch.float32).reshape(n).contiguous()
        with torch.cuda.device(self.device):
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            out = {"depth": torch.empty((n, 1, height, width), dtype=torch.float32, device=self.device),
                   "mask": torch.empty((n, 1, height, width), dtype=torch.float32, device=self.device),
                   "colors": torch.empty((n, height, width, 3), dtype=torch.uint8, device=self.device),
                   "normals": torch.empty((n, height, width, 3), dtype=torch.float32, device=self.device)}
            _lib.check(lib.endo_fusion_render(_host_doubles(self.origin), self.voxel_size, self.truncation, nx, ny, nz, _lib.ptr(self.tsdf),
                                              _lib.ptr(self.weight), _lib.ptr(self.color), _lib.ptr(intrinsics), _lib.ptr(rotations),
                                              _lib.ptr(translations), _lib.ptr(scales), _lib.ptr(boundaries), n, height, width, min_weight,
                                              step, 0 if skip else NO_SKIP, _lib.ptr(out["depth"]), _lib.ptr(out["mask"]),
                                              _lib.ptr(out["colors"]), _lib.ptr(out["normals"]), _lib.ptr(workspace), need, _lib.stream()),
                       "endo_fusion_render")
        return out

    def _track_call(self, depth, boundaries, intrinsics, n, height, width):
        """The checked device inputs of residuals and track, and one call of endo_fusion_track on them for given poses and scales."""
        depth = _device_tensor(depth, torch.float32, (n, height, width), "depth")
        boundaries = _device_tensor(boundaries, torch.float32, (n, height, width), "boundaries")
        intrinsics = _device_tensor(intrinsics, torch.float32, (n, 3, 3), "intrinsics")
        for name, t in (("depth", depth), ("boundaries", boundaries), ("intrinsics", intrinsics)):
            if t.device != self.device:
                raise ValueError("%s lives on %s, the volume on %s" % (name, t.device, self.device))
        lib = _lib.load()
        need = int(lib.endo_fusion_track_workspace_bytes(n, height, width))
        nx, ny, nz = self.dims
        if need < 0 or nx > 2 ** 24:
            raise ValueError("%d frames of %d x %d against %d x %d x %d voxels are outside endo_fusion_track's sizes" % (n, height, width, nx, ny, nz))
        origin = _host_doubles(self.origin)
        with torch.cuda.device(self.device):
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            meta = torch.empty(n * 8 * TRACK_SUMS + n * 4, dtype=torch.uint8, device=self.device)          # sums, then flags: one read
        sums, flags = meta[:n * 8 * TRACK_SUMS].view(torch.float64), meta[n * 8 * TRACK_SUMS:].view(torch.int32)

        def call(rotations, translations, scales, min_weight, per_pixel):
            rotations, translations = _poses(rotations, translations, n, self.device)
            scales = torch.from_numpy(np.ascontiguousarray(np.asarray(scales, np.float32).reshape(n))).to(self.device)
            with torch.cuda.device(self.device):
                maps = None
                if per_pixel:
                    maps = {"residual": torch.empty((n, 1, height, width), dtype=torch.float32, device=self.device),
                            "valid": torch.empty((n, 1, height, width), dtype=torch.float32, device=self.device),
                            "gradient": torch.empty((n, height, width, 3), dtype=torch.float32, device=self.device)}
                _lib.check(lib.endo_fusion_track(origin, self.voxel_size, self.truncation, nx, ny, nz, _lib.ptr(self.tsdf),
                                                 _lib.ptr(self.weight), _lib.ptr(depth), _lib.ptr(boundaries), _lib.ptr(intrinsics),
                                                 _lib.ptr(rotations), _lib.ptr(translations), _lib.ptr(scales), n, height, width,
                                                 min_weight, _lib.ptr(sums), _lib.ptr(flags), _lib.ptr(maps["residual"]) if maps else None,
                                                 _lib.ptr(maps["valid"]) if maps else None, _lib.ptr(maps["gradient"]) if maps else None,
                                                 _lib.ptr(workspace), need, _lib.stream()), "endo_fusion_track")
                host = meta.cpu().numpy()          # the call's one read back (it waits for the stream)
            return (host[:n * 8 * TRACK_SUMS].view(np.float64).reshape(n, TRACK_SUMS).copy(),
                    [FLAGS[v] for v in host[n * 8 * TRACK_SUMS:].view(np.int32)], maps)
        return call

    @staticmethod
    def _track_arguments(depth, scales, min_weight):
        if not torch.is_tensor(depth) or depth.dim() not in (3, 4):
            raise ValueError("depth must be an (N, 1, H, W) or (N, H, W) device tensor")
        n, height, width = int(depth.shape[0]), int(depth.shape[-2]), int(depth.shape[-1])
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError("min_weight is NaN")
        if scales is None:
            scales = np.ones(n, np.float64)
        else:
            scales = (scales.detach().cpu().numpy() if torch.is_tensor(scales) else np.asarray(scales)).astype(np.float64).reshape(-1)
            if scales.shape[0] != n:
                raise ValueError("scales must hold one value per frame: %d, not %d" % (n, scales.shape[0]))
        return n, height, width, scales, min_weight

    def residuals(self, depth, boundaries, intrinsics, rotations, translations, scales=None, min_weight=1.0, per_pixel=True):
        """Each predicted pixel's signed distance to the model (csrc/fusion_track.hip, two launches whatever N is, one read of the
        sums): the pixel back-projected under its frame's scale and pose, ``x = R (s d ray) + t``, and the trilinear tsdf sampled
        there, times the truncation.  depth and boundaries (N, 1, H, W) or (N, H, W) fp32 and intrinsics (N, 3, 3) fp32 on the
        device; rotations (N, 3, 3) and translations (N, 3) as integrate takes them; scales: N per-frame scales or None for ones, as
        in render.  A pixel is a sample when its boundary is > 0.5, its depth finite and positive and the eight voxels around the
        point all have weight >= min_weight (render's cell rule).  Returns a dictionary: ``residual`` and ``valid`` (N, 1, H, W) and
        ``gradient`` (N, H, W, 3), fp32 device tensors, 0 where the pixel is no sample (None with per_pixel=False): the signed
        distance, positive in free space, 1, and the distance's gradient per unit length in the tracker's frame; per frame ``sums``
        ((N, 40) numpy fp64, the layout of endo_fusion_track), ``count``, ``rms`` (NaN without a sample) and ``flags`` ("ok" or
        "bad_scale": a scale that is not finite and positive; such a frame has no sample).  tests/fusion_track_restate.py states them."""
        n, height, width, scales, min_weight = self._track_arguments(depth, scales, min_weight)
        call = self._track_call(depth, boundaries, intrinsics, n, height, width)
        sums, flags, maps = call(rotations, translations, scales, min_weight, bool(per_pixel))
        out = dict(maps) if maps else {"residual": None, "valid": None, "gradient": None}
        out.update({"sums": sums, "flags": flags, "count": [int(round(v)) for v in sums[:, 0]], "rms": [_track_rms(row) for row in sums]})
        return out

    def track(self, depth, boundaries, intrinsics, rotations, translations, scales=None, with_scale=True, iterations=20, tolerance=None,
              min_weight=1.0, min_count=64, damping=0.0):
        """Frame-to-model alignment of N frames against the volume: Gauss-Newton on the signed distances of ``residuals`` over a
        similarity per frame (rotation, translation and, with_scale, the scale: monocular depth is known up to scale), the whole batch
        in lock-step.  Each iteration is one call without per-pixel outputs, one read of N x 40 doubles and a numpy fp64 solve of
        ``(JtJ + damping diag(JtJ)) delta = -Jt r``, 7 x 7 or 6 x 6; then ``R <- exp([omega]x) R``, ``t <- t + tau``,
        ``s <- s exp(sigma)``: the increment acts in the tracker's frame about the camera centre.  A frame stops when
        ``max(|omega| rho, |tau|, |sigma| rho) <= tolerance``, rho the rms length of its samples' rays (None: 1e-3 voxel_size, two
        orders above the float32 floor of the per-pixel work and far below what the surface resolves); the others go on.  One more
        call after the last update gives the count and rms of the returned poses.  Returns a list of N Tracking.  A frame that
        fails -- "bad_scale", "too_few" (fewer than min_count samples) or "singular" (the system is not positive definite) --
        keeps its input pose and scale; nothing raises for it."""
        n, height, width, scales, min_weight = self._track_arguments(depth, scales, min_weight)
        tolerance = 1.0e-3 * self.voxel_size if tolerance is None else float(tolerance)
        call = self._track_call(depth, boundaries, intrinsics, n, height, width)
        rot, tr = _poses(rotations, translations, n, torch.device("cpu"))
        rot, tr = rot.numpy().copy(), tr.numpy().copy()
        start = (rot.copy(), tr.copy(), scales.copy())
        status, steps, converged = ["ok"] * n, [0] * n, [False] * n
        history, initial = [[] for _ in range(n)], [float("nan")] * n
        active = list(range(n))
        for it in range(int(iterations)):
            if not active:
                break
            sums, flags, _ = call(rot, tr, scales, min_weight, False)
            for f in list(active):
                rms = _track_rms(sums[f])
                history[f].append(rms)
                if it == 0:
                    initial[f] = rms
                delta = None
                if flags[f] != "ok":
                    status[f] = flags[f]
                elif sums[f, 0] < min_count:
                    status[f] = "too_few"
                else:
                    delta = gauss_newton_step(sums[f], with_scale, damping)
                    if delta is None:
                        status[f] = "singular"
                if delta is None:          # it stays where it came from
                    rot[f], tr[f], scales[f] = start[0][f], start[1][f], start[2][f]
                    active.remove(f)
                    continue
                rot[f] = rodrigues(delta[:3]) @ rot[f]
                tr[f] = tr[f] + delta[3:6]
                scales[f] = scales[f] * math.exp(delta[6])
                steps[f] += 1
                rho = math.sqrt(sums[f, 4] / sums[f, 0])
                if max(float(np.linalg.norm(delta[:3])) * rho, float(np.linalg.norm(delta[3:6])), abs(float(delta[6])) * rho) <= tolerance:
                    converged[f] = True
                    active.remove(f)
        sums, flags, _ = call(rot, tr, scales, min_weight, False)
        out = []
        for f in range(n):
            if status[f] == "ok" and flags[f] != "ok":
                status[f] = flags[f]
            if not history[f]:          # iterations = 0
                initial[f] = _track_rms(sums[f])
            out.append(Tracking(rot[f], tr[f], scales[f], steps[f], converged[f], status[f], int(round(sums[f, 0])), _track_rms(sums[f]),
                                initial[f], history[f]))
        return out

    def observed_voxels(self):
        """The number of voxels at least one frame has seen (one read)."""
        return int(torch.count_nonzero(self.weight))
