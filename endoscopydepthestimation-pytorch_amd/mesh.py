"""A triangle mesh on the device and what it looks like from posed cameras: the CT model of the reference's README, step 4, seen from
a frame -- the dense depth a prediction is measured against (evaluate.model_depth_errors).  registration.register aligns clouds to the
model's vertices and fusion.TSDFVolume.render ray-casts the project's own fused volume; this module draws a surface that comes from
elsewhere.  The reference has no code for it; tests/mesh_render_restate.py is the numpy float32 statement, bit for bit.

    per mesh    TriangleMesh: (V, 3 or 6) fp32 rows of x, y, z(, r, g, b) and (T, 3) int32 faces, uploaded once;
                TriangleMesh.from_ply reads what reader.read_mesh reads, TriangleMesh(*volume.extract_mesh()[::2]) takes the fused
                surface where it is
    per batch   mesh.render (csrc/mesh_render.hip, four launches whatever the batch, no read back): the ray through every pixel centre
                against the triangles, watertight on shared edges, the nearest hit per pixel: depth, mask, triangle, barycentric
                coordinates, face normals and, with colour columns, colours

A pose maps scaled camera coordinates to the mesh's frame, ``x = R (s x_cam) + t``, as everywhere in fusion.
"""

import numpy as np
import torch

from . import _lib, reader, registration
from .fusion import FLAGS, _device_tensor, _poses

CULL_BACK = 1          # ENDO_MESH_CULL_BACK
CULL_FRONT = 2         # ENDO_MESH_CULL_FRONT
BRUTE = 4              # ENDO_MESH_BRUTE
_CULL = {None: 0, "none": 0, "back": CULL_BACK, "front": CULL_FRONT}


def __getattr__(name):
    # the kernel's constants, asked of the library itself (tests take their edge sizes from here): the pixel tile of one wave of the
    # queue pass (x, y), the largest box in pixels the setup pass tests in place, the threads of a block
    if name == "RENDER_TILE":
        lib = _lib.load()
        return tuple(int(lib.endo_mesh_render_tile(which)) for which in range(4))
    raise AttributeError(name)


class TriangleMesh(object):
    """vertices: (V, 3) rows of x, y, z or (V, 6) rows of x, y, z, r, g, b (fusion.TSDFVolume.extract_mesh's and utils.write_mesh's
    rows), an array or a device tensor, which is used where it is; faces: (T, 3) indices into them, counter-clockwise as seen from
    outside.  A face with an index outside 0 .. V - 1 is kept and never hit.  V = 0 and T = 0 are valid."""

    def __init__(self, vertices, faces, device=None):
        if not torch.is_tensor(vertices):
            host = np.ascontiguousarray(np.asarray(vertices, np.float32))
            if host.ndim != 2:
                raise ValueError("vertices must be (V, 3) or (V, 6) rows")
            vertices = torch.from_numpy(host).to(device if device is not None else "cuda")
        if vertices.dim() != 2 or vertices.shape[1] not in (3, 6):
            raise ValueError("vertices must be (V, 3) rows of x, y, z or (V, 6) rows of x, y, z, r, g, b, not %s" % (tuple(vertices.shape),))
        if not vertices.is_cuda:
            raise RuntimeError("vertices must live on the GPU: the MI355X path has no CPU fallback")
        if not torch.is_tensor(faces):
            host = np.asarray(faces)
            if host.size and (host.min() < -2 ** 31 or host.max() > 2 ** 31 - 1):
                raise ValueError("faces must fit int32")
            faces = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32).reshape(-1, 3))).to(vertices.device)
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
            raise ValueError("faces must be (T, 3) int32 indices, not %s of %s" % (str(faces.dtype).replace("torch.", ""), tuple(faces.shape)))
        if faces.device != vertices.device:
            raise ValueError("faces live on %s, the vertices on %s" % (faces.device, vertices.device))
        self.vertices = vertices.detach().to(torch.float32).contiguous()
        self.faces = faces.detach().to(torch.int32).contiguous()
        self.device = self.vertices.device
        self.has_colors = int(self.vertices.shape[1]) >= 6

    @classmethod
    def from_ply(cls, path, device=None):
        """The mesh of a PLY file (reader.read_mesh)."""
        vertices, faces = reader.read_mesh(path)
        return cls(vertices, faces, device=device)

    def target(self):
        """The vertices as a registration.TargetModel (prepared on every call: keep it)."""
        return registration.TargetModel(self.vertices)

    def render(self, intrinsics, rotations, translations, height, width, scales=None, boundaries=None, cull=None, brute=False):
        """The mesh seen by N posed cameras (csrc/mesh_render.hip, four launches whatever N is, no read back).  intrinsics (N, 3, 3)
        fp32 on the device; rotations (N, 3, 3) and translations (N, 3) as fusion.TSDFVolume.render takes them; scales: N per-frame
        scales or None for ones -- with a frame's own scale the depth is in the units of that frame's prediction; boundaries
        (N, 1, H, W) or (N, H, W) fp32 or None: a pixel that is not > 0.5 has no hit.  cull: None, "back" (only faces whose normal
        points to the camera are hit) or "front".  brute=True tests every pixel against every triangle: same bytes, far more work.
        Returns a dictionary of device tensors, all 0 where a ray meets no triangle: ``depth`` and ``mask`` (N, 1, H, W) fp32,
        ``normals`` (N, H, W, 3) fp32 unit face normals in the mesh's frame, turned towards the camera, ``colors`` (N, H, W, 3) uint8
        in fusion.TSDFVolume.render's byte order (None for a mesh without colour columns), ``triangle`` (N, H, W) int32, the face of
        the hit, -1 without one, and ``barycentric`` (N, H, W, 3) fp32, the weights of its three corners; and ``flags``, the (N,)
        int32 device tensor of fusion.FLAGS indices ("ok" or "bad_scale": a scale that is not finite and positive renders nothing)."""
        n, height, width = (int(intrinsics.shape[0]) if torch.is_tensor(intrinsics) and intrinsics.dim() == 3 else 0), int(height), int(width)
        if cull not in _CULL:
            raise ValueError("cull is None, 'back' or 'front', not %r" % (cull,))
        if n <= 0:
            raise ValueError("intrinsics must be an (N, 3, 3) device tensor")
        intrinsics = _device_tensor(intrinsics, torch.float32, (n, 3, 3), "intrinsics")
        if boundaries is not None:
            boundaries = _device_tensor(boundaries, torch.float32, (n, height, width), "boundaries")
        for name, t in (("intrinsics", intrinsics), ("boundaries", boundaries)):
            if t is not None and t.device != self.device:
                raise ValueError("%s lives on %s, the mesh on %s" % (name, t.device, self.device))
        lib = _lib.load()
        count, triangles = int(self.vertices.shape[0]), int(self.faces.shape[0])
        need = int(lib.endo_mesh_render_workspace_bytes(n, height, width, triangles))
        if need < 0:
            raise ValueError("%d frames of %d x %d of %d triangles are outside endo_mesh_render's sizes" % (n, height, width, triangles))
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
                   "triangle": torch.empty((n, height, width), dtype=torch.int32, device=self.device),
                   "barycentric": torch.empty((n, height, width, 3), dtype=torch.float32, device=self.device),
                   "normals": torch.empty((n, height, width, 3), dtype=torch.float32, device=self.device),
                   "colors": torch.empty((n, height, width, 3), dtype=torch.uint8, device=self.device) if self.has_colors else None,
                   "flags": torch.empty(n, dtype=torch.int32, device=self.device)}
            _lib.check(lib.endo_mesh_render(_lib.ptr(self.vertices) if count else None, int(self.vertices.shape[1]), count,
                                            _lib.ptr(self.faces) if triangles else None, triangles, _lib.ptr(intrinsics),
                                            _lib.ptr(rotations), _lib.ptr(translations), _lib.ptr(scales), _lib.ptr(boundaries), n, height,
                                            width, _CULL[cull] | (BRUTE if brute else 0), _lib.ptr(out["depth"]), _lib.ptr(out["mask"]),
                                            _lib.ptr(out["triangle"]), _lib.ptr(out["barycentric"]), _lib.ptr(out["normals"]),
                                            _lib.ptr(out["colors"]), _lib.ptr(out["flags"]), _lib.ptr(workspace), need, _lib.stream()),
                       "endo_mesh_render")
        return out


def flag_names(flags):
    """The host names (fusion.FLAGS) of a render's ``flags`` tensor: one read."""
    return [FLAGS[v] for v in flags.cpu().tolist()]
