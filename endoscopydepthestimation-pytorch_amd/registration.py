"""Similarity registration (scale, rotation, translation) of a point cloud to a model by iterative closest point: the last step of the
reference's workflow.  Its README, step 4: after evaluate.py, "apply a registration algorithm that is able to estimate a similarity
transformation to register the predicted point clouds to the corresponding CT model to calculate residual errors".  The reference has
no code for it; tests/registration_restate.py is the numpy fp64 statement of what is computed here.

    per target      TargetModel: the rows uploaded once and prepared once (endo_registration_prepare: centred on their fp64 mean,
                    rounded to fp32, in the search's operand form), for every frame and iteration that follows
    per iteration   endo_registration_match (csrc/registration.hip, two launches): the nearest target row of every source row by exact
                    brute force, its distance in fp64 against the caller's rows, and 20 fp64 sums over the rows within the distance
                    cap; one read of the 20 doubles; similarity_from_sums (Umeyama's closed form, numpy fp64) on the host
    at the end      one more match, so that the residuals belong to the transform that is returned

A transform maps a source row x to ``scale * rotation @ x + translation``.
"""

import ctypes
import math

import numpy as np
import torch

from . import _lib, reader

WAVE = 64
_SUMS = 20


def _tile(which):
    return int(_lib.load().endo_registration_tile(which))


def __getattr__(name):
    # the search kernel's tile constants, asked of the library itself (tests take their edge sizes from here)
    if name == "SOURCE_TILE":
        return _tile(0)
    if name == "TARGET_TILE":
        return _tile(1)
    raise AttributeError(name)


def _transform_array(scale, rotation, translation):
    r = np.eye(3) if rotation is None else np.asarray(rotation, np.float64).reshape(3, 3)
    t = np.zeros(3) if translation is None else np.asarray(translation, np.float64).reshape(3)
    arr = np.concatenate([[float(scale)], r.reshape(9), t]).astype(np.float64)
    if not np.all(np.isfinite(arr)):
        raise ValueError("the transform must be finite")
    return arr


def _host_doubles(values):
    values = [float(v) for v in values]
    return (ctypes.c_double * len(values))(*values)


def _rows(points, name):
    """A device view of fp32 point rows and its row stride in floats: (P, C >= 3) with unit column stride, rows C or more apart."""
    if not torch.is_tensor(points):
        points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float32))).cuda()
    if points.dim() != 2 or points.shape[1] < 3:
        raise ValueError("%s must be (P, C) rows of x, y, z, ... with C >= 3" % name)
    if not points.is_cuda:
        raise RuntimeError("%s must live on the GPU: the MI355X path has no CPU fallback" % name)
    if points.dtype != torch.float32:
        points = points.float()
    if points.stride(1) != 1 or (points.shape[0] > 1 and points.stride(0) < points.shape[1]):
        points = points.contiguous()
    return points, max(int(points.stride(0)), int(points.shape[1]))


def similarity_from_sums(sums, with_scale=True, source_centre=None, target_centre=None):
    """Umeyama's closed form from the 20 sums of endo_registration_match ([0] n, [4..6] sum s, [7..9] sum t, [10] sum |s|^2, [11 + 3 i + j]
    sum t_i s_j, s and t relative to source_centre and target_centre; None: the origin), in numpy fp64.  Returns (scale, R, t) of the
    least-squares similarity ``target ~ scale * R source + t`` in the callers' coordinates, the two centres folded back in.
    with_scale=False: the rigid fit (scale 1).  det R = +1 always (the reflection guard on the SVD of the 3 x 3 cross-covariance).  Fewer than 3 rows or a source
    without extent raise ValueError naming the count."""
    sums = np.asarray(sums, np.float64).reshape(-1)
    if sums.shape[0] != _SUMS:
        raise ValueError("sums holds %d values, not 20" % sums.shape[0])
    n = sums[0]
    count = int(round(float(n))) if np.isfinite(n) else 0
    if not np.isfinite(n) or count < 3:
        raise ValueError("a similarity needs at least 3 corresponding rows; %d are within the distance cap" % count)
    mean_s = sums[4:7] / n
    mean_t = sums[7:10] / n
    var_s = sums[10] / n - float(mean_s @ mean_s)
    cov = sums[11:20].reshape(3, 3) / n - np.outer(mean_t, mean_s)
    if not np.isfinite(var_s) or var_s <= 0.0:
        raise ValueError("the %d source rows within the distance cap have no extent (sum |s - mean|^2 = 0)" % count)
    u, d, vt = np.linalg.svd(cov)
    sign = np.ones(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        sign[2] = -1.0
    rot = (u * sign) @ vt
    scale = float((d * sign).sum() / var_s) if with_scale else 1.0
    if source_centre is not None:
        mean_s = mean_s + np.asarray(source_centre, np.float64).reshape(3)
    if target_centre is not None:
        mean_t = mean_t + np.asarray(target_centre, np.float64).reshape(3)
    return scale, rot, mean_t - scale * (rot @ mean_s)


class TargetModel(object):
    """A target point set on the device, uploaded and prepared once for any number of frames and iterations.  points: (K, C >= 3) rows
    of x, y, z, ... (an array, or a device tensor, which is used where it is)."""

    def __init__(self, points, device=None):
        if not torch.is_tensor(points):
            host = np.ascontiguousarray(np.asarray(points, np.float32))
            if host.ndim != 2 or host.shape[1] < 3:
                raise ValueError("points must be (K, C) rows of x, y, z, ... with C >= 3")
            points = torch.from_numpy(host).to(device if device is not None else "cuda")
        self.points, self.stride = _rows(points, "points")
        self.count = int(self.points.shape[0])
        lib = _lib.load()
        need = int(lib.endo_registration_prepared_bytes(self.count))
        if need < 0:
            raise ValueError("a target of %d rows is outside endo_registration_prepare's sizes" % self.count)
        with torch.cuda.device(self.points.device):
            self.centre = self.points[:, :3].to(torch.float64).mean(dim=0).cpu().numpy()          # the fp64 mean: one read, once
            if not np.all(np.isfinite(self.centre)):
                raise ValueError("the target's coordinates must be finite")
            self.prepared = torch.empty(need, dtype=torch.uint8, device=self.points.device)
            _lib.check(lib.endo_registration_prepare(_lib.ptr(self.points), self.stride, self.count, _host_doubles(self.centre),
                                                     _lib.ptr(self.prepared), need, _lib.stream()), "endo_registration_prepare")

    @classmethod
    def from_ply(cls, path, device=None):
        rows = reader.read_point_cloud(path)
        return cls(np.asarray([row[:3] for row in rows], np.float64).astype(np.float32).reshape(-1, 3), device=device)


def _as_target(target):
    return target if isinstance(target, TargetModel) else TargetModel(target)


class _Matcher(object):
    """One source against one target: the buffers of endo_registration_match, allocated once for all iterations."""

    def __init__(self, source, target):
        self.target = _as_target(target)
        self.source, self.stride = _rows(source, "source")
        if self.source.device != self.target.points.device:
            raise ValueError("source and target live on different devices")
        self.count = int(self.source.shape[0])
        if self.count == 0:
            raise ValueError("the source cloud is empty")
        self.lib = _lib.load()
        self.need = int(self.lib.endo_registration_workspace_bytes(self.count, self.target.count))
        if self.need < 0:
            raise ValueError("%d source rows against %d target rows are outside endo_registration_match's sizes" % (self.count, self.target.count))
        dev = self.source.device
        with torch.cuda.device(dev):
            self.centre = self.source[:, :3].to(torch.float64).mean(dim=0).cpu().numpy()
            self.workspace = torch.empty(self.need, dtype=torch.uint8, device=dev)
            self.index = torch.empty(self.count, dtype=torch.int32, device=dev)
            self.distance = torch.empty(self.count, dtype=torch.float32, device=dev)
            self.sums = torch.empty(_SUMS, dtype=torch.float64, device=dev)
        if not np.all(np.isfinite(self.centre)):
            raise ValueError("the source's coordinates must be finite")

    def launch(self, transform, cap):
        """Queue one match on the current stream; the results are in self.index / distance / sums."""
        t = self.target
        with torch.cuda.device(self.source.device):
            _lib.check(self.lib.endo_registration_match(_lib.ptr(self.source), self.stride, self.count, _host_doubles(transform),
                                                        _lib.ptr(t.prepared), _lib.ptr(t.points), t.stride, t.count,
                                                        _host_doubles(self.centre), float(cap), _lib.ptr(self.index),
                                                        _lib.ptr(self.distance), _lib.ptr(self.sums), _lib.ptr(self.workspace), self.need,
                                                        _lib.stream()), "endo_registration_match")

    def match(self, transform, cap):
        """One match and its one read: the 20 sums as a host array."""
        self.launch(transform, cap)
        return self.sums.cpu().numpy()


def _residuals(sums):
    n = int(round(float(sums[0])))
    if n == 0:
        return 0, float("nan"), float("nan"), float("nan")
    return n, float(sums[1] / sums[0]), math.sqrt(float(sums[2] / sums[0])), float(sums[3])


def nearest_points(source, target, scale=1.0, rotation=None, translation=None, max_distance=None):
    """One match: every row of ``source`` moved by the transform, against ``target`` (a TargetModel, or rows to make one of).  Returns a
    dictionary: index (int32) and distance (fp32), device tensors of one entry per source row; count, mean, rms and max over the rows
    within max_distance (None: all), host numbers (NaN where count is 0); sums, the kernel's 20 doubles."""
    matcher = _Matcher(source, target)
    cap = float("inf") if max_distance is None else float(max_distance)
    sums = matcher.match(_transform_array(scale, rotation, translation), cap)
    n, mean, rms, peak = _residuals(sums)
    return {"index": matcher.index, "distance": matcher.distance, "count": n, "mean": mean, "rms": rms, "max": peak, "sums": sums}


class Registration(object):
    """The result of register(): scale, rotation (3 x 3) and translation of the similarity source -> target and its 4 x 4 matrix; count,
    mean, rms and max of the distances within the last cap, under that transform; iterations, converged, history (the rms of every
    iteration, before its update); index / distance, the final match's device tensors."""

    def __init__(self, scale, rotation, translation, residuals, iterations, converged, history, index, distance):
        self.scale, self.rotation, self.translation = float(scale), np.array(rotation, np.float64), np.array(translation, np.float64)
        self.matrix = np.eye(4)
        self.matrix[:3, :3] = self.scale * self.rotation
        self.matrix[:3, 3] = self.translation
        self.count, self.mean, self.rms, self.max = residuals
        self.iterations, self.converged, self.history = int(iterations), bool(converged), list(history)
        self.index, self.distance = index, distance

    def transform_array(self):
        return _transform_array(self.scale, self.rotation, self.translation)

    def __repr__(self):
        return "Registration(scale=%.6g, count=%d, rms=%.6g, iterations=%d, converged=%s)" % (
            self.scale, self.count, self.rms, self.iterations, self.converged)


def register(source, target, scale=1.0, rotation=None, translation=None, with_scale=True, iterations=50, tolerance=1e-9, max_distance=None,
             reject_factor=3.0):
    """Iterative closest point from the given start.  Each iteration: one match under the current distance cap (max_distance at first),
    one read of the 20 sums, similarity_from_sums on them, the next cap ``min(max_distance, reject_factor * this iteration's rms)``
    (reject_factor=None: max_distance throughout), and the stop test ``|rms_prev - rms| <= tolerance * rms``.  One more match after the
    last update gives the residuals of the returned transform.  A match that keeps fewer than 3 rows raises ValueError."""
    matcher = _Matcher(source, target)
    top = float("inf") if max_distance is None else float(max_distance)
    cap = top
    transform = _transform_array(scale, rotation, translation)
    history, converged, previous = [], False, None
    for _ in range(int(iterations)):
        sums = matcher.match(transform, cap)
        s, rot, t = similarity_from_sums(sums, with_scale, matcher.centre, matcher.target.centre)
        rms = math.sqrt(float(sums[2] / sums[0]))
        history.append(rms)
        transform = _transform_array(s, rot, t)
        if reject_factor is not None:
            cap = min(top, float(reject_factor) * rms)
        if previous is not None and abs(previous - rms) <= float(tolerance) * rms:
            converged = True
            break
        previous = rms
    sums = matcher.match(transform, cap)
    if int(round(float(sums[0]))) < 3:
        raise ValueError("a similarity needs at least 3 corresponding rows; %d are within the distance cap" % int(round(float(sums[0]))))
    return Registration(transform[0], transform[1:10].reshape(3, 3), transform[10:13], _residuals(sums), len(history), converged, history,
                        matcher.index, matcher.distance)


def similarity_apply(rows, scale=1.0, rotation=None, translation=None, out=None):
    """endo_similarity_apply: the rows' x, y, z moved by the transform in fp64 and rounded to fp32, the other columns copied.  rows:
    (P, C >= 3) fp32 on the device; returns a tensor of the same shape (``out``, when given: contiguous, same shape; it may be rows)."""
    rows, stride = _rows(rows, "rows")
    if stride != rows.shape[1]:          # the kernel copies whole rows: no columns the caller did not hand over
        rows, stride = rows.contiguous(), int(rows.shape[1])
    if out is None:
        with torch.cuda.device(rows.device):
            out = torch.empty((rows.shape[0], stride), dtype=torch.float32, device=rows.device)[:, :rows.shape[1]]
    elif out.shape != rows.shape or out.dtype != torch.float32 or out.device != rows.device or (
            out.shape[0] > 1 and (out.stride(1) != 1 or out.stride(0) != stride)):
        raise ValueError("out must be float32 rows of the shape and row stride of the input")
    if rows.shape[0]:
        with torch.cuda.device(rows.device):
            _lib.check(_lib.load().endo_similarity_apply(_lib.ptr(rows), stride, int(rows.shape[0]),
                                                         _host_doubles(_transform_array(scale, rotation, translation)), _lib.ptr(out),
                                                         _lib.stream()), "endo_similarity_apply")
    return out
