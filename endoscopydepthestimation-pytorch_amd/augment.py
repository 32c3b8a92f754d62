"""Training-phase image augmentations on the device -- the reference's albumentations pipeline (train.py:121-142), applied to
each frame of a pair with its own draws (dataset.py:432-447) before Normalize(0.5, 0.5).

Restated from **albumentations 0.4.6** (the last line that has ``IAAAdditiveGaussianNoise``, which ties the reference to < 1.0):

    Compose(p=1) of three OneOf blocks, each applied with p = 0.5.  OneOf picks one child with probabilities proportional to the
    children's own p (OneOf.__init__ normalises them) and calls it with force_apply, which a nested Compose passes on.
    colour    Compose(RandomBrightnessContrast(0.3, 0.3), RandomGamma((80, 120)), HueSaturationValue(30, 0, 0))   -- all three;
              weight 1.0, Compose's default p
              | HueSaturationValue(30, 30, 30)                                                                   -- weight 0.5
              so 2/3 : 1/3 given the block applies, 1/3 and 1/6 of all frames
    quality   Blur(7) | MedianBlur(7) | MotionBlur(7) | JpegCompression(20, 100)        -- all p = 0.5: uniform; ksize in {3, 5, 7}
    noise     GaussNoise(var_limit=(10, 30)) | IAAAdditiveGaussianNoise(scale=(0.005 * 255, 0.02 * 255), per_channel=False)   -- uniform

The draws happen on the host (``TrainingAugmentation.sample``, a seeded ``random.Random``: the same distributions as albumentations,
not its RNG stream); the pixels never leave the device: ``apply`` hands one record per frame (include/endo_hip.h,
``endo_augment_frame``) to csrc/augment.hip, which runs a batch through a fixed five launches whatever the frames drew.

Arithmetic on uint8, as 0.4.6 / OpenCV / libjpeg-turbo do it (tests/augment_restate.py states each in numpy):
  * brightness-contrast: float32 LUT ``arange(256) * alpha + beta * 255``, clipped, truncated; gamma: float64 LUT
    ``arange(0, 256/255, 1/255) ** gamma * 255`` truncated -- composed into one LUT;
  * hue-saturation-value: cv2.COLOR_RGB2HSV (8 bit, hue in [0, 180)), LUTs ``mod(i + dh, 180)``, ``clip(i + ds)``, ``clip(i + dv)``
    truncated, cv2.COLOR_HSV2RGB (float) -- OpenCV's scalar paths, PARITY UNPINNED against cv2 itself;
  * blur: k x k box, BORDER_REFLECT_101, rounded; median: BORDER_REPLICATE; motion: the 8-connected line of cv2.line over a
    k x k mask, mean of its taps rounded half to even, BORDER_REFLECT_101 (cv2.filter2D's float path may differ by 1 at exact ties,
    and cv2.line's rasterisation is restated: both unpinned);
  * JPEG: cv2.imencode / imdecode of the RGB array read as B, G, R (IJG-scaled Annex K tables, force_baseline, 4:2:0) -- bit-identical
    to libjpeg-turbo (tests/golden/augment_jpeg.npz);
  * noise: GaussNoise ``clip(float(v) + n, 0, 255)`` truncated, n ~ N(0, var) per pixel and channel; additive
    ``clip(round_half_even(v + n), 0, 255)``, n ~ N(0, scale^2) once per pixel.  Normals from Philox4x32-10 keyed by (seed, frame,
    pixel): the same plan gives the same bytes whatever the batch size or launch geometry.
"""

import ctypes
import math
import random

import numpy as np
import torch

from . import _lib

COLOUR_OPS = ("brightness_contrast_gamma_hue", "hue_saturation_value")
QUALITY_OPS = ("blur", "median_blur", "motion_blur", "jpeg_compression")
NOISE_OPS = ("gauss_noise", "additive_gaussian_noise")
KSIZES = (3, 5, 7)

FRAME_DTYPE = np.dtype([("colour", "<i4"), ("spatial", "<i4"), ("ksize", "<i4"), ("jpeg", "<i4"), ("noise", "<i4"), ("sigma", "<f4"),
                        ("seed", "<u4", (2,)), ("motion", "<u4", (2,)), ("reserved", "<i4", (6,)), ("rgb_lut", "u1", (256,)),
                        ("hsv_lut", "u1", (3, 256)), ("quant", "<u2", (2, 64))])
_SPATIAL_CODE = {"blur": 1, "median_blur": 2, "motion_blur": 3}
_NOISE_CODE = {"gauss_noise": 1, "additive_gaussian_noise": 2}

# ITU T.81 Annex K tables (natural order), jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl
_STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
_STD_CHROMA = np.full(64, 99, dtype=np.int64)
_STD_CHROMA[[0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 24, 25]] = [17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 47, 66]


# ---------------------------------------------------------------------------------------------
# host-side tables
# ---------------------------------------------------------------------------------------------
def identity_lut():
    return np.arange(256, dtype=np.uint8)


def brightness_contrast_lut(alpha, beta):
    """albumentations 0.4.6 _brightness_contrast_adjust_uint, beta_by_max=True: float32 arange * alpha + beta * 255, clip, truncate."""
    lut = np.arange(256).astype(np.float32)
    if alpha != 1:
        lut *= np.float32(alpha)
    if beta != 0:
        lut += np.float32(beta * 255)
    return np.clip(lut, 0, 255).astype(np.uint8)


def gamma_lut(gamma):
    """albumentations 0.4.6 gamma_transform on uint8: (arange(0, 256/255, 1/255) ** gamma * 255).astype(uint8), float64."""
    return (np.arange(0, 256.0 / 255, 1.0 / 255) ** gamma * 255).astype(np.uint8)


def hsv_luts(hue_shift, sat_shift, val_shift):
    """albumentations 0.4.6 _shift_hsv_uint8: (3, 256) uint8 LUTs for H (mod 180), S and V (clipped), truncated."""
    i = np.arange(256, dtype=np.int16)
    return np.stack([np.mod(i + hue_shift, 180).astype(np.uint8), np.clip(i + sat_shift, 0, 255).astype(np.uint8),
                     np.clip(i + val_shift, 0, 255).astype(np.uint8)])


def jpeg_quant_tables(quality):
    """(2, 64) uint16, natural order: jcparam.c jpeg_set_quality(quality, force_baseline=TRUE) -- the IJG scaling of the Annex K
    tables, every entry clamped to [1, 255]."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("JPEG quality must lie in [1, 100]")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (_STD_LUMA, _STD_CHROMA)]).astype(np.uint16)


def line_mask(ksize, xs, ys, xe, ye):
    """k x k uint8 0/1 mask of cv2.line(mask, (xs, ys), (xe, ye), 1, thickness=1): OpenCV's 8-connected LineIterator (Bresenham:
    the major axis advances every step, the minor one when the error term is negative), restated -- unpinned against cv2.  cv2.line
    builds its iterator with leftToRight = true, so the segment is walked from its left end: swapping the endpoints gives the same mask."""
    mask = np.zeros((ksize, ksize), np.uint8)
    if xe < xs:
        xs, ys, xe, ye = xe, ye, xs, ys
    dx, dy = xe - xs, ye - ys
    sx, sy = (1 if dx >= 0 else -1), (1 if dy >= 0 else -1)
    dx, dy = abs(dx), abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err = major - 2 * minor
    x, y = xs, ys
    for _ in range(major + 1):
        mask[y, x] = 1
        if err < 0:
            err += 2 * major - 2 * minor
            x += sx
            y += sy
        else:
            err -= 2 * minor
            if steep:
                y += sy
            else:
                x += sx
    return mask


# ---------------------------------------------------------------------------------------------
# plans: one dictionary per frame, {"colour": None | {...}, "quality": None | {...}, "noise": None | {...}}
# ---------------------------------------------------------------------------------------------
class TrainingAugmentation(object):
    """The reference's training transform (train.py:121-142).  ``sample(frames)`` draws the per-frame plans from this object's own
    generator (seeded by `seed`), ``apply(imgs_u8, plan)`` runs them on a device uint8 (F, H, W, 3) RGB batch, ``__call__`` does both.
    ``last_plan`` is the plan of the latest call."""

    def __init__(self, seed=None):
        self.rng = random.Random(seed)
        self.last_plan = None
        self._params = _Params()

    def _frame(self):
        rng = self.rng
        plan = {"colour": None, "quality": None, "noise": None}
        if rng.random() < 0.5:
            # OneOf weights = the children's p: the nested Compose has p = 1.0, HueSaturationValue p = 0.5 -> 2/3 : 1/3
            if rng.random() < 2.0 / 3.0:          # RandomBrightnessContrast -> RandomGamma -> HueSaturationValue(30, 0, 0)
                plan["colour"] = {"op": COLOUR_OPS[0], "alpha": 1.0 + rng.uniform(-0.3, 0.3), "beta": rng.uniform(-0.3, 0.3),
                                  "gamma": rng.randint(80, 120) / 100.0, "hue": rng.uniform(-30, 30), "sat": 0.0, "val": 0.0}
            else:
                plan["colour"] = {"op": COLOUR_OPS[1], "hue": rng.uniform(-30, 30), "sat": rng.uniform(-30, 30), "val": rng.uniform(-30, 30)}
        if rng.random() < 0.5:
            op = QUALITY_OPS[rng.randrange(4)]
            if op == "jpeg_compression":
                plan["quality"] = {"op": op, "quality": rng.randint(20, 100)}
            else:
                k = rng.choice(KSIZES)
                plan["quality"] = {"op": op, "ksize": k}
                if op == "motion_blur":          # albumentations 0.4.6 MotionBlur.get_params
                    xs, xe = rng.randint(0, k - 1), rng.randint(0, k - 1)
                    if xs == xe:
                        ys, ye = rng.sample(range(k), 2)
                    else:
                        ys, ye = rng.randint(0, k - 1), rng.randint(0, k - 1)
                    plan["quality"]["kernel"] = line_mask(k, xs, ys, xe, ye)
        if rng.random() < 0.5:
            op = NOISE_OPS[rng.randrange(2)]
            sigma = math.sqrt(rng.uniform(10, 30)) if op == "gauss_noise" else rng.uniform(0.005 * 255, 0.02 * 255)
            plan["noise"] = {"op": op, "sigma": sigma, "seed": rng.getrandbits(64)}
        return plan

    def sample(self, frames):
        return [self._frame() for _ in range(int(frames))]

    def apply(self, imgs_u8, plan, out_f32=None, out_u8=None):
        return apply_plan(imgs_u8, plan, out_f32=out_f32, out_u8=out_u8, params=self._params)

    def __call__(self, imgs_u8, out_f32=None, out_u8=None):
        plan = self.sample(imgs_u8.shape[0])
        self.last_plan = plan
        return self.apply(imgs_u8, plan, out_f32=out_f32, out_u8=out_u8)


def plan_records(plan):
    """The endo_augment_frame records of a plan (numpy structured array, FRAME_DTYPE)."""
    rec = np.zeros(len(plan), dtype=FRAME_DTYPE)
    for f, p in enumerate(plan):
        r = rec[f]
        r["rgb_lut"] = identity_lut()
        r["hsv_lut"] = hsv_luts(0, 0, 0)
        r["quant"] = 1
        c = p.get("colour")
        if c is not None:
            colour = 0
            lut = identity_lut()
            if c.get("alpha") is not None or c.get("beta") is not None:
                lut = brightness_contrast_lut(c.get("alpha", 1.0), c.get("beta", 0.0))
                colour |= 1
            if c.get("gamma") is not None:
                lut = gamma_lut(c["gamma"])[lut]
                colour |= 1
            if c.get("hue") is not None:
                r["hsv_lut"] = hsv_luts(c["hue"], c.get("sat", 0.0), c.get("val", 0.0))
                colour |= 2
            r["rgb_lut"] = lut
            r["colour"] = colour
        q = p.get("quality")
        if q is not None:
            if q["op"] == "jpeg_compression":
                r["jpeg"] = 1
                r["quant"] = jpeg_quant_tables(q["quality"])
            else:
                k = int(q["ksize"])
                if k not in KSIZES:
                    raise ValueError("ksize must be 3, 5 or 7")
                r["spatial"] = _SPATIAL_CODE[q["op"]]
                r["ksize"] = k
                if q["op"] == "motion_blur":
                    kern = np.asarray(q["kernel"]).reshape(k, k) != 0
                    bits = 0
                    for i in np.flatnonzero(kern.reshape(-1)):
                        bits |= 1 << int(i)
                    r["motion"] = [bits & 0xFFFFFFFF, bits >> 32]
        n = p.get("noise")
        if n is not None:
            r["noise"] = _NOISE_CODE[n["op"]]
            r["sigma"] = n["sigma"]
            seed = int(n["seed"]) & (2 ** 64 - 1)
            r["seed"] = [seed & 0xFFFFFFFF, seed >> 32]
    return rec


class _Params(object):
    """Pinned host records of endo_augment; a slot is rewritten only after the stream has passed its previous use."""

    def __init__(self, slots=4):
        self.slots = [dict(buf=None, event=None) for _ in range(slots)]
        self._next = 0

    def stage(self, rec):
        slot = self.slots[self._next]
        self._next = (self._next + 1) % len(self.slots)
        if slot["event"] is not None:
            slot["event"].synchronize()
        raw = rec.view(np.uint8).reshape(-1)
        if slot["buf"] is None or slot["buf"].numel() < raw.size:
            slot["buf"] = torch.empty(raw.size, dtype=torch.uint8).pin_memory()
        slot["buf"][:raw.size].numpy()[:] = raw
        return slot

    @staticmethod
    def done(slot):
        if slot["event"] is None:
            slot["event"] = torch.cuda.Event()
        slot["event"].record()


_params = None


def apply_plan(imgs_u8, plan, out_f32=None, out_u8=None, params=None):
    """Run a plan on a device uint8 (F, H, W, 3) RGB batch on the current stream.  Writes out_u8 (F, H, W, 3) uint8 and / or out_f32
    (F, 3, H, W) fp32 = Normalize(0.5, 0.5); with neither, returns a new uint8 tensor.  Returns out_f32 if given, else out_u8.
    params: the pinned record slots to stage through (a TrainingAugmentation has its own; default: this module's, one thread at a time)."""
    global _params
    lib = _lib.load()
    if imgs_u8.dtype != torch.uint8 or not imgs_u8.is_cuda or not imgs_u8.is_contiguous() or imgs_u8.dim() != 4 or imgs_u8.shape[-1] != 3:
        raise ValueError("expected a contiguous uint8 device tensor (F, H, W, 3)")
    frames, h, w = int(imgs_u8.shape[0]), int(imgs_u8.shape[1]), int(imgs_u8.shape[2])
    if len(plan) != frames:
        raise ValueError("the plan has %d frames, the batch %d" % (len(plan), frames))
    if lib.endo_augment_frame_bytes() != FRAME_DTYPE.itemsize:
        raise RuntimeError("endo_augment_frame layout differs from FRAME_DTYPE")
    if out_u8 is None and out_f32 is None:
        out_u8 = torch.empty_like(imgs_u8)
    for t, shape, dt in ((out_u8, (frames, h, w, 3), torch.uint8), (out_f32, (frames, 3, h, w), torch.float32)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
            raise ValueError("output must be a contiguous device tensor of shape %s, %s" % (shape, dt))
    need = int(lib.endo_augment_workspace_bytes(frames, h, w))
    if need < 0:
        raise ValueError("frames of %d x %d are too small (H, W >= 4)" % (h, w))
    workspace = torch.empty(need, dtype=torch.uint8, device=imgs_u8.device)
    if params is None:
        if _params is None:
            _params = _Params()
        params = _params
    slot = params.stage(plan_records(plan))
    _lib.check(lib.endo_augment(_lib.ptr(imgs_u8), ctypes.c_void_p(slot["buf"].data_ptr()), frames, h, w, _lib.ptr(out_u8), _lib.ptr(out_f32),
                                _lib.ptr(workspace), need, _lib.stream()), "endo_augment")
    params.done(slot)
    return out_f32 if out_f32 is not None else out_u8


# ---------------------------------------------------------------------------------------------
# one operation on a whole batch (the same kernels); per-frame parameters may be scalars or sequences of length F
# ---------------------------------------------------------------------------------------------
def _per_frame(value, frames):
    if isinstance(value, (list, tuple, np.ndarray)) and not (isinstance(value, np.ndarray) and value.ndim == 2):
        if len(value) != frames:
            raise ValueError("expected one value per frame")
        return list(value)
    return [value] * frames


def _single(imgs_u8, stage, entries, out_f32, out_u8):
    plan = [{"colour": None, "quality": None, "noise": None} for _ in entries]
    for p, e in zip(plan, entries):
        p[stage] = e
    return apply_plan(imgs_u8, plan, out_f32=out_f32, out_u8=out_u8)


def brightness_contrast_gamma(imgs_u8, alpha=1.0, beta=0.0, gamma=None, out_f32=None, out_u8=None):
    """RandomBrightnessContrast (contrast alpha, brightness beta by max) then, when gamma is given, RandomGamma."""
    f = imgs_u8.shape[0]
    return _single(imgs_u8, "colour", [{"op": "lut", "alpha": a, "beta": b, "gamma": g}
                                       for a, b, g in zip(_per_frame(alpha, f), _per_frame(beta, f), _per_frame(gamma, f))], out_f32, out_u8)


def shift_hsv(imgs_u8, hue_shift, sat_shift=0.0, val_shift=0.0, out_f32=None, out_u8=None):
    """HueSaturationValue with the given shifts (hue over OpenCV's 8-bit range [0, 180))."""
    f = imgs_u8.shape[0]
    return _single(imgs_u8, "colour", [{"op": "hsv", "hue": hh, "sat": ss, "val": vv}
                                       for hh, ss, vv in zip(_per_frame(hue_shift, f), _per_frame(sat_shift, f), _per_frame(val_shift, f))],
                   out_f32, out_u8)


def box_blur(imgs_u8, ksize, out_f32=None, out_u8=None):
    """Blur: cv2.blur with a k x k box, BORDER_REFLECT_101."""
    return _single(imgs_u8, "quality", [{"op": "blur", "ksize": k} for k in _per_frame(ksize, imgs_u8.shape[0])], out_f32, out_u8)


def median_blur(imgs_u8, ksize, out_f32=None, out_u8=None):
    """MedianBlur: cv2.medianBlur, BORDER_REPLICATE."""
    return _single(imgs_u8, "quality", [{"op": "median_blur", "ksize": k} for k in _per_frame(ksize, imgs_u8.shape[0])], out_f32, out_u8)


def motion_blur(imgs_u8, kernel, out_f32=None, out_u8=None):
    """MotionBlur with a given k x k 0/1 mask (one for every frame, or a list of masks): the mean of the marked taps."""
    single = not isinstance(kernel, (list, tuple)) or np.ndim(kernel[0]) < 2
    masks = [np.asarray(kernel)] * imgs_u8.shape[0] if single else [np.asarray(k) for k in kernel]
    return _single(imgs_u8, "quality", [{"op": "motion_blur", "ksize": m.shape[0], "kernel": m} for m in masks], out_f32, out_u8)


def jpeg_compression(imgs_u8, quality, out_f32=None, out_u8=None):
    """JpegCompression: the cv2.imencode / cv2.imdecode round trip at `quality`, bit-identical to libjpeg-turbo."""
    return _single(imgs_u8, "quality", [{"op": "jpeg_compression", "quality": q} for q in _per_frame(quality, imgs_u8.shape[0])], out_f32, out_u8)


def gauss_noise(imgs_u8, sigma, seed, out_f32=None, out_u8=None):
    """GaussNoise with standard deviation sigma (albumentations draws var in var_limit and uses sqrt(var))."""
    f = imgs_u8.shape[0]
    return _single(imgs_u8, "noise", [{"op": "gauss_noise", "sigma": s, "seed": seed} for s in _per_frame(sigma, f)], out_f32, out_u8)


def additive_gaussian_noise(imgs_u8, scale, seed, out_f32=None, out_u8=None):
    """IAAAdditiveGaussianNoise(per_channel=False) with standard deviation `scale`."""
    f = imgs_u8.shape[0]
    return _single(imgs_u8, "noise", [{"op": "additive_gaussian_noise", "sigma": s, "seed": seed} for s in _per_frame(scale, f)], out_f32, out_u8)
