"""Plain-torch fp32 restatement of the photometric term (losses.PhotometricLoss): the reference's chain

    [u, v] = _warp_coordinate_generate(depth, mask, t, R, K)          (models.py:377-429: oracle.geometry.projected_coordinates)
    warped = images_warping(colors_2, u, v, padding_mode)             (models.py:317-336: F.grid_sample, image_warp_restate)
    MaskedL1Loss(eps)([colors_1, warped, intersect])                  (losses.py:82-91)

for the shapes tests/golden/photometric.npz does not hold; it is pinned to the reference's own outputs by that fixture
(tests/test_photometric_host.py).  Also the input builders and the conditions the fixture's generator and the tests share."""

import numpy as np
import torch

import image_warp_restate as iwr

MODES = iwr.MODES
KINK_MARGIN = 1.0e-3          # no pixel that counts may have a source location this close (pixels) to a cell boundary
OFFSET_LO, OFFSET_HI = 0.05, 0.5          # |colors_1 - warped| of the built inputs: away from the kink of |.|


def masked_l1(images, warped, intersect, eps=1.0):
    """losses.py:82-91."""
    loss = torch.sum(intersect * torch.abs(images - warped), dim=(1, 2, 3)) / (eps + torch.sum(intersect, dim=(1, 2, 3)))
    return torch.mean(loss)


def photometric(colors_1, colors_2, depth, mask, intersect, t, r, k, eps=1.0, padding_mode="zeros"):
    """The scalar; depth, mask, intersect (N, 1, H, W)."""
    u, v = iwr.warp_coordinates(depth, mask, t, r, k)
    warped = iwr.images_warping(colors_2, u, v, padding_mode)
    return masked_l1(colors_1, warped, intersect, eps)


def value_and_grad(colors_1, colors_2, depth, mask, intersect, t, r, k, eps=1.0, padding_mode="zeros"):
    """(loss, d loss / d depth) on the CPU."""
    depth = depth.detach().clone().requires_grad_(True)
    loss = photometric(colors_1, colors_2, depth, mask, intersect, t, r, k, eps, padding_mode)
    grad, = torch.autograd.grad(loss, depth)
    return loss.detach(), grad


def coordinates(depth, mask, t, r, k):
    """(u, v), each (N, H, W) numpy float32, without a graph."""
    with torch.no_grad():
        u, v = iwr.warp_coordinates(depth, mask, t, r, k)
    return u.numpy(), v.numpy()


def near_kink(u, v, margin=KINK_MARGIN):
    """Pixels whose source location (u - 0.5, v - 0.5) lies within ``margin`` of a multiple of 0.5 in x or y: the cell boundaries of
    every padding mode, the border clips (0 and size - 1) and the reflection points (-0.5 and size - 0.5 and their periods).  A
    non-finite coordinate counts as near."""
    near = np.zeros(np.shape(u), dtype=bool)
    for coord in (u, v):
        loc = 2.0 * (np.asarray(coord, np.float64) - 0.5)
        with np.errstate(invalid="ignore"):
            near |= ~np.isfinite(loc) | (np.abs(loc - np.round(loc)) <= 2.0 * margin)
    return near


def smooth_images(rng, shape):
    """Images whose adjacent pixels differ by at most 0.05 (make_image_warp_golden.py's chain images): one plane wave per channel."""
    n, c, h, w = shape
    ys = np.linspace(0.0, 1.0, h)[None, None, :, None]
    xs = np.linspace(0.0, 1.0, w)[None, None, None, :]
    fy, fx = rng.uniform(0.1, 0.5, (2, n, c, 1, 1))
    ph = rng.uniform(0.0, 2.0 * np.pi, (n, c, 1, 1))
    return (0.4 * np.cos(2.0 * np.pi * (fy * ys + fx * xs) + ph)).astype(np.float32)


def offsets(rng, shape):
    """Magnitudes in [OFFSET_LO, OFFSET_HI] with random signs."""
    return (rng.uniform(OFFSET_LO, OFFSET_HI, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)).astype(np.float32)


def case(shape, seed, pose_scale=1.0, per_sample=True, spin=0.0):
    """Inputs at ``shape`` = (N, C, H, W) for the tests against the restatement: smooth colours 2, a smooth depth, a boundary mask with
    a masked-out margin, per-sample intrinsics and poses, and a random binary intersect mask that is cleared wherever the CPU
    coordinates lie within the margin of a kink (there the device may pick the other cell, and the derivative jumps).  colors_1 is NOT
    built here: it depends on the padding mode (``colors_1_for``).  pose_scale multiplies the translation (large: coordinates leave the
    image); spin (radians) is added to the rotation about the optical axis: with 0.6 the corners of the frame leave the image on all four
    sides."""
    n, c, h, w = shape
    rng = np.random.default_rng(seed)
    k = np.zeros((n, 3, 3), np.float32)
    for i in range(n):
        j = i if per_sample else 0
        k[i] = [[0.9 * w + 3.0 * j, 0.0, 0.5 * w + j], [0.0, 0.9 * w + 2.0 * j, 0.5 * h - j], [0.0, 0.0, 1.0]]
    ang = rng.normal(0.0, 0.03, (n, 3))
    rot = np.zeros((n, 3, 3), np.float32)
    for i in range(n):
        ax, ay, az = ang[i]
        az += spin
        rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        rot[i] = (rz @ ry @ rx).astype(np.float32)
    t = (rng.normal(0.0, 0.04, (n, 3, 1)) * pose_scale).astype(np.float32)
    ys = np.linspace(0.0, 1.0, h)[None, None, :, None]
    xs = np.linspace(0.0, 1.0, w)[None, None, None, :]
    depth = (0.6 + 0.2 * np.cos(2.0 * np.pi * (0.7 * ys + 0.4 * xs) + rng.uniform(0, 6.0, (n, 1, 1, 1)))
             + rng.normal(0.0, 0.01, (n, 1, h, w))).astype(np.float32)
    mask = np.ones((n, 1, h, w), np.float32)
    if h > 4 and w > 4:
        mask[:, :, 0, :] = 0.0
        mask[:, :, :, -1] = 0.0
        mask[:, :, h // 2, w // 2] = 0.0
    x = {"colors_2": smooth_images(rng, shape), "depth": depth, "mask": mask, "t": t, "R": rot, "K": k}
    x = {key: torch.from_numpy(val) for key, val in x.items()}
    u, v = coordinates(x["depth"], x["mask"], x["t"], x["R"], x["K"])
    # the device's coordinates are within 1e-5 of max |.| of these (tests/test_gpu_image_warp.py COORD_TOL): twice that, at least KINK_MARGIN
    finite = np.isfinite(u) & np.isfinite(v)
    reach = max(float(np.abs(u[finite]).max()), float(np.abs(v[finite]).max())) if finite.any() else 0.0
    margin = max(KINK_MARGIN, 2.0e-5 * reach)
    inter = (rng.random((n, h, w)) < 0.7) & ~near_kink(u, v, margin)
    x["intersect"] = torch.from_numpy(inter[:, None].astype(np.float32))
    x["offsets"] = torch.from_numpy(offsets(rng, shape))
    return x


def colors_1_for(x, mode):
    """colors_1 = the restatement's warped colours 2 in ``mode`` plus the case's offsets: no element on the kink of |.|."""
    with torch.no_grad():
        u, v = iwr.warp_coordinates(x["depth"], x["mask"], x["t"], x["R"], x["K"])
        return iwr.images_warping(x["colors_2"], u, v, mode) + x["offsets"]
