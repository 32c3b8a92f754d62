"""numpy restatements of the training augmentations (endoscopydepthestimation-pytorch_amd/augment.py, csrc/augment.hip): what the
kernels are checked against.  Sources restated: albumentations 0.4.6, OpenCV's 8-bit colour / filter paths, libjpeg-turbo's encoder
(jccolor.c, jcsample.c, jcprepct.c, jfdctint.c, jcdctmgr.c, jccoefct.c); the decoder half is oracle.reader's.
Images are uint8 (..., H, W, 3) in RGB order, as albumentations sees them."""

import numpy as np

from oracle import reader as oreader


# ---------------------------------------------------------------------------------------------
# colour
# ---------------------------------------------------------------------------------------------
def apply_lut(img, lut):
    return np.asarray(lut, np.uint8)[img]


def rgb_to_hsv(img, hrange=180, blue_index=2):
    """cv2.COLOR_RGB2HSV (hrange 180) / COLOR_RGB2HSV_FULL (256) on uint8, OpenCV's scalar fixed-point path (color_hsv RGB2HSV_b):
    sdiv[i] = round((255 << 12) / i), hdiv[i] = round((hrange << 12) / (6 i)), + hrange when negative, saturated to 8 bits.
    blue_index 2: RGB input; 0: BGR.  PARITY UNPINNED against cv2 itself."""
    img = np.asarray(img, np.uint8)
    b = img[..., blue_index].astype(np.int64)
    g = img[..., 1].astype(np.int64)
    r = img[..., 2 - blue_index].astype(np.int64)
    idx = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256, np.int64)
    hdiv = np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << 12) / idx).astype(np.int64)
    hdiv[1:] = np.rint((hrange << 12) / (6.0 * idx)).astype(np.int64)
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    hterm = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (hterm * hdiv[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + hrange, h)
    return np.stack([np.clip(h, 0, 255), s, v], axis=-1).astype(np.uint8)


_SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])          # {b, g, r} per sector


def hsv180_to_rgb(hsv):
    """cv2.COLOR_HSV2RGB on uint8 (color_hsv HSV2RGB_b -> HSV2RGB_native, hscale = 6 / 180), every operation in float32 as written
    there: s = S / 255, v = V / 255, h = fmod(H * hscale, 6), sector = floor(h), tab = {v, v (1 - s), v (1 - s f), v (1 - s (1 - f))},
    output cvRound(x * 255).  PARITY UNPINNED against cv2 itself (its SIMD path included)."""
    hsv = np.asarray(hsv, np.uint8)
    f32 = np.float32
    s = hsv[..., 1].astype(f32) * f32(1.0 / 255.0)
    v = hsv[..., 2].astype(f32) * f32(1.0 / 255.0)
    h = hsv[..., 0].astype(f32) * f32(6.0 / 180.0)
    h = np.fmod(h, f32(6.0))
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f32(0), h).astype(f32)
    one = f32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    pick = _SECTORS[sector]                                               # (..., 3): b, g, r indices
    bgr = np.take_along_axis(tab, pick, axis=-1)
    grey = (s == 0)[..., None]
    bgr = np.where(grey, v[..., None], bgr)
    rgb = bgr[..., ::-1] * f32(255.0)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def shift_hsv(img, luts):
    """albumentations 0.4.6 _shift_hsv_uint8 with the (3, 256) LUTs of augment.hsv_luts."""
    hsv = rgb_to_hsv(img, 180)
    out = np.stack([np.asarray(luts[c], np.uint8)[hsv[..., c]] for c in range(3)], axis=-1)
    return hsv180_to_rgb(out)


# ---------------------------------------------------------------------------------------------
# spatial
# ---------------------------------------------------------------------------------------------
def _windows(img, k, mode):
    """(..., H, W, 3, k, k) views of the padded image; mode "reflect" = BORDER_REFLECT_101, "edge" = BORDER_REPLICATE."""
    r = k // 2
    pad = [(0, 0)] * (img.ndim - 3) + [(r, r), (r, r), (0, 0)]
    p = np.pad(img, pad, mode=mode)
    return np.lib.stride_tricks.sliding_window_view(p, (k, k), axis=(-3, -2))


def box_blur(img, k):
    """cv2.blur(img, (k, k)): the integer sum over the box / k^2, rounded to nearest (k^2 odd: no ties)."""
    s = _windows(np.asarray(img, np.uint8), k, "reflect").astype(np.int64).sum(axis=(-2, -1))
    return ((2 * s + k * k) // (2 * k * k)).astype(np.uint8)


def median_blur(img, k):
    """cv2.medianBlur(img, k) per channel, BORDER_REPLICATE."""
    img = np.asarray(img, np.uint8)
    out = np.empty_like(img)
    flat = img.reshape((-1,) + img.shape[-3:])
    for i in range(flat.shape[0]):
        win = _windows(flat[i], k, "edge").reshape(flat.shape[1:] + (k * k,))
        out.reshape(flat.shape)[i] = np.partition(win, (k * k) // 2, axis=-1)[..., (k * k) // 2]
    return out


def motion_blur(img, mask):
    """cv2.filter2D(img, -1, mask / mask.sum()) as specified: correlation, centre anchor, BORDER_REFLECT_101, the integer sum of the
    n marked taps / n rounded half to even."""
    mask = np.asarray(mask) != 0
    k = mask.shape[0]
    r = k // 2
    img = np.asarray(img, np.uint8)
    pad = [(0, 0)] * (img.ndim - 3) + [(r, r), (r, r), (0, 0)]
    p = np.pad(img, pad, mode="reflect").astype(np.int64)
    h, w = img.shape[-3], img.shape[-2]
    s = np.zeros(img.shape, np.int64)
    for i, j in zip(*np.nonzero(mask)):
        s += p[..., i:i + h, j:j + w, :]
    n = int(mask.sum())
    q, rem = s // n, s % n
    q += (2 * rem > n) | ((2 * rem == n) & (q % 2 == 1))
    return q.astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# JPEG: encoder half (libjpeg-turbo) + oracle.reader's decoder half
# ---------------------------------------------------------------------------------------------
def _fdct_1d(d, first):
    """jfdctint.c jpeg_fdct_islow, one pass over the leading axis of d (8, ...) int64."""
    tmp0, tmp7 = d[0] + d[7], d[0] - d[7]
    tmp1, tmp6 = d[1] + d[6], d[1] - d[6]
    tmp2, tmp5 = d[2] + d[5], d[2] - d[5]
    tmp3, tmp4 = d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    shift = 11 if first else 15
    rnd = 1 << (shift - 1)
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) * 4, (tmp10 - tmp11) * 4
    else:
        o[0], o[4] = (tmp10 + tmp11 + 2) >> 2, (tmp10 - tmp11 + 2) >> 2
    z1 = (tmp12 + tmp13) * 4433
    o[2] = (z1 + tmp13 * 6270 + rnd) >> shift
    o[6] = (z1 + tmp12 * (-15137) + rnd) >> shift
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = (t4 + z1 + z3 + rnd) >> shift
    o[5] = (t5 + z2 + z4 + rnd) >> shift
    o[3] = (t6 + z2 + z3 + rnd) >> shift
    o[1] = (t7 + z1 + z4 + rnd) >> shift
    return np.stack(o)


def fdct_islow(blocks):
    """(..., 8, 8) level-shifted samples [row][column] -> (..., 8, 8) DCT outputs scaled by 8, as jpeg_fdct_islow leaves them."""
    b = np.asarray(blocks, np.int64)
    rows = _fdct_1d(np.moveaxis(b, -1, 0), True)            # pass 1 over each row: (8 u, ..., 8 rows)
    rows = np.moveaxis(rows, 0, -1)                          # (..., rows, u)
    cols = _fdct_1d(np.moveaxis(rows, -2, 0), False)         # pass 2 over each column
    return np.moveaxis(cols, 0, -2)


def quantize(coef, quant):
    """libjpeg-turbo jcdctmgr.c quantize() with compute_reciprocal(8 q): sign(t) * (((|t| + c) * fq) >> r)."""
    q = np.asarray(quant, np.int64).reshape(8, 8)
    div = 8 * q
    b = np.floor(np.log2(div)).astype(np.int64)
    r = 16 + b
    fq = (np.int64(1) << r) // div
    fr = (np.int64(1) << r) % div
    c = div // 2
    pow2 = fr == 0
    fq = np.where(pow2, fq >> 1, np.where(fr <= div // 2, fq, fq + 1))
    r = np.where(pow2, r - 1, r)
    c = np.where(~pow2 & (fr <= div // 2), c + 1, c)
    t = np.asarray(coef, np.int64)
    v = ((np.abs(t) + c) * fq) >> r
    return np.where(t < 0, -v, v)


def jpeg_encode(img, quant):
    """Quantised coefficient blocks [Y (2 my, 2 mx, 8, 8), Cb (my, mx, 8, 8), Cr] of cv2.imencode(".jpg") of an RGB array (which cv2
    reads as B, G, R) at 4:2:0 with the (2, 64) natural-order tables `quant` -- blocks as endo_jpeg_entropy_decode returns them,
    the dummy blocks of jccoefct.c compress_data included."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    mx, my = (w + 15) // 16, (h + 15) // 16
    p = np.pad(img, ((0, my * 16 - h), (0, mx * 16 - w), (0, 0)), mode="edge").astype(np.int64)   # expand_right / bottom_edge
    R, G, B = p[..., 2], p[..., 1], p[..., 0]
    y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16                                          # jccolor.c, SCALEBITS 16
    cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    bias = np.where(np.arange(mx * 8) % 2 == 1, 2, 1)
    ch = (h + 1) // 2
    rows = np.minimum(np.arange(my * 8), ch - 1)                                                   # jcprepct: repeat the last chroma row
    chroma = []
    for plane in (cb, cr):
        d = (plane[0::2, 0::2] + plane[0::2, 1::2] + plane[1::2, 0::2] + plane[1::2, 1::2] + bias) >> 2   # jcsample h2v2_downsample
        chroma.append(d[rows])
    out = []
    for plane, q in ((y, quant[0]), (chroma[0], quant[1]), (chroma[1], quant[1])):
        bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
        blocks = (plane - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        out.append(quantize(fdct_islow(blocks), q))
    # jccoefct.c compress_data: luma blocks past the image's blocks are dummies -- zero, with the DC of the block before them in the MCU
    yb = out[0]
    wb, hb = (w + 7) // 8, (h + 7) // 8
    if wb % 2:
        yb[:, wb] = 0
        yb[:, wb, 0, 0] = yb[:, wb - 1, 0, 0]
    if hb % 2:
        yb[hb] = 0
        for m in range(mx):
            yb[hb, 2 * m:2 * m + 2, 0, 0] = yb[hb - 1, 2 * m + 1, 0, 0]
    return out


def jpeg_roundtrip(img, quant):
    """cv2.imdecode(cv2.imencode(".jpg", img)) of an RGB array: libjpeg's decoder on jpeg_encode's blocks, channels back in the
    array's order (cv2's B, G, R = the array's 0, 1, 2)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    blocks = jpeg_encode(img, quant)
    tables = [np.asarray(quant[0]).reshape(8, 8), np.asarray(quant[1]).reshape(8, 8), np.asarray(quant[1]).reshape(8, 8)]
    rgb = oreader.decode_jpeg_blocks(blocks, tables, w, h)
    return np.ascontiguousarray(rgb[..., ::-1])
