"""Writes tests/golden/augment_jpeg.npz: the JPEG files the training augmentation's JpegCompression round trip is pinned against.

albumentations 0.4.6 JpegCompression is cv2.imencode(".jpg", img, quality) + cv2.imdecode on an RGB array that cv2 takes for B, G, R;
the same bytes come from Pillow (libjpeg-turbo) encoding img[..., ::-1] at 4:2:0 with the IJG-scaled Annex K tables that
jpeg_set_quality(quality, force_baseline=TRUE) builds.  The tables are handed to Pillow explicitly and read back from every file,
so a table that differs from augment.jpeg_quant_tables (force_baseline's clamp to 255 included) fails here.

Needs numpy and Pillow only.  Contents:
  img_<name>      uint8 (H, W, 3) RGB source images: crops of the example sequence's first frame at 256 x 320, 64 x 96 and 37 x 53
                  (odd, not a multiple of 8), and a synthetic 48 x 80 image of saturated colours with hard edges
  jpg_<name>_q<q> uint8 bytes of the file, for every image and q in QUALITIES
  quant_q<q>      uint16 (2, 64) natural-order tables
Run from the repository root: python tests/golden/make_augment_golden.py
"""

import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
QUALITIES = (20, 31, 50, 68, 85, 95, 100)
FRAME = os.path.join(HERE, "example_sequence", "bag_1", "_start_004259_end_004629_stride_25_segment_13", "00004584.jpg")

# ITU T.81 Annex K tables, natural order (libjpeg jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl)
STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
            103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66] + [99] * 38


def quant_tables(quality):
    """jcparam.c jpeg_set_quality(quality, force_baseline=TRUE): scale 5000 / q below 50, else 200 - 2 q; (t * scale + 50) / 100
    clamped to [1, 255].  Stated here on its own, so that the fixture also checks augment.jpeg_quant_tables."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.array([[min(255, max(1, (t * scale + 50) // 100)) for t in table] for table in (STD_LUMA, STD_CHROMA)], np.uint16)


def synthetic(h=48, w=80):
    """Saturated primaries and secondaries in hard-edged bands, a checkerboard and a white / black diagonal."""
    img = np.zeros((h, w, 3), np.uint8)
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]],
                       np.uint8)
    for x in range(w):
        img[:, x] = colours[(x // 7) % len(colours)]
    yy, xx = np.mgrid[0:h, 0:w]
    board = ((yy // 3 + xx // 3) % 2 == 0) & (yy >= h // 2)
    img[board] = colours[(xx[board] // 5) % 3 + 3]
    img[np.abs(yy - xx * h // w) <= 1] = [255, 255, 255]
    img[np.abs(yy + xx * h // w - h) <= 1] = [0, 0, 0]
    return img


def sources():
    from PIL import Image
    with Image.open(FRAME) as im:
        frame = np.asarray(im.convert("RGB"))
    return {"256x320": frame[400:656, 800:1120].copy(), "64x96": frame[300:364, 1000:1096].copy(), "37x53": frame[611:648, 901:954].copy(),
            "48x80": synthetic()}


def encode(img, quality):
    """Pillow's bytes for cv2.imencode(".jpg", img, [IMWRITE_JPEG_QUALITY, quality]) of an RGB array img."""
    from PIL import Image
    q = quant_tables(quality)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(buf, format="JPEG", qtables=[q[0].tolist(), q[1].tolist()], subsampling=2,
                                                              optimize=False, progressive=False)
    data = buf.getvalue()
    with Image.open(io.BytesIO(data)) as back:
        got = back.quantization
    # Pillow takes and reports the tables in natural order
    for t in (0, 1):
        if not np.array_equal(np.asarray(got[t]), q[t]):
            raise AssertionError("quality %d: table %d read back differs from the IJG-scaled table" % (quality, t))
    return data


def build():
    out = {}
    for name, img in sources().items():
        out["img_" + name] = img
        for q in QUALITIES:
            out["jpg_%s_q%d" % (name, q)] = np.frombuffer(encode(img, q), np.uint8)
    for q in QUALITIES:
        out["quant_q%d" % q] = quant_tables(q)
    return out


def main():
    path = os.path.join(HERE, "augment_jpeg.npz")
    np.savez_compressed(path, **build())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
