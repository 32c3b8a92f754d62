"""Test phase on the host (reference evaluate.py:329-345, utils.py:825-865, 1405-1412): the numpy restatement the device outputs are
checked against (tests/evaluate_restate.py) on hand-made cases, the PNG and PLY writers that replace cv2.imwrite and plyfile, and the
frame-file lookup of --load_all_frames.  No GPU."""

import importlib
import os
import struct
import zlib
from fractions import Fraction

import numpy as np
import pytest

import evaluate_restate as er

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
utils = ea.utils


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def test_jet_table():
    """COLORMAP_JET restated: 256 B, G, R entries, entry 0 = (128, 0, 0), entry 255 = (0, 0, 128), every entry within half a unit of
    255 x the exact piecewise-linear curve, and each channel rising, flat at 255 and falling in that order."""
    assert er.JET.shape == (256, 3) and er.JET.dtype == np.uint8
    assert tuple(er.JET[0]) == (128, 0, 0) and tuple(er.JET[255]) == (0, 0, 128)
    for i in range(256):
        x = Fraction(i, 255)
        for ch, (a, c) in enumerate(((Fraction(1, 2), Fraction(5, 2)), (Fraction(-1, 2), Fraction(7, 2)), (Fraction(-3, 2), Fraction(9, 2)))):
            exact = 255 * min(max(min(4 * x + a, c - 4 * x), Fraction(0)), Fraction(1))
            assert abs(int(er.JET[i, ch]) - exact) <= Fraction(1, 2), (i, ch)
    for ch in range(3):
        v = er.JET[:, ch].astype(int)
        top = np.flatnonzero(v == 255)
        assert top.size > 0 and np.all(np.diff(top) == 1), ch          # one plateau at 255
        assert np.all(np.diff(v[:top[0] + 1]) >= 0) and np.all(np.diff(v[top[-1]:]) <= 0), ch
    assert np.array_equal(er.JET[:, 0] == 255, er.JET[::-1, 2] == 255)          # blue and red mirror each other


def _below(target):
    """The largest float32 c whose 255 * (0.5 c + 0.5) (float32, three roundings) is below `target`: a display value x.99999."""
    f32 = np.float32
    c = f32(2.0 * target / 255.0 - 1.0)
    while f32(255) * (f32(0.5) * c + f32(0.5)) >= f32(target):
        c = np.nextafter(c, f32(-2))
    return c


def test_color_display_truncates_and_masks():
    targets = [1, 2, 100, 128, 200, 254, 255]
    c = np.zeros((3, 2, len(targets)), np.float32)
    for j, t in enumerate(targets):
        c[:, 0, j] = _below(t)
        c[:, 1, j] = np.float32(2.0 * t / 255.0 - 1.0) if t < 255 else np.float32(1.0)
    v = np.float32(255) * (np.float32(0.5) * c[0, 0] + np.float32(0.5))
    assert np.all(v > np.array(targets, np.float32) - np.float32(1e-3)) and np.all(v < np.array(targets, np.float32))
    u = er.display_u8(c)
    assert u[0, :, 0].tolist() == [t - 1 for t in targets]          # x.99999 truncates
    assert u[1, -1, 0] == 255
    # the masked-out pixels: c = b * colors = 0 gives 127 before the mask, 0 after it
    zero = np.zeros((3, 4, 5), np.float32)
    assert np.all(er.display_u8(zero) == 127)
    b = np.ones((4, 5), np.float32)
    b[1:3, 2:] = 0.0
    disp = er.color_display(zero, b)
    assert np.all(disp[b == 0] == 0) and np.all(disp[b == 1] == 127)
    # channel order: RGB input -> B, G, R
    rgb = np.stack([np.full((1, 1), v, np.float32) for v in (1.0, 0.0, -1.0)])
    assert er.color_display(rgb, np.ones((1, 1), np.float32))[0, 0].tolist() == [0, 127, 255]
    # HSV: grey (s = 0) keeps v in all three channels; hue 0 at full s, v is pure red
    hsv = np.stack([np.full((1, 2), v, np.float32) for v in (-1.0, 1.0, 1.0)])
    hsv[1, 0, 0] = -1.0
    assert er.color_display(hsv, np.ones((1, 2), np.float32), is_hsv=True)[0].tolist() == [[255, 255, 255], [0, 0, 255]]


def test_depth_display():
    d = np.zeros((3, 4), np.float32)
    assert np.all(er.depth_index(d) == 0) and np.all(er.depth_display(d) == er.JET[0])          # all-zero frame: entry 0, no NaN
    d = np.array([[0.0, 1.0, 2.0, 4.0]], np.float32)
    assert er.depth_index(d).tolist() == [[0, 63, 127, 255]]
    # a value whose 255 * d / max is x.99999 truncates
    m = np.float32(3.0)
    x = np.float32(100.0 / 255.0 * 3.0)
    while (np.float32(255) * x) / m >= np.float32(100):
        x = np.nextafter(x, np.float32(0))
    assert (np.float32(255) * x) / m > np.float32(99.99)
    assert er.depth_index(np.array([[x, m]], np.float32)).tolist() == [[99, 255]]
    p = er.panel(np.zeros((3, 1, 4), np.float32), np.ones((1, 4), np.float32), d, False)
    assert p.shape == (1, 8, 3) and np.array_equal(p[0, 4:], er.JET[[0, 63, 127, 255]])


def test_point_cloud_restatement_order():
    d = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    b = np.ones((3, 4), np.float32)
    b[0, 1] = 0.0
    col = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
    k = np.array([[2, 0, 1.5], [0, 4, 1], [0, 0, 1]], np.float32)
    pc = er.point_cloud(d, col, b, k, 1)
    assert pc.shape == (11, 6) and pc.dtype == np.float32
    assert pc[0].tolist() == [np.float32(-1.5) / np.float32(2) * np.float32(1), -0.25, 1.0, 2.0, 1.0, 0.0]
    assert pc[1, 2] == 3.0          # (0, 1) is masked out
    assert er.point_cloud(d, col, b, k, 2)[:, 2].tolist() == [1.0, 3.0, 9.0, 11.0]          # (0, 0), (0, 2), (2, 0), (2, 2)


# ---------------------------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 33), (64, 2 * 97)])
def test_write_png_decodes_to_the_panel(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    bgr = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    path = tmp_path / "x.png"
    utils.write_png(path, bgr)
    with Image.open(str(path)) as im:
        assert im.mode == "RGB" and im.size == (shape[1], shape[0])
        assert np.array_equal(np.asarray(im), bgr[:, :, ::-1])
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    assert struct.unpack(">IIBBBBB", data[16:29]) == (shape[1], shape[0], 8, 2, 0, 0, 0)
    assert struct.unpack(">I", data[29:33])[0] == zlib.crc32(data[12:29]) & 0xFFFFFFFF
    with pytest.raises(ValueError):
        utils.write_png(path, bgr[..., 0])


HEADER = ("ply\nformat {}\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
          "property uchar green\nproperty uchar blue\nend_header\n")


def _points(n, seed=3):
    rng = np.random.default_rng(seed)
    pts = np.empty((n, 6), np.float32)
    pts[:, :3] = (rng.standard_normal((n, 3)) * np.array([1e-3, 10.0, 1e4])).astype(np.float32)
    pts[:, 3:] = rng.integers(0, 256, size=(n, 3))
    if n >= 4:
        pts[0, :3] = [0.0, -0.0, np.float32(1) / np.float32(3)]
        pts[1, :3] = [np.finfo(np.float32).tiny, np.finfo(np.float32).max, -np.finfo(np.float32).eps]
        pts[2, 3:] = [0, 255, 128]
    return pts


@pytest.mark.parametrize("n", [0, 1, 257])
def test_write_point_cloud_text(tmp_path, n):
    pts = _points(n)
    path = tmp_path / "p.ply"
    utils.write_point_cloud(path, pts)
    text = path.read_text()
    head = HEADER.format("ascii 1.0", n)
    assert text.startswith(head)
    lines = text[len(head):].split("\n")
    assert lines[-1] == "" and len(lines) == n + 1
    back = np.array([[float(v) for v in line.split(" ")] for line in lines[:-1]], np.float64).reshape(-1, 6)
    assert all(len(line.split(" ")) == 6 for line in lines[:-1])
    assert np.array_equal(back[:, :3].astype(np.float32).view(np.uint32), pts[:, :3].view(np.uint32))          # every bit, -0 included
    assert np.array_equal(back[:, 3:], pts[:, 3:].astype(np.float64))
    assert all(v.isdigit() for line in lines[:-1] for v in line.split(" ")[3:])          # uchar values print as integers


@pytest.mark.parametrize("n", [0, 1, 257])
def test_write_point_cloud_binary(tmp_path, n):
    pts = _points(n)
    path = tmp_path / "p.ply"
    utils.write_point_cloud(path, pts, text=False)
    data = path.read_bytes()
    head = HEADER.format("binary_little_endian 1.0", n).encode("ascii")
    assert data.startswith(head) and len(data) == len(head) + 15 * n
    rec = np.frombuffer(data[len(head):], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, name in enumerate(("x", "y", "z")):
        assert np.array_equal(rec[name].view(np.uint32), pts[:, k].view(np.uint32))
    for k, name in enumerate(("red", "green", "blue")):
        assert np.array_equal(rec[name], pts[:, 3 + k].astype(np.uint8))


def test_get_filenames_from_frame_indexes(tmp_path):
    root = tmp_path / "seq"
    for rel in ("a/00000007.jpg", "a/00000003.jpg", "b/c/00000005.jpg", "b/00000003.jpg", "a/00000009.png", "00000011.jpg"):
        (root / rel).parent.mkdir(parents=True, exist_ok=True)
        (root / rel).write_bytes(b"")
    got = utils.get_filenames_from_frame_indexes(root, [11, 9, 7, 5, 3, 1])
    assert [os.path.relpath(str(p), str(root)) for p in got] == ["00000011.jpg", "a/00000003.jpg", "a/00000007.jpg", "b/c/00000005.jpg"]
    assert utils.get_filenames_from_frame_indexes(root, []) == []
