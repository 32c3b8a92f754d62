"""Training augmentations (augment.py, reference train.py:121-142), the host half: the sampler's distributions, the LUT and table
builders, the C ABI's argument checks, and the numpy restatement of the JPEG encoder (tests/augment_restate.py) against the files
libjpeg-turbo wrote for tests/golden/augment_jpeg.npz -- read back through the library's host-only Huffman decoder, no GPU."""

import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

import augment_restate as ar
from oracle import reader as oreader

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
augment = importlib.import_module("endoscopydepthestimation-pytorch_amd.augment")

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "augment_jpeg.npz")
NAMES = ("256x320", "64x96", "37x53", "48x80")
QUALITIES = (20, 31, 50, 68, 85, 95, 100)


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def draws():
    return augment.TrainingAugmentation(seed=11).sample(200000)


# ---------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_stage_and_branch_frequencies(draws):
    n = len(draws)
    for stage in ("colour", "quality", "noise"):
        rate = sum(p[stage] is not None for p in draws) / n
        assert abs(rate - 0.5) < 0.005, (stage, rate)
    # albumentations 0.4.6 OneOf weights its children by their own p: colour = Compose (p 1.0) vs HueSaturationValue (p 0.5)
    shares = [("colour", augment.COLOUR_OPS[0], 1.0 / 3), ("colour", augment.COLOUR_OPS[1], 1.0 / 6)]
    shares += [("quality", op, 0.125) for op in augment.QUALITY_OPS] + [("noise", op, 0.25) for op in augment.NOISE_OPS]
    for stage, op, share in shares:
        rate = sum(p[stage] is not None and p[stage]["op"] == op for p in draws) / n
        assert abs(rate - share) < 0.005, (op, rate, share)


def test_sampler_parameter_ranges(draws):
    colour = [p["colour"] for p in draws if p["colour"] is not None]
    for c in colour:
        assert -30 <= c["hue"] <= 30
        if c["op"] == augment.COLOUR_OPS[0]:
            assert 0.7 <= c["alpha"] <= 1.3 and -0.3 <= c["beta"] <= 0.3 and c["sat"] == 0 and c["val"] == 0
            assert 0.8 <= c["gamma"] <= 1.2 and abs(round(c["gamma"] * 100) - c["gamma"] * 100) < 1e-9
        else:
            assert -30 <= c["sat"] <= 30 and -30 <= c["val"] <= 30
    gammas = {c["gamma"] for c in colour if "gamma" in c}
    assert 0.8 in gammas and 1.2 in gammas
    quality = [p["quality"] for p in draws if p["quality"] is not None]
    qualities = {q["quality"] for q in quality if q["op"] == "jpeg_compression"}
    assert min(qualities) == 20 and max(qualities) == 100
    for op in ("blur", "median_blur", "motion_blur"):
        assert {q["ksize"] for q in quality if q["op"] == op} == {3, 5, 7}
    for p in draws:
        n = p["noise"]
        if n is None:
            continue
        if n["op"] == "gauss_noise":
            assert np.sqrt(10) <= n["sigma"] <= np.sqrt(30)
        else:
            assert 1.275 <= n["sigma"] <= 5.1
        assert 0 <= n["seed"] < 2 ** 64


def _eight_connected(mask):
    """The marked taps form one 8-connected chain (a rasterised segment): a path that visits each once with king moves."""
    pts = [tuple(p) for p in np.argwhere(mask)]
    if len(pts) < 2:
        return False
    degree = [sum(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for b in pts) for a in pts]
    return degree.count(1) == 2 and all(1 <= d <= 2 for d in degree)


def test_motion_kernels_are_lines(draws):
    masks = [p["quality"]["kernel"] for p in draws if p["quality"] is not None and p["quality"]["op"] == "motion_blur"]
    assert len(masks) > 20000
    vertical = 0
    for m in masks[:5000]:
        k = m.shape[0]
        assert m.shape == (k, k) and set(np.unique(m)) <= {0, 1}
        assert _eight_connected(m), m
        cols = np.nonzero(m.any(axis=0))[0]
        if len(cols) == 1:
            vertical += 1
            assert m.sum() >= 2
    assert vertical > 0


def test_line_mask_known_answers():
    assert augment.line_mask(3, 0, 0, 2, 2).tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert augment.line_mask(5, 0, 0, 4, 2).tolist() == [[1, 1, 0, 0, 0], [0, 0, 1, 1, 0], [0, 0, 0, 0, 1]] + [[0] * 5] * 2
    assert augment.line_mask(5, 4, 2, 0, 0).tolist() == augment.line_mask(5, 0, 0, 4, 2).tolist()          # walked from the left end
    assert augment.line_mask(5, 4, 0, 0, 2).tolist() == [[0, 0, 0, 0, 1], [0, 0, 1, 1, 0], [1, 1, 0, 0, 0]] + [[0] * 5] * 2
    assert augment.line_mask(3, 2, 0, 0, 1).tolist() == [[0, 0, 1], [1, 1, 0], [0, 0, 0]]          # (0, 1) -> (2, 0) on a tie
    rng = np.random.default_rng(0)
    for _ in range(200):
        k = int(rng.choice([3, 5, 7]))
        xs, ys, xe, ye = (int(v) for v in rng.integers(0, k, 4))
        assert np.array_equal(augment.line_mask(k, xs, ys, xe, ye), augment.line_mask(k, xe, ye, xs, ys))
    assert augment.line_mask(7, 3, 6, 3, 1)[1:7, 3].tolist() == [1] * 6 and augment.line_mask(7, 3, 6, 3, 1).sum() == 6


def test_sampler_is_reproducible():
    a = augment.TrainingAugmentation(seed=5).sample(64)
    b = augment.TrainingAugmentation(seed=5).sample(64)
    c = augment.TrainingAugmentation(seed=6).sample(64)
    assert repr(a) == repr(b) and repr(a) != repr(c)
    ra, rb = augment.plan_records(a), augment.plan_records(b)
    assert ra.tobytes() == rb.tobytes()


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------
def test_lut_builders_known_answers():
    at = [0, 1, 127, 254, 255]
    assert augment.brightness_contrast_lut(1.3, 0.3)[at].tolist() == [76, 77, 241, 255, 255]          # 255 * 0.3 = 76.5
    assert augment.brightness_contrast_lut(0.7, -0.3)[at].tolist() == [0, 0, 12, 101, 102]            # 127 * 0.7 - 76.5 = 12.4
    assert augment.brightness_contrast_lut(1.0, 0.0).tolist() == list(range(256))
    assert augment.gamma_lut(0.8)[at].tolist() == [0, 3, 145, 254, 255]
    assert augment.gamma_lut(1.2)[at].tolist() == [0, 0, 110, 253, 255]
    assert augment.gamma_lut(1.0)[[1, 2, 3, 127, 255]].tolist() == [1, 2, 3, 127, 255]
    h, s, v = augment.hsv_luts(-30.5, 12.7, -12.7)
    assert h[[0, 30, 31, 179]].tolist() == [149, 179, 0, 148]          # mod(i - 30.5, 180), truncated
    assert s[[0, 250, 255]].tolist() == [12, 255, 255] and v[[0, 12, 13, 255]].tolist() == [0, 0, 0, 242]
    rec = augment.plan_records([{"colour": {"op": augment.COLOUR_OPS[0], "alpha": 1.3, "beta": 0.3, "gamma": 0.8, "hue": 0.0, "sat": 0.0,
                                            "val": 0.0}, "quality": None, "noise": None}])
    assert rec["colour"][0] == 3
    assert np.array_equal(rec["rgb_lut"][0], augment.gamma_lut(0.8)[augment.brightness_contrast_lut(1.3, 0.3)])


def test_quant_tables_match_ijg_scaling(fixture):
    for q in QUALITIES:
        assert np.array_equal(augment.jpeg_quant_tables(q), fixture["quant_q%d" % q])
    assert augment.jpeg_quant_tables(100).max() == 1 and augment.jpeg_quant_tables(1).max() == 255          # force_baseline clamp
    assert augment.jpeg_quant_tables(50)[0, :3].tolist() == [16, 11, 10]


def test_frame_record_layout_matches_the_library():
    assert ea._lib.load().endo_augment_frame_bytes() == augment.FRAME_DTYPE.itemsize == 1344


def test_bad_arguments_are_refused_before_any_launch():
    """endo_augment checks its arguments on the host.  Every call below also hands a workspace one byte short, so that none of them
    can reach a launch: a bad record returns ENDO_E_UNSUPPORTED (checked first), everything else ENDO_E_BADARG."""
    lib = ea._lib.load()
    fake = ctypes.c_void_p(256)
    need = lib.endo_augment_workspace_bytes(1, 8, 8)
    assert need > 0 and lib.endo_augment_workspace_bytes(1, 3, 8) == -1 and lib.endo_augment_workspace_bytes(0, 8, 8) == -1

    def call(rec, src=fake, h=8, w=8, out=fake):
        return lib.endo_augment(src, ctypes.c_void_p(rec.ctypes.data), len(rec), h, w, out, None, fake, need - 1, None)

    base = {"colour": None, "quality": None, "noise": None}
    assert call(augment.plan_records([base])) == -1          # the short workspace
    for code, value in (("ksize", 4), ("ksize", 9), ("ksize", 1), ("spatial", 4), ("colour", 4), ("noise", 3), ("jpeg", 2)):
        rec = augment.plan_records([dict(base, quality={"op": "blur", "ksize": 3})])
        rec[code] = value
        assert call(rec) == -2, (code, value)
    rec = augment.plan_records([dict(base, quality={"op": "motion_blur", "ksize": 3, "kernel": np.eye(3)})])
    rec["motion"] = 0
    assert call(rec) == -2
    rec["motion"] = [1 << 9, 0]          # a tap outside the 3 x 3 mask
    assert call(rec) == -2
    rec = augment.plan_records([dict(base, quality={"op": "jpeg_compression", "quality": 50})])
    rec["quant"][0, 0, 5] = 0
    assert call(rec) == -2
    rec["quant"][0, 0, 5] = 256
    assert call(rec) == -2
    for sigma in (float("nan"), -1.0, float("inf")):
        assert call(augment.plan_records([dict(base, noise={"op": "gauss_noise", "sigma": sigma, "seed": 1})])) == -2
    ok = augment.plan_records([base])
    assert call(ok, src=None) == -1 and call(ok, out=None) == -1 and call(ok, h=2) == -1
    with pytest.raises(ValueError):
        augment.plan_records([dict(base, quality={"op": "median_blur", "ksize": 9})])


# ---------------------------------------------------------------------------------------------
# JPEG encoder restatement against libjpeg-turbo's files
# ---------------------------------------------------------------------------------------------
def entropy_decode(raw):
    lib = ea._lib.load()
    buf = np.frombuffer(raw, np.uint8)
    info = np.zeros(16, np.int32)
    assert lib.endo_jpeg_info(ctypes.c_void_p(buf.ctypes.data), len(raw), ctypes.c_void_p(info.ctypes.data)) == 0
    total = int(info[13])
    blocks = np.zeros((total, 64), np.int16)
    quant = np.zeros((3, 64), np.uint16)
    assert lib.endo_jpeg_entropy_decode(ctypes.c_void_p(buf.ctypes.data), len(raw), ctypes.c_void_p(blocks.ctypes.data), total,
                                        ctypes.c_void_p(quant.ctypes.data)) == 0
    planes, off = [], 0
    for c in range(3):
        bw, bh = int(info[7 + 2 * c]), int(info[8 + 2 * c])
        planes.append(blocks[off:off + bw * bh].reshape(bh, bw, 8, 8))
        off += bw * bh
    return info, planes, quant


@pytest.mark.parametrize("name", NAMES)
def test_encoder_restatement_matches_libjpeg_coefficients(fixture, name):
    """For every image and quality: jccolor + jcsample + edge expansion + jfdctint + jcdctmgr (restated) give the quantised blocks --
    dummy blocks included -- and the tables libjpeg-turbo wrote, and the restated decode of those blocks is the file's decode."""
    img = fixture["img_" + name]
    h, w = img.shape[:2]
    for q in QUALITIES:
        raw = fixture["jpg_%s_q%d" % (name, q)].tobytes()
        info, planes, quant = entropy_decode(raw)
        assert (int(info[0]), int(info[1]), int(info[3]), int(info[4])) == (w, h, 2, 2)
        tables = augment.jpeg_quant_tables(q)
        assert np.array_equal(quant[0], tables[0]) and np.array_equal(quant[1], tables[1]) and np.array_equal(quant[2], tables[1])
        mine = ar.jpeg_encode(img, tables)
        for c in range(3):
            assert np.array_equal(mine[c], planes[c]), (name, q, c)
        decoded = oreader.decode_jpeg_blocks(planes, [t.reshape(8, 8) for t in (tables[0], tables[1], tables[1])], w, h)
        assert np.array_equal(ar.jpeg_roundtrip(img, tables), np.ascontiguousarray(decoded[..., ::-1])), (name, q)


def test_fixture_script_reproduces_the_bytes(fixture, tmp_path):
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        maker = importlib.import_module("make_augment_golden")
    finally:
        sys.path.pop(0)
    fresh = maker.build()
    assert sorted(fresh) == sorted(fixture.files)
    for key in fixture.files:
        assert np.array_equal(fresh[key], fixture[key]), key


# ---------------------------------------------------------------------------------------------
# colour restatements
# ---------------------------------------------------------------------------------------------
KNOWN = np.array([[[0, 0, 255], [0, 255, 0], [255, 0, 0], [0, 255, 255], [255, 255, 0], [255, 0, 255], [0, 0, 0], [255, 255, 255],
                   [128, 128, 128], [10, 20, 40], [200, 100, 50]]], dtype=np.uint8)          # B, G, R (test_reader's known answers)


def test_hsv180_restatement_reduces_to_hsv_full():
    """With 256 in place of 180 the restated cv2.COLOR_RGB2HSV is oracle.reader.bgr_to_hsv_full's COLOR_BGR2HSV_FULL, on the
    known-answer pixels of tests/test_reader.py and on random ones."""
    rng = np.random.default_rng(3)
    for px in (KNOWN, rng.integers(0, 256, (1, 5000, 3)).astype(np.uint8)):
        assert np.array_equal(ar.rgb_to_hsv(px[..., ::-1], hrange=256), oreader.bgr_to_hsv_full(px, 0))
        assert np.array_equal(ar.rgb_to_hsv(px, hrange=256, blue_index=0), oreader.bgr_to_hsv_full(px, 0))
    hsv = ar.rgb_to_hsv(KNOWN[..., ::-1], hrange=180)[0]
    assert hsv[:6, 0].tolist() == [0, 60, 120, 30, 90, 150] and hsv[:6, 1:].min() == 255


def test_hsv180_roundtrip_of_primaries():
    """HSV2RGB of the converted primaries / secondaries / greys gives them back exactly."""
    rgb = KNOWN[..., ::-1][:, :9]
    assert np.array_equal(ar.hsv180_to_rgb(ar.rgb_to_hsv(rgb, 180)), rgb)
    assert np.array_equal(ar.shift_hsv(rgb, augment.hsv_luts(0, 0, 0)), rgb)


def test_spatial_restatements_basic_identities():
    rng = np.random.default_rng(0)
    flat = np.full((9, 11, 3), 77, np.uint8)
    img = rng.integers(0, 256, (9, 11, 3)).astype(np.uint8)
    for k in (3, 5, 7):
        assert np.array_equal(ar.box_blur(flat, k), flat) and np.array_equal(ar.median_blur(flat, k), flat)
        point = np.zeros((k, k), np.uint8)
        point[k // 2, k // 2] = 1
        assert np.array_equal(ar.motion_blur(img, point), img)
        med = ar.median_blur(img, k)
        r = k // 2
        pad = np.pad(img, ((r, r), (r, r), (0, 0)), mode="edge")
        assert med[4, 5, 1] == int(np.median(pad[4:4 + k, 5:5 + k, 1]))

