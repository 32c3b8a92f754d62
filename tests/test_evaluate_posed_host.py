"""CPU-only checks of the posed test output (reference utils.py:1246-1402, 1747-1770, 1887-1897): the numpy restatement against the
fixture the reference's own functions wrote (tests/golden/make_evaluate_posed_golden.py), the pose readers against their recorded
outputs, and the two new C-ABI entries' presence and size checks.  No GPU compute is launched here."""

import ctypes
import importlib
import os

import numpy as np
import pytest

import evaluate_posed_restate as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSED = os.path.join(ROOT, "tests", "golden", "posed")
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
reader = ea.reader


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def g(golden):
    return golden("evaluate_posed.npz")


def poses(g):
    keys = [str(k) for k in g["readers::initial_keys"]]
    at = [keys.index(str(n)) for n in g["whole::names"]]
    return g["readers::initial_rotations"][at], g["readers::initial_translations"][at]


def test_restatement_equals_the_reference_records(g):
    c, b, pred, k = (g["whole::" + n] for n in ("colors", "boundaries", "predictions", "intrinsics"))
    rot, tr = poses(g)
    depth, color, depth_img, clouds, ranges = pr.batch_outputs(c, b, pred, k, rot, tr)
    for f in range(c.shape[0]):
        assert same(clouds[f], g["whole::cloud_%d" % f]) and len(clouds[f]) > 30, f
        assert same(color[f], g["whole::color_%d" % f]), f
        assert same(pr.depth_index(depth[f, 0]), g["whole::depth_index_%d" % f]), f
        assert ranges[f, 0] < ranges[f, 1]
    assert color.min() == 0 and color.max() == 255          # the clip acts on both sides
    assert same(pr.point_cloud(depth[0, 0], color[0], b[0, 0], k[0], tr[0], rot[0], 2), g["ds2::cloud"])
    lo, hi = g["thr::thresholds"]
    thr = pr.point_cloud(depth[0, 0], color[0], b[0, 0], k[0], tr[0], rot[0], 1, lo, hi)
    assert same(thr, g["thr::cloud"]) and 0 < len(thr) < len(clouds[0])
    with pytest.raises(ZeroDivisionError):
        pr.point_cloud(depth[0, 0], color[0], np.zeros_like(b[0, 0]), k[0], tr[0], rot[0], 1)


def test_colors_from_u8_round_trip():
    """utils.point_cloud_from_depth_and_initial_pose hands a uint8 colour image to the float entry: every byte must come back."""
    u = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    c = ea.utils._colors_from_u8(u, 1, 256)
    assert c.shape == (1, 3, 1, 256) and c.dtype == np.float32
    assert np.array_equal(pr.color_image(c[0]), u)


def test_readers_equal_the_reference_records(g):
    idx, tr, rot = reader.read_initial_pose_file(os.path.join(POSED, "initial_poses"))
    assert idx == [int(v) for v in g["readers::initial_indexes"]] and idx == sorted(idx) and all(isinstance(v, int) for v in idx)
    keys = [str(k) for k in g["readers::initial_keys"]]
    assert sorted(tr) == keys and sorted(rot) == keys
    with open(os.path.join(POSED, "initial_poses")) as fp:
        lines = {"%08d" % int(line.split(", ")[0]): np.array(line.split(", "), dtype=np.float64) for line in fp}
    for i, key in enumerate(keys):
        assert same(tr[key], g["readers::initial_translations"][i]) and tr[key].shape == (3,), key
        assert same(rot[key], g["readers::initial_rotations"][i]) and rot[key].shape == (3, 3), key
        plain = reader.quaternion_matrix(lines[key][4:])[:3, :3]
        assert np.array_equal(rot[key], plain * np.array([1.0, -1.0, -1.0])) and abs(np.linalg.det(rot[key]) - 1.0) < 1e-12   # y / z flip
    t_list, r_list = reader.read_pose_messages_from_tracker(os.path.join(POSED, "tracker_poses.csv"))
    assert isinstance(t_list, list) and isinstance(r_list, list) and len(t_list) == len(g["readers::tracker_translations"]) == 3
    for i in range(3):
        assert same(t_list[i], g["readers::tracker_translations"][i]) and same(r_list[i], g["readers::tracker_rotations"][i]), i
    assert same(reader.read_pose_corresponding_image_indexes(os.path.join(POSED, "pose_image_indexes")), g["readers::indexes"])
    a, b = reader.read_pose_corresponding_image_indexes_and_time_difference(os.path.join(POSED, "pose_image_indexes_and_time_difference"))
    assert same(a, g["readers::indexes_2"]) and same(b, g["readers::time_differences"]) and b.min() < 0
    r, t = reader.read_camera_to_tcp_transform(POSED)
    assert same(r, g["readers::camera_to_tcp_rotation"]) and same(t, g["readers::camera_to_tcp_translation"])


def test_library_exports_the_posed_entries():
    """Fails without the feature: the parent's library has neither symbol."""
    if not os.path.exists(ea._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(ea._lib.LIB_PATH)
    for name in ("endo_evaluate_posed", "endo_evaluate_posed_workspace_bytes"):
        assert hasattr(raw, name), "libendo_hip.so does not export %s" % name
        assert name in ea._lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "endo_hip.h")).read()
    assert "int endo_evaluate_posed(" in text and "int64_t endo_evaluate_posed_workspace_bytes(" in text
    assert ea._lib.load().endo_abi_version() == 7          # additive: the version stays


def test_workspace_bytes_checks_its_sizes():
    lib = ea._lib.load()
    assert lib.endo_evaluate_posed_workspace_bytes(0, 64, 96) == -1
    assert lib.endo_evaluate_posed_workspace_bytes(65536, 1, 1) == -1
    assert lib.endo_evaluate_posed_workspace_bytes(1, 64, 0) == -1
    need = lib.endo_evaluate_posed_workspace_bytes(2, 64, 96)
    assert need >= 2 * 64 * (8 + 16) + 2 * 8          # row offsets, four row statistics, two whole-map values per frame
    # argument validation happens before any device work
    assert lib.endo_evaluate_posed(*([None] * 6 + [1, 2, 2, 0, 1, 0, 0.0, 0.0] + [None] * 7 + [need, None])) == -1
