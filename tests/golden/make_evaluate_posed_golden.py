"""Writes tests/golden/evaluate_posed.npz and the small text inputs under tests/golden/posed/: inputs and the outputs of the reference's
own posed test output -- utils.write_test_output_with_initial_pose (utils.py:1316-1355), utils.point_cloud_from_depth_and_initial_pose
(1246-1295), utils.display_depth_map (773-781) up to its index image, and the readers read_initial_pose_file (1385-1402),
read_pose_messages_from_tracker (1298-1313), read_pose_corresponding_image_indexes[_and_time_difference] (1747-1770) and
read_camera_to_tcp_transform (1887-1897) -- run unmodified.

    python tests/golden/make_evaluate_posed_golden.py <directory of the reference checkout>

Needs the reference, so it is run where that exists and not by the test suite; only inputs and recorded outputs are written, no
reference source is stored.  The missing imports are stubbed as make_golden.py does (its import_reference).  Three more process-local
stand-ins, none of which touches the reference's text:

  * the ``np`` name of the reference's utils module is a proxy of numpy whose ``array`` unwraps the size-1 arrays inside a list of
    tuples: point_cloud_from_depth_and_initial_pose collects rows of (1,) arrays (depth_map[h, w] of an (H, W, 1) map) and numpy 2
    refuses ``np.array(rows, dtype='float32')`` for them; and whose ``float`` is Python's (``np.float`` left numpy in 1.24);
  * ``cv2.applyColorMap`` returns its input (display_depth_map's uint8 index image, what COLORMAP_JET is applied to) and ``cv2.imwrite``
    records its arguments;
  * ``utils.write_point_cloud`` (plyfile) records its arguments.

The recorded arithmetic is numpy 2's: with weak Python scalars ``20.0 / (z_max - z_min)`` is a float32.  Under the numpy of the
reference's time it was a float64, which moves a coordinate by about one float32 ulp before the transform.

Records, keys ``<record>::<name>``:

  whole (N = 2, 7 x 9, RGB): write_test_output_with_initial_pose on masked colours in [-1.2, 1.2] (so the clip acts), a {0, 1} boundary
      at about 70 %, positive predictions, intrinsics, and the poses read from posed/initial_poses by the reference's reader.  Per
      frame f: cloud_f (downsampling 1, no thresholds), color_f (what cv2.imwrite got), depth_index_f.
  ds2: point_cloud_from_depth_and_initial_pose on frame 0 of the same batch with the reference's own colour image, downsampling 2.
  thr: the same at downsampling 1 with min_threshold 100, max_threshold 150.
  readers: the outputs of the five readers on the files under posed/.

Every record is asserted equal, bit for bit, to tests/evaluate_posed_restate.py before it is written; an empty mask is asserted to raise
ZeroDivisionError in both."""

import os
import pathlib
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (import_reference's stubs)
import evaluate_posed_restate as pr  # noqa: E402

SEED = 20241201
N, H, W = 2, 7, 9
NAMES = ["00000012", "00000007"]
MIN_THRESHOLD, MAX_THRESHOLD = 100, 150
POSED = os.path.join(HERE, "posed")
F32 = np.float32


class NumpyProxy(object):
    """numpy, except ``array`` on a list of tuples (size-1 arrays unwrapped to scalars) and ``float``."""
    float = float

    def __getattr__(self, name):
        return getattr(np, name)

    def array(self, obj, *args, **kw):
        if isinstance(obj, list) and obj and isinstance(obj[0], tuple):
            obj = [tuple(v.item() if isinstance(v, np.ndarray) and v.size == 1 else v for v in row) for row in obj]
        return np.array(obj, *args, **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def write_text_inputs():
    os.makedirs(POSED, exist_ok=True)
    rng = np.random.default_rng(SEED + 1)
    with open(os.path.join(POSED, "initial_poses"), "w") as f:
        for name in NAMES + ["00000031"]:
            q = rng.standard_normal(4)
            q /= np.linalg.norm(q)
            t = rng.uniform(-50.0, 50.0, 3)
            f.write(", ".join([str(int(name))] + ["%.9f" % v for v in list(t) + list(q)]) + "\n")
    with open(os.path.join(POSED, "tracker_poses.csv"), "w") as f:
        f.write("time,seq,stamp,frame_id,child_frame_id,x,y,z,qx,qy,qz,qw\n")
        for i in range(3):
            q = rng.standard_normal(4)
            q /= np.linalg.norm(q)
            t = rng.uniform(-0.5, 0.5, 3)
            f.write(",".join(["%d" % (1500000000 + i), "%d" % i, "%d" % (1500000000 + i), "world", "sensor"]
                             + ["%.12f" % v for v in list(t) + list(q)]) + "\n")
    with open(os.path.join(POSED, "pose_image_indexes"), "w") as f:
        f.write("".join("%d\n" % v for v in (7, 12, 31, 40)))
    with open(os.path.join(POSED, "pose_image_indexes_and_time_difference"), "w") as f:
        f.write("".join("%d, %d\n" % v for v in ((7, 3), (12, -14), (31, 0), (40, 250))))
    with open(os.path.join(POSED, "camera_to_tcp"), "w") as f:
        f.write(" ".join("%.8f" % v for v in rng.uniform(-1.0, 1.0, 12)) + "\n")


def reader_records(utils, out):
    idx, tr, rot = utils.read_initial_pose_file(os.path.join(POSED, "initial_poses"))
    keys = sorted(tr)
    assert keys == sorted(rot) and set(NAMES) <= set(keys)
    out["readers::initial_indexes"] = np.array(idx, np.int64)
    out["readers::initial_keys"] = np.array(keys)
    out["readers::initial_translations"] = np.stack([tr[k] for k in keys])
    out["readers::initial_rotations"] = np.stack([rot[k] for k in keys])
    t_list, r_list = utils.read_pose_messages_from_tracker(os.path.join(POSED, "tracker_poses.csv"))
    out["readers::tracker_translations"] = np.stack(t_list)
    out["readers::tracker_rotations"] = np.stack(r_list)
    out["readers::indexes"] = utils.read_pose_corresponding_image_indexes(os.path.join(POSED, "pose_image_indexes"))
    a, b = utils.read_pose_corresponding_image_indexes_and_time_difference(os.path.join(POSED, "pose_image_indexes_and_time_difference"))
    out["readers::indexes_2"], out["readers::time_differences"] = a, b
    r, t = utils.read_camera_to_tcp_transform(pathlib.Path(POSED))
    out["readers::camera_to_tcp_rotation"], out["readers::camera_to_tcp_translation"] = r, t
    assert out["readers::indexes"].dtype == np.float32 and a.dtype == np.int32 and r.shape == (3, 3) and t.shape == (3, 1)
    return tr, rot


def inputs():
    rng = np.random.default_rng(SEED)
    b = (rng.random((N, 1, H, W)) < 0.7).astype(F32)
    c = (b * rng.uniform(-1.2, 1.2, (N, 3, H, W)).astype(F32)).astype(F32)
    pred = rng.uniform(0.2, 3.0, (N, 1, H, W)).astype(F32)
    k = np.zeros((N, 3, 3), F32)
    k[:, 0, 0] = rng.uniform(0.8, 1.2, N) * W
    k[:, 1, 1] = rng.uniform(0.8, 1.2, N) * W
    k[:, 0, 2] = rng.uniform(0.4, 0.6, N) * W
    k[:, 1, 2] = rng.uniform(0.4, 0.6, N) * H
    k[:, 2, 2] = 1.0
    return c, b, pred, k


def main(reference):
    mg.REF = reference
    ref = mg.import_reference()
    utils = ref["utils"]
    assert os.path.dirname(os.path.abspath(utils.__file__)) == os.path.abspath(reference)
    utils.np = NumpyProxy()
    cv2 = sys.modules["cv2"]
    written, clouds = {}, {}
    cv2.applyColorMap = lambda image, mode: image
    cv2.imwrite = lambda path, image: written.__setitem__(os.path.basename(path), np.array(image))
    utils.write_point_cloud = lambda path, cloud: clouds.__setitem__(os.path.basename(path), np.array(cloud))

    write_text_inputs()
    out = {}
    tr, rot = reader_records(utils, out)
    c, b, pred, k = inputs()
    out.update({"whole::colors": c, "whole::boundaries": b, "whole::predictions": pred, "whole::intrinsics": k,
                "whole::names": np.array(NAMES)})
    with np.errstate(all="raise"):
        utils.write_test_output_with_initial_pose(pathlib.Path("."), torch.from_numpy(c), torch.from_numpy(pred), torch.from_numpy(b),
                                                  torch.from_numpy(k), False, NAMES, tr, rot)
    rots = np.stack([rot[n] for n in NAMES])
    trs = np.stack([tr[n] for n in NAMES])
    depth, want_color, _, want_clouds, _ = pr.batch_outputs(c, b, pred, k, rots, trs)
    for f, name in enumerate(NAMES):
        cloud = clouds["test_point_cloud_%s.ply" % name]
        color = written["test_color_%s.jpg" % name]
        index = written["test_depth_%s.jpg" % name].reshape(H, W)
        assert cloud.dtype == np.float32 and color.dtype == np.uint8 and index.dtype == np.uint8
        assert same(cloud, want_clouds[f]), "frame %d: the restatement's cloud differs from the reference's" % f
        assert same(color, want_color[f]), "frame %d: colour image" % f
        assert same(index, pr.depth_index(depth[f, 0])), "frame %d: depth index" % f
        out["whole::cloud_%d" % f], out["whole::color_%d" % f], out["whole::depth_index_%d" % f] = cloud, color, index
    fn = utils.point_cloud_from_depth_and_initial_pose
    d0 = depth[0].transpose(1, 2, 0)
    color0 = written["test_color_%s.jpg" % NAMES[0]]
    b0 = b[0].transpose(1, 2, 0)
    ds2 = fn(d0, color0, b0, k[0], trs[0], rots[0], 2)
    thr = fn(d0, color0, b0, k[0], trs[0], rots[0], 1, min_threshold=MIN_THRESHOLD, max_threshold=MAX_THRESHOLD)
    assert same(ds2, pr.point_cloud(depth[0, 0], color0, b[0, 0], k[0], trs[0], rots[0], 2)), "downsampling 2"
    assert same(thr, pr.point_cloud(depth[0, 0], color0, b[0, 0], k[0], trs[0], rots[0], 1, MIN_THRESHOLD, MAX_THRESHOLD)), "thresholds"
    assert 0 < len(thr) < len(out["whole::cloud_0"]) and 0 < len(ds2) < len(out["whole::cloud_0"])
    out["ds2::cloud"], out["thr::cloud"] = ds2, thr
    out["thr::thresholds"] = np.array([MIN_THRESHOLD, MAX_THRESHOLD], np.float32)
    for f_ in (fn, pr.point_cloud):          # an empty mask: the Python-int sentinels divide 20.0 by 0
        try:
            if f_ is fn:
                f_(d0, color0, np.zeros_like(b0), k[0], trs[0], rots[0], 1)
            else:
                f_(depth[0, 0], color0, np.zeros_like(b[0, 0]), k[0], trs[0], rots[0], 1)
        except ZeroDivisionError:
            continue
        raise AssertionError("an empty mask did not raise ZeroDivisionError")
    path = os.path.join(HERE, "evaluate_posed.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 100 * 1000, os.path.getsize(path)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))
    print("  rows: whole %d + %d, downsampling 2 %d, thresholds %d" % (len(out["whole::cloud_0"]), len(out["whole::cloud_1"]), len(ds2),
                                                                       len(thr)))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "utils.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
