"""Posed test output on the device (reference utils.py:1246-1355): endo_evaluate_posed (csrc/evaluate_posed.hip) bit for bit against the
numpy restatement (tests/evaluate_posed_restate.py, itself held to the reference by tests/golden/make_evaluate_posed_golden.py), against
the reference's recorded outputs, against endo_evaluate for an identity pose, and under poisoned, guarded buffers; then
evaluate.run_posed_test_phase end to end on the committed example sequence.  Run with ``pytest -m gpu`` on an MI355X.

Only a frame whose kept depths are all equal (scale = 20 / 0, non-finite coordinates in the reference too) is compared with equal_nan: a
NaN's payload is not part of the contract.  Everything else is compared as bits."""

import importlib
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import evaluate_posed_restate as pr
from guarded_alloc import guarded
from test_gpu_evaluate import random_batch, sequence, trained  # noqa: F401  (the two fixtures of the example sequence)

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate = ea.evaluate
THRESHOLDS = (100.0, 150.0)          # min_threshold, max_threshold


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_poses(n, seed):
    rng = np.random.default_rng(seed)
    rot = np.stack([ea.reader.quaternion_matrix(rng.standard_normal(4))[:3, :3] for _ in range(n)])
    return np.ascontiguousarray(rot, np.float64), rng.uniform(-50.0, 50.0, (n, 3))


def posed_batch(n, h, w, seed):
    """test_gpu_evaluate.random_batch (elliptical boundary with holes and empty rows, colours near the truncation edges, exact-zero
    depths, frame 1 all zeros when n >= 3: a zero z range) with the colours stretched past [-1, 1], so that the clip acts, and poses."""
    c, b, pred, kk = random_batch(n, h, w, seed)
    c = (c * np.float32(1.15)).astype(np.float32)
    rot, tr = random_poses(n, seed + 7)
    return c, b, pred, kk, rot, tr


def call_posed(c, b, pred, kk, rot, tr, is_hsv=False, ds=1, thr=None):
    """The C entry on separately allocated outputs (so that a guarded context puts bands around each); numpy copies of everything."""
    lib = ea._lib.load()
    n, _, h, w = c.shape
    d = dev()
    tin = [torch.from_numpy(np.ascontiguousarray(a, t)).to(d) for a, t in ((c, np.float32), (b, np.float32), (pred, np.float32),
                                                                           (kk, np.float32), (rot, np.float64), (tr, np.float64))]
    need = int(lib.endo_evaluate_posed_workspace_bytes(n, h, w))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=d)
    depth = torch.empty((n, 1, h, w), dtype=torch.float32, device=d)
    color = torch.empty((n, h, w, 3), dtype=torch.uint8, device=d)
    dimg = torch.empty((n, h, w, 3), dtype=torch.uint8, device=d)
    points = torch.empty((n * h * w, 6), dtype=torch.float32, device=d)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=d)
    ranges = torch.empty((n, 2), dtype=torch.float32, device=d)
    p = ea._lib.ptr
    rc = lib.endo_evaluate_posed(*[p(t) for t in tin], n, h, w, int(is_hsv), ds, 0 if thr is None else 1, 0.0 if thr is None else thr[0],
                                 0.0 if thr is None else thr[1], p(depth), p(color), p(dimg), p(points), p(offsets), p(ranges), p(ws), need,
                                 ea._lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {"depth": depth.cpu().numpy(), "color": color.cpu().numpy(), "depth_images": dimg.cpu().numpy(), "points": points.cpu().numpy(),
            "offsets": offsets.cpu().tolist(), "ranges": ranges.cpu().numpy()}


def check(got, c, b, pred, kk, rot, tr, is_hsv=False, ds=1, thr=None):
    n = c.shape[0]
    lo, hi = (None, None) if thr is None else thr
    depth, color, dimg, clouds, ranges = pr.batch_outputs(c, b, pred, kk, rot, tr, is_hsv, ds, lo, hi)
    assert np.array_equal(bits(got["depth"]), bits(depth))
    assert np.array_equal(got["color"], color)
    assert np.array_equal(got["depth_images"], dimg)
    assert np.array_equal(bits(got["ranges"]), bits(ranges))
    off = got["offsets"]
    assert off[0] == 0 and len(off) == n + 1
    for f in range(n):
        rows = got["points"][off[f]:off[f + 1]]
        assert rows.shape == clouds[f].shape, (f, rows.shape, clouds[f].shape)
        if ranges[f, 0] == ranges[f, 1]:
            assert np.array_equal(rows, clouds[f], equal_nan=True) and (~np.isfinite(rows[:, :3])).any(axis=1).all(), f
        else:
            assert np.array_equal(bits(rows), bits(clouds[f])), f
            assert np.isfinite(rows).all(), f
    return clouds, ranges


@pytest.mark.parametrize("ds,is_hsv,thr", [(1, False, None), (2, True, None), (3, False, THRESHOLDS), (1, True, THRESHOLDS),
                                           (2, False, THRESHOLDS)])
def test_small_frames_match_restatement(ds, is_hsv, thr):
    """(3, 7, 9): the downsampling predicate, both colour paths, the written set smaller than the kept set; frame 1 has a zero z range."""
    args = posed_batch(3, 7, 9, seed=40 + ds)
    clouds, ranges = check(call_posed(*args, is_hsv=is_hsv, ds=ds, thr=thr), *args, is_hsv=is_hsv, ds=ds, thr=thr)
    assert ranges[1, 0] == ranges[1, 1] == 0 and ranges[0, 0] < ranges[0, 1]
    if thr is not None:
        plain = pr.batch_outputs(*args, is_hsv, ds)[3]
        assert 0 < len(clouds[0]) < len(plain[0])


@pytest.mark.parametrize("shape", [(2, 5, 255), (2, 5, 256), (2, 5, 257), (1, 3, 520)])
def test_chunk_loop_widths(shape):
    """Rows narrower than, equal to and wider than the 256-wide chunk: the write kernel's running base."""
    args = posed_batch(*shape, seed=sum(shape))
    check(call_posed(*args, thr=THRESHOLDS), *args, thr=THRESHOLDS)
    check(call_posed(*args, is_hsv=True, ds=2), *args, is_hsv=True, ds=2)


def test_more_rows_than_scan_threads():
    """17 x 61 = 1037 rows, more than the scan block's 1024 threads; 17 frames, more than its 16 waves."""
    args = posed_batch(17, 61, 9, seed=17)
    check(call_posed(*args), *args)


def test_empty_frame_single_pixel_frame_and_empty_rows():
    n, h, w = 4, 9, 13
    c, b, pred, kk, rot, tr = posed_batch(n, h, w, seed=5)
    pred[1] = np.abs(np.random.default_rng(6).standard_normal((1, h, w)).astype(np.float32)) + np.float32(0.5)   # undo random_batch's zero frame
    b[0, 0, 3:5] = 0.0          # rows without kept pixels inside a frame
    b[1] = 0.0                  # an empty frame between two non-empty ones
    b[2] = 0.0
    b[2, 0, 4, 6] = 1.0         # exactly one kept pixel
    c = (b * c).astype(np.float32)
    got = call_posed(c, b, pred, kk, rot, tr)
    clouds, ranges = check(got, c, b, pred, kk, rot, tr)
    off = got["offsets"]
    assert off[1] > 0 and off[2] == off[1] and off[3] == off[2] + 1 and off[4] > off[3]          # continuous across the empty frame
    assert np.isposinf(got["ranges"][1, 0]) and np.isneginf(got["ranges"][1, 1])
    assert got["ranges"][2, 0] == got["ranges"][2, 1] == pred[2, 0, 4, 6] > 0
    assert len(clouds[2]) == 1 and not np.isfinite(got["points"][off[2], :3]).all()
    # downsampling 2 keeps only even rows and columns: odd rows are rows without kept pixels
    check(call_posed(c, b, pred, kk, rot, tr, ds=2, thr=THRESHOLDS), c, b, pred, kk, rot, tr, ds=2, thr=THRESHOLDS)


def test_fixture_records_through_the_c_abi(golden):
    """The reference's own recorded outputs (tests/golden/evaluate_posed.npz) from the device."""
    g = golden("evaluate_posed.npz")
    c, b, pred, kk = (g["whole::" + n] for n in ("colors", "boundaries", "predictions", "intrinsics"))
    keys = [str(k) for k in g["readers::initial_keys"]]
    at = [keys.index(str(n)) for n in g["whole::names"]]
    rot, tr = g["readers::initial_rotations"][at], g["readers::initial_translations"][at]
    got = call_posed(c, b, pred, kk, rot, tr)
    off = got["offsets"]
    for f in range(c.shape[0]):
        assert np.array_equal(bits(got["points"][off[f]:off[f + 1]]), bits(g["whole::cloud_%d" % f])), f
        assert np.array_equal(got["color"][f], g["whole::color_%d" % f]), f
        assert np.array_equal(got["depth_images"][f], pr.er.JET[g["whole::depth_index_%d" % f]]), f
    one = [a[:1] for a in (c, b, pred, kk, rot, tr)]
    got = call_posed(*one, ds=2)
    assert np.array_equal(bits(got["points"][:got["offsets"][1]]), bits(g["ds2::cloud"]))
    got = call_posed(*one, thr=tuple(float(v) for v in g["thr::thresholds"]))
    assert np.array_equal(bits(got["points"][:got["offsets"][1]]), bits(g["thr::cloud"]))
    # the same records through the host interface of one frame
    depth0 = (b[0, 0] * pred[0, 0]).astype(np.float32)
    for ds, thr, key in ((1, (None, None), "whole::cloud_0"), (2, (None, None), "ds2::cloud"), (1, tuple(g["thr::thresholds"]), "thr::cloud")):
        rows = ea.utils.point_cloud_from_depth_and_initial_pose(depth0[:, :, None], g["whole::color_0"], b[0, 0][:, :, None], kk[0], tr[0],
                                                                rot[0], ds, min_threshold=thr[0], max_threshold=thr[1])
        assert rows.dtype == np.float32 and np.array_equal(bits(rows), bits(g[key])), key
    with pytest.raises(ZeroDivisionError):
        ea.utils.point_cloud_from_depth_and_initial_pose(depth0, g["whole::color_0"], np.zeros_like(depth0), kk[0], tr[0], rot[0], 1)
    assert np.array_equal(ea.utils.display_depth_map(depth0[:, :, None]), pr.er.JET[g["whole::depth_index_0"]])
    with pytest.raises(NotImplementedError):
        ea.utils.display_depth_map(depth0, 0.0, 1.0)


def test_identity_pose_is_endo_evaluate_times_the_scale():
    """A check that does not pass through the restatement: with R = I and t = 0 the fp64 transform is exact (up to -0 + 0 = +0), so
    xyz equals endo_evaluate's xyz times the float32 scale 20 / (z_max - z_min)."""
    n, h, w = 2, 16, 24
    c, b, pred, kk = random_batch(n, h, w, seed=21)
    rot, tr = np.broadcast_to(np.eye(3), (n, 3, 3)).copy(), np.zeros((n, 3))
    got = call_posed(c, b, pred, kk, rot, tr, ds=2)
    t = [torch.from_numpy(a).to(dev()) for a in (c, b, pred, kk)]
    plain = evaluate.outputs_from_predictions(*t, is_hsv=False, point_cloud_downsampling=2)
    assert plain["offsets"] == got["offsets"] and got["offsets"][-1] > 20
    points = plain["points"].cpu().numpy()
    for f in range(n):
        rows = points[plain["offsets"][f]:plain["offsets"][f + 1], :3]
        z_min, z_max = got["ranges"][f]
        assert z_min == rows[:, 2].min() and z_max == rows[:, 2].max() and z_max > z_min
        scale = np.float32(20.0) / (z_max - z_min)
        want = ((rows * scale).astype(np.float64) + 0.0).astype(np.float32)
        assert np.array_equal(bits(got["points"][got["offsets"][f]:got["offsets"][f + 1], :3]), bits(want)), f


def test_poisoned_buffers_and_guard_bands():
    """Outputs and workspace 0xFF-filled (NaN / -1) before the call give what zero-filled ones give; nothing is written outside a
    buffer (the context checks every guard band on exit); point rows behind frame_offsets[N] keep what they held."""
    args = posed_batch(3, 11, 300, seed=3)
    runs = {}
    for fill in ("poison", "zeros"):
        with guarded(device="cuda", fill=fill) as alloc:
            runs[fill] = call_posed(*args, is_hsv=True, ds=2, thr=THRESHOLDS)
            assert alloc.check() >= 7
    a, z = runs["poison"], runs["zeros"]
    total = a["offsets"][-1]
    assert a["offsets"] == z["offsets"] and 0 < total < len(a["points"])
    for key in ("depth", "color", "depth_images", "ranges"):
        assert np.array_equal(a[key].view(np.uint8), z[key].view(np.uint8)), key
    assert np.array_equal(a["points"][:total].view(np.uint8), z["points"][:total].view(np.uint8))
    assert np.all(a["points"][total:].view(np.uint8) == 0xFF) and np.all(z["points"][total:].view(np.uint8) == 0)
    check(z, *args, is_hsv=True, ds=2, thr=THRESHOLDS)


def test_bad_arguments():
    lib = ea._lib.load()
    # N = 1, 2 x 2.  The inputs may share one block of zeros; every output and the workspace has a block of its own: the scan writes
    # frame_ranges = (+inf, -inf), and an output aliased with the boundaries or the row offsets would steer the write kernel's addresses.
    x = torch.zeros(1024, device=dev())
    p = ea._lib.ptr(x)
    s = ea._lib.stream()
    need = int(lib.endo_evaluate_posed_workspace_bytes(1, 2, 2))
    assert 0 < need <= 4096
    outs = [torch.zeros(1024, device=dev()) for _ in range(7)]          # depth, two images, points, offsets, ranges, workspace
    o = [ea._lib.ptr(t) for t in outs]
    args = [p, p, p, p, p, p, 1, 2, 2, 0, 1, 0, 0.0, 0.0] + o + [need, s]
    assert lib.endo_evaluate_posed(*args) == 0
    for i, bad in ((0, None), (4, None), (5, None), (6, 0), (6, 65536), (8, 0), (9, 2), (10, 0), (11, 2), (15, None), (19, None), (20, None),
                   (21, need - 1)):
        a = list(args)
        a[i] = bad
        assert lib.endo_evaluate_posed(*a) == -1, i
    a = list(args)
    a[11], a[12] = 1, float("nan")
    assert lib.endo_evaluate_posed(*a) == -1
    torch.cuda.synchronize()


def read_png(path):
    """utils.write_png's files back as (H, W, 3) uint8 R, G, B: colour type 2, 8 bits, filter type 0 on every row."""
    data = open(str(path), "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        (length,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        if kind == b"IHDR":
            size = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + length
    width, height = size[:2]
    assert size[2:] == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(height, 1 + 3 * width)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(height, width, 3)


def read_ply(path):
    head, body = open(str(path)).read().split("end_header\n")
    rows = np.array([[float(v) for v in line.split(" ")] for line in body.splitlines()], np.float64).reshape(-1, 6)
    assert "element vertex %d\n" % len(rows) in head
    return rows.astype(np.float32)


def test_run_posed_test_phase_on_the_example_sequence(sequence, trained, tmp_path):
    model, _ = trained
    model.eval()
    names = ea.utils.get_filenames_from_frame_indexes(os.path.dirname(sequence), ea.reader.read_visible_view_indexes(sequence))
    names = [str(p) for p in names]
    frames = ea.dataset.TestFrames(names, batch_size=2, suggested_h=256, suggested_w=320)
    pose_file = tmp_path / "initial_poses"
    pose_file.write_text("4594, 10.5, -3.25, 7.0, 0.5, 0.5, -0.5, 0.5\n4584, -1.5, 2.0, 30.0, 0.9, 0.1, 0.3, -0.2\n")
    indexes, translations, rotations = ea.reader.read_initial_pose_file(pose_file)
    assert indexes == [4584, 4594] and sorted(rotations) == ["00004584", "00004594"]
    missing = dict(rotations)
    del missing["00004594"]
    with pytest.raises(KeyError):
        evaluate.run_posed_test_phase(model, frames, translations, missing, tmp_path / "never")
    assert not (tmp_path / "never").exists()          # raised before anything ran
    (batch,) = list(frames)
    assert batch["names"] == ["00004584", "00004594"]
    out = evaluate.posed_test_outputs(model, batch, [rotations[n] for n in batch["names"]], [translations[n] for n in batch["names"]])
    off = out["offsets"]
    points = out["points"][:off[-1]].cpu().numpy()
    assert off[1] > 1000 and off[2] - off[1] == off[1] and np.isfinite(points).all()          # the two frames share the boundary
    assert np.all(out["ranges"][:, 0] < out["ranges"][:, 1])
    # the device rows are the restatement's on the device's own predictions
    want = pr.batch_outputs(out["colors"].cpu().numpy(), batch["boundaries"].cpu().numpy(), out["predictions"].cpu().numpy(),
                            batch["intrinsics"].cpu().numpy(), np.stack([rotations[n] for n in batch["names"]]),
                            np.stack([translations[n] for n in batch["names"]]))
    for f in range(2):
        assert np.array_equal(bits(points[off[f]:off[f + 1]]), bits(want[3][f])), f
        # a cloud normalised to a z range of 20 units, then moved rigidly: its extent along the camera's z axis is 20
        back = (points[off[f]:off[f + 1], :3].astype(np.float64) - translations[batch["names"][f]]) @ rotations[batch["names"][f]]
        assert abs((back[:, 2].max() - back[:, 2].min()) - 20.0) < 1e-3
    out_dir = tmp_path / "out"
    result = evaluate.run_posed_test_phase(model, frames, translations, rotations, out_dir)
    assert result == {"frames": 2, "empty": [], "zero_range": [], "merged_points": off[-1]}
    for f, name in enumerate(batch["names"]):
        assert np.array_equal(bits(read_ply(out_dir / ("test_point_cloud_%s.ply" % name))), bits(points[off[f]:off[f + 1]])), name
        # write_png takes cv2's B, G, R and stores R, G, B: the file's channels are the image's, reversed
        assert np.array_equal(read_png(out_dir / ("test_color_%s.png" % name))[:, :, ::-1], out["color_images"][f].cpu().numpy()), name
        assert np.array_equal(read_png(out_dir / ("test_depth_%s.png" % name))[:, :, ::-1], out["depth_images"][f].cpu().numpy()), name
        assert np.array_equal(out["color_images"][f].cpu().numpy(), want[1][f]) and np.array_equal(out["depth_images"][f].cpu().numpy(), want[2][f])
    assert np.array_equal(bits(read_ply(out_dir / "sequence.ply")), bits(points))          # the merged cloud: their concatenation
    # no files, no merged cloud: the count only
    assert evaluate.run_posed_test_phase(model, frames, translations, rotations, tmp_path / "none", write_images=False, write_ply=False)[
        "frames"] == 2
    assert list((tmp_path / "none").iterdir()) == []
