"""evaluate.model_depth_errors / run_model_depth_phase end to end against a mesh whose depth is known: a stand-in network whose
predictions are the restated render of the test mesh at the tracker's poses, each frame times its own factor.  The same composition
with the restatements on the CPU (tests/mesh_render_restate.py, tests/evaluate_posed_restate.py, tests/registration_restate.py) gives
the figures the device is held to.  Run with ``pytest -m gpu`` on an MI355X."""
import csv
import importlib
import struct

import numpy as np
import pytest
import torch

import evaluate_posed_restate as pr
import mesh_render_restate as mr
import registration_restate as rr

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate, mesh = ea.evaluate, ea.mesh
H, W = 37, 53
FACTORS = (0.6, 1.7, 3.0, 0.9, 12.0)
# the tracker-to-model similarity, known: x_model = sigma Q x_tracker + tau
TRUTH = (1.3, rr.rotation_about((0.3, -1.0, 0.5), 25.0), np.array([4.0, -2.5, 7.0]))
EPS = 1.0e-8


class Predictions(object):
    """A stand-in for the network in eval mode: the sequence's depth maps, batch after batch."""
    training = False

    def __init__(self, batches):
        self.batches, self.calls = batches, 0

    def __call__(self, masked):
        self.calls += 1
        return self.batches[self.calls - 1]


class Batches(list):
    """A stand-in for dataset.TestFrames: the batches, and the file names the phases check the pose keys of."""
    image_file_names = []


_sequences = {}


def sequence(fine):
    """The tube (fine: 24 x 36 quads, enough vertices for ICP), five cameras inside it in the model's frame, their poses in the
    tracker's frame under TRUTH, and the restated render from there: made once and left unchanged."""
    if fine not in _sequences:
        vertices, faces = mr.tube(24, 36) if fine else mr.tube()
        eyes = [(0.0, 0.0, 0.6), (0.2, -0.1, 0.9), (-0.1, 0.2, 1.3), (0.1, 0.1, 1.7), (0.0, -0.2, 2.1)]
        targets = [(0.2, 0.0, 4.0), (0.0, 0.3, 4.0), (0.5, 0.0, 4.0), (0.3, -0.2, 4.0), (0.6, 0.1, 4.0)]
        model_rot = np.stack([mr.look_at(e, t) for e, t in zip(eyes, targets)])
        sigma, q, tau = TRUTH
        rotations = np.stack([q.T @ r for r in model_rot])
        translations = np.stack([q.T @ (np.asarray(e) - tau) / sigma for e in eyes])
        k = np.stack([mr.intrinsics(30.0, H, W)] * 5)
        seen = composed(vertices, faces, k, rotations, translations, [TRUTH] * 5)
        _sequences[fine] = dict(vertices=vertices, faces=faces, k=k, rotations=rotations, translations=translations, seen=seen,
                                names=["%08d" % (200 + f) for f in range(5)])
    return _sequences[fine]


def composed(vertices, faces, k, rotations, translations, transforms, boundaries=None):
    """The restated render at the poses evaluate places the cameras at in the model's frame."""
    rot, tr = evaluate._model_poses(rotations, translations, list(transforms), len(rotations))
    return mr.render(vertices, faces, k, rot, tr, H, W, boundaries=boundaries)


def restated_errors(predictions, seen):
    """models.DepthScalingLayer and losses.depth_metrics' abs rel in numpy: per-pixel float32, sums in float64."""
    scale, abs_rel = [], []
    for pred, depth, mask in zip(predictions[:, 0], seen["depth"][:, 0], seen["mask"][:, 0]):
        hit = mask > 0
        ratio = (depth[hit] / (np.float32(EPS) + pred[hit])).astype(np.float64)
        s = np.float32(ratio.sum() / (EPS + hit.sum()))
        scaled = s * pred[hit]
        scale.append(float(s))
        abs_rel.append(float((np.abs(scaled - depth[hit]) / (np.float32(EPS) + depth[hit])).astype(np.float64).mean()))
    return np.array(scale), np.array(abs_rel)


def batches_of(seq, predictions, boundaries, picks=(slice(0, 3), slice(3, 5))):
    d = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    batches, outputs = Batches(), []
    for pick in picks:          # a batch of three and one of two
        count = len(seq["names"][pick])
        batches.append({"names": seq["names"][pick], "colors": torch.from_numpy(rng.uniform(-1, 1, (count, 3, H, W)).astype(np.float32)).to(d),
                        "boundaries": torch.from_numpy(boundaries[pick]).to(d), "intrinsics": torch.from_numpy(seq["k"][pick]).to(d)})
        outputs.append(torch.from_numpy(predictions[pick]).to(d))
    batches.image_file_names = ["/data/sequence/%s.jpg" % name for pick in picks for name in seq["names"][pick]]
    return batches, Predictions(outputs)


def read_table(path):
    with open(str(path)) as f:
        return list(csv.reader(f))


def png_shape(path):
    with open(str(path), "rb") as f:
        head = f.read(26)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    width, height = struct.unpack(">II", head[16:24])
    return height, width, head[24], head[25]


def test_the_phase_recovers_each_frames_factor(tmp_path):
    """refine=False with the known similarity as ``initial``: every covered pixel's scaled prediction is the rendered depth up to
    float32 rounding, so sigma 1, 2, 3 are exactly 1, the scale is 1 / factor to 4 ulp, and abs rel is within 4 x what the same
    composition gives with the restatements on the CPU -- measured there: 1.5e-08 .. 2.8e-08 over the five frames (the rounding of
    render x factor and of scale x prediction, half an ulp each on average)."""
    seq = sequence(False)
    seen = seq["seen"]
    assert seen["mask"].mean() > 0.5
    factors = np.asarray(FACTORS, np.float32)
    predictions = seen["depth"] * factors[:, None, None, None]
    boundaries = np.ones((5, 1, H, W), np.float32)
    boundaries[:, :, :2, :] = 0.0
    want = composed(seq["vertices"], seq["faces"], seq["k"], seq["rotations"], seq["translations"], [TRUTH] * 5, boundaries[:, 0])
    want_scale, want_abs_rel = restated_errors(predictions, want)
    print("restated abs rel per frame: %s" % ", ".join("%.3e" % v for v in want_abs_rel))
    batches, model = batches_of(seq, predictions, boundaries)
    rotations = {name: seq["rotations"][f] for f, name in enumerate(seq["names"])}
    translations = {name: seq["translations"][f] for f, name in enumerate(seq["names"])}
    model_mesh = mesh.TriangleMesh(seq["vertices"], seq["faces"])

    missing = dict(rotations)
    del missing[seq["names"][3]]
    with pytest.raises(KeyError):
        evaluate.run_model_depth_phase(model, batches, translations, missing, model_mesh, tmp_path / "never", initial=TRUTH)
    assert not (tmp_path / "never").exists() and model.calls == 0          # raised before anything ran

    out_dir = tmp_path / "out"
    result = evaluate.run_model_depth_phase(model, batches, translations, rotations, model_mesh, out_dir, initial=TRUTH)
    assert model.calls == 2 and result["frames"] == 5 and result["failed"] == [] and result["covered"] == 5
    assert sorted(p.name for p in out_dir.iterdir()) == ["model_depth_%s.png" % name for name in seq["names"]] + ["model_depth_errors.csv"]
    table = read_table(out_dir / "model_depth_errors.csv")
    assert tuple(table[0]) == evaluate.MODEL_DEPTH_COLUMNS == ("name", "pixels", "scale", "abs_rel", "sigma_1", "sigma_2", "sigma_3")
    assert [row[0] for row in table[1:]] == seq["names"] and len(table) == 6
    for f, (row, kept) in enumerate(zip(table[1:], result["rows"])):
        print("model depth of %s" % ", ".join(row))
        assert (row[0], int(row[1])) == kept[:2] and [float(v) for v in row[2:]] == list(kept[2:])
        assert int(row[1]) == int(want["mask"][f].sum()) > 1000
        assert [float(v) for v in row[4:]] == [1.0, 1.0, 1.0]
        assert abs(float(row[2]) * float(factors[f]) - 1.0) <= 4.0 * 2.0 ** -23
        assert abs(float(row[2]) - want_scale[f]) <= 2.0 ** -22 * want_scale[f]
        assert float(row[3]) <= 4.0 * want_abs_rel[f], (float(row[3]), want_abs_rel[f])
        assert png_shape(out_dir / ("model_depth_%s.png" % row[0])) == (H, 2 * W, 8, 2)
    assert np.abs(result["mean_metrics"][1:] - 1.0).max() == 0.0

    # the function itself: the rendered maps are the restatement's at the composed poses, byte for byte
    d = torch.device("cuda:0")
    out = evaluate.model_depth_errors(torch.from_numpy(predictions).to(d), torch.from_numpy(boundaries).to(d), torch.from_numpy(seq["k"]).to(d),
                                      seq["rotations"], seq["translations"], model_mesh, TRUTH)
    for name in ("depth", "mask", "triangle", "barycentric", "normals"):
        assert out[name].cpu().numpy().tobytes() == want[name].tobytes(), name
    assert out["metrics"].shape == (5, 4) and out["pixels"].cpu().tolist() == [float(want["mask"][f].sum()) for f in range(5)]
    assert out["scaled"].shape == (5, 1, H, W) and out["scale"].dtype == torch.float64
    # without images, and a frame the model does not cover: NaN in its row, nothing raises
    far = dict(translations)
    far[seq["names"][0]] = translations[seq["names"][0]] + 500.0
    batches, model = batches_of(seq, predictions, boundaries)
    result = evaluate.run_model_depth_phase(model, batches, far, rotations, model_mesh, tmp_path / "bare", initial=TRUTH, write_images=False)
    assert sorted(p.name for p in (tmp_path / "bare").iterdir()) == ["model_depth_errors.csv"]
    assert result["covered"] == 4 and result["rows"][0][1] == 0 and all(np.isnan(v) for v in result["rows"][0][2:])


REFINED = 3          # the frames of the refine test: the restated ICP on the CPU is what the test's time goes to


def restated_refine():
    """The refine=True composition with the restatements alone: (predictions, boundaries, start, keyword arguments, abs rel per frame
    with refine, abs rel per frame from the truth)."""
    seq = sequence(True)
    factors = np.asarray(FACTORS, np.float32)
    predictions = (seq["seen"]["depth"] * factors[:, None, None, None])[:REFINED]
    boundaries = seq["seen"]["mask"][:REFINED].copy()          # the posed clouds hold pixels the tube covers and no others
    boundaries[:, :, :2, :] = 0.0
    boundaries[:, :, 0::2, 1::2] = 0.0                         # every other one of them, as a checkerboard
    boundaries[:, :, 1::2, 0::2] = 0.0
    sigma, q, tau = TRUTH
    start = (sigma * 1.01, rr.rotation_about((0.0, 1.0, 0.3), 1.0) @ q, tau + 0.05)
    kw = dict(iterations=20)
    pose = (seq["k"][:REFINED], seq["rotations"][:REFINED], seq["translations"][:REFINED])
    first = composed(seq["vertices"], seq["faces"], *pose, [start] * REFINED, boundaries[:, 0])
    first_scale, _ = restated_errors(predictions, first)
    transforms = []
    for f in range(REFINED):
        depth = boundaries[f, 0] * predictions[f, 0]
        cloud = pr.point_cloud(depth, np.zeros((H, W, 3), np.uint8), boundaries[f, 0], seq["k"][f], seq["translations"][f], seq["rotations"][f])
        fit = rr.register(cloud[:, :3], seq["vertices"], *evaluate._cloud_start(start, seq["translations"][f], first_scale[f],
                                                                                 pr.frame_range(depth, boundaries[f, 0], 1)), **kw)
        transforms.append((fit["scale"], fit["rotation"], fit["translation"]))
    want = composed(seq["vertices"], seq["faces"], *pose, transforms, boundaries[:, 0])
    plain = composed(seq["vertices"], seq["faces"], *pose, [TRUTH] * REFINED, boundaries[:, 0])
    return predictions, boundaries, start, kw, restated_errors(predictions, want)[1], restated_errors(predictions, plain)[1]


def test_refining_each_frame_by_registration(tmp_path):
    """refine=True on the fine tube (24 x 36 quads, 900 vertices) from a start 1 degree, 0.05 units and 1 % off the known similarity:
    every frame's posed cloud registers to the model's vertices, and each frame's abs rel stays within 4 x what the same composition
    gives on the CPU with the restated posed cloud, the restated ICP and the restated render.  Measured there: abs rel 2.99e-03, 5.76e-03 and 3.59e-03 for
    the three frames -- closest points are taken among the vertices, not on the triangles between them, so a frame lands a fraction of the
    vertex spacing from where it was seen -- against 1.4e-08 .. 3.1e-08 from the truth without refine: a margin of about 2e+05, which
    is the fit's, not the renderer's."""
    seq = sequence(True)
    factors = np.asarray(FACTORS, np.float32)
    predictions, boundaries, start, kw, want_abs_rel, plain_abs_rel = restated_refine()
    print("restated abs rel per frame with refine: %s; without, from the truth: %s; margin %s" % (
        ", ".join("%.3e" % v for v in want_abs_rel), ", ".join("%.3e" % v for v in plain_abs_rel),
        ", ".join("%.2e" % v for v in want_abs_rel / plain_abs_rel)))
    batches, model = batches_of(seq, predictions, boundaries, (slice(0, 2), slice(2, REFINED)))
    rotations = {name: seq["rotations"][f] for f, name in enumerate(seq["names"])}
    translations = {name: seq["translations"][f] for f, name in enumerate(seq["names"])}
    model_mesh = mesh.TriangleMesh(seq["vertices"], seq["faces"])
    result = evaluate.run_model_depth_phase(model, batches, translations, rotations, model_mesh, tmp_path / "out", initial=start, refine=True,
                                            write_images=False, **kw)
    assert result["frames"] == REFINED and result["failed"] == [] and result["covered"] == REFINED
    for f, row in enumerate(result["rows"]):
        print("refined model depth of %s" % ", ".join(str(v) for v in row))
        assert row[1] > 400 and row[3] <= 4.0 * want_abs_rel[f], (row[3], want_abs_rel[f])
        assert abs(row[2] * float(factors[f]) - 1.0) < 0.05          # (the start was 1 % off; the fit ends nearer)
