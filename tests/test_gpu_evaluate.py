"""Test phase on the device (reference evaluate.py:279-346): endo_evaluate (csrc/evaluate.hip) bit for bit against the numpy restatement
(tests/evaluate_restate.py) and against utils.point_cloud_from_depth, then dataset.TestFrames + evaluate.run_test_phase end to end on the
committed example sequence with the reference-written checkpoint.  Run with ``pytest -m gpu`` on an MI355X."""

import gzip
import importlib
import os
import shutil

import numpy as np
import pytest
import torch

import evaluate_restate as er
from oracle import network as onet
from test_gpu_parity import noise_aware

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
evaluate = ea.evaluate

HERE = os.path.dirname(os.path.abspath(__file__))
SEQ_NAME = "_start_004259_end_004629_stride_25_segment_13"


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_batch(n, h, w, seed):
    """Masked inputs as the network sees them: an elliptical {0, 1} boundary with holes, colours in [-1, 1] (a quarter of them at
    c = 2 k / 255 - 1 and its float32 neighbours, where 255 (0.5 c + 0.5) lands within an ulp of an integer) times the boundary,
    positive depths with a few exact zeros and one frame of zeros when n >= 3, plausible intrinsics."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    b = (((yy - h / 2) / (0.45 * h)) ** 2 + ((xx - w / 2) / (0.48 * w)) ** 2 <= 1.0).astype(np.float32)
    b = np.broadcast_to(b, (n, 1, h, w)).copy()
    b[rng.random(b.shape) < 0.05] = 0.0
    c = rng.uniform(-1.0, 1.0, (n, 3, h, w)).astype(np.float32)
    near = rng.random(c.shape) < 0.25
    k = rng.integers(0, 256, size=c.shape)
    edge = (np.float32(2.0) * k.astype(np.float32) / np.float32(255.0) - np.float32(1.0)).astype(np.float32)
    step = rng.integers(-1, 2, size=c.shape)
    edge = np.where(step < 0, np.nextafter(edge, np.float32(-2)), np.where(step > 0, np.nextafter(edge, np.float32(2)), edge))
    c = np.where(near, np.clip(edge, -1.0, 1.0), c).astype(np.float32)
    c = (b * c).astype(np.float32)
    pred = np.abs(rng.standard_normal((n, 1, h, w)).astype(np.float32)) * np.float32(3.0)
    pred[rng.random(pred.shape) < 0.02] = 0.0
    if n >= 3:
        pred[1] = 0.0
    kk = np.zeros((n, 3, 3), np.float32)
    kk[:, 0, 0] = rng.uniform(0.8, 1.2, n) * w
    kk[:, 1, 1] = rng.uniform(0.8, 1.2, n) * w
    kk[:, 0, 2] = rng.uniform(0.4, 0.6, n) * w
    kk[:, 1, 2] = rng.uniform(0.4, 0.6, n) * h
    kk[:, 2, 2] = 1.0
    return c, b, pred, kk


def device_outputs(c, b, pred, kk, is_hsv, ds=1):
    t = [torch.from_numpy(a).to(dev()) for a in (c, b, pred, kk)]
    out = evaluate.outputs_from_predictions(*t, is_hsv=is_hsv, point_cloud_downsampling=ds)
    return out["depth"].cpu().numpy(), out["panels"].cpu().numpy(), out["points"].cpu().numpy(), out["offsets"]


# sizes 2 .. 4 (at n = 2): a row one pixel short of the write kernel's 256-pixel chunk, exactly one chunk, and one pixel into a second
SIZES = [(64, 96), (256, 320), (5, 255), (5, 256), (5, 257)]
CASES = ([(n, s, hsv) for hsv in (False, True) for s in (0, 1) for n in (1, 3, 8)] +
         [(2, s, hsv) for hsv in (False, True) for s in (2, 3, 4)])


@pytest.mark.parametrize("n, size, is_hsv", [(n, SIZES[s], hsv) for n, s, hsv in CASES], ids=["%d-size%d-%s" % c for c in CASES])
def test_outputs_match_restatement(n, size, is_hsv):
    h, w = size
    c, b, pred, kk = random_batch(n, h, w, seed=n * 100 + h + int(is_hsv))
    ds = 2 if (n == 3 and h == 64) else 1
    depth, panels, points, offsets = device_outputs(c, b, pred, kk, is_hsv, ds)
    want_depth, want_panels, want_clouds = er.batch_outputs(c, b, pred, kk, is_hsv, ds)
    assert np.array_equal(bits(depth), bits(want_depth))
    assert panels.shape == (n, h, 2 * w, 3)
    for f in range(n):
        bad = np.argwhere(np.any(panels[f] != want_panels[f], axis=-1))
        assert bad.size == 0, "frame %d: %d panel pixels differ, first at %s: %s vs %s" % (
            f, len(bad), bad[0], panels[f][tuple(bad[0])], want_panels[f][tuple(bad[0])])
    assert offsets[0] == 0 and len(offsets) == n + 1
    for f in range(n):
        got = points[offsets[f]:offsets[f + 1]]
        assert got.shape == want_clouds[f].shape, f
        assert np.array_equal(bits(got), bits(want_clouds[f])), f
    if n >= 3:
        assert np.all(panels[1, :, w:] == er.JET[0])          # the all-zero frame: entry 0, no NaN


def test_points_match_point_cloud_from_depth():
    """Each frame's slice equals utils.point_cloud_from_depth (endo_point_cloud) on that frame's depth, colour display and boundary."""
    n, h, w = 3, 256, 320
    c, b, pred, kk = random_batch(n, h, w, seed=9)
    depth, panels, points, offsets = device_outputs(c, b, pred, kk, False)
    for f in range(n):
        want = ea.utils.point_cloud_from_depth(depth[f, 0], panels[f, :, :w], b[f, 0], kk[f], 1)
        assert np.array_equal(bits(points[offsets[f]:offsets[f + 1]]), bits(want)), f


def test_bad_arguments():
    lib = ea._lib.load()
    assert lib.endo_evaluate_workspace_bytes(0, 64, 96) == -1 and lib.endo_evaluate_workspace_bytes(1, 64, 0) == -1
    assert lib.endo_evaluate_workspace_bytes(65536, 1, 1) == -1 and lib.endo_evaluate_workspace_bytes(2, 64, 96) > 0
    x = torch.zeros(1024, device=dev())          # every argument points into it: in bounds for N = 1, 2 x 2
    p = ea._lib.ptr(x)
    s = ea._lib.stream()
    need = int(lib.endo_evaluate_workspace_bytes(1, 2, 2))
    assert need <= x.numel() * 4
    args = [p, p, p, p, 1, 2, 2, 0, 1, p, p, p, p, p, need, s]
    assert lib.endo_evaluate(*args) == 0
    for i, bad in ((0, None), (4, 0), (7, 2), (8, 0), (14, need - 1)):
        a = list(args)
        a[i] = bad
        assert lib.endo_evaluate(*a) == -1, i
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """The committed example folder with the mask unpacked next to the other files (as tests/test_reader.py's fixture)."""
    src = os.path.join(HERE, "golden", "example_sequence", "bag_1", SEQ_NAME)
    dst = tmp_path_factory.mktemp("data_root") / "bag_1" / SEQ_NAME
    shutil.copytree(src, str(dst))
    with gzip.open(os.path.join(src, "undistorted_mask.bmp.gz"), "rb") as f, open(str(dst / "undistorted_mask.bmp"), "wb") as out:
        out.write(f.read())
    return str(dst)


@pytest.fixture(scope="module")
def trained(golden, tmp_path_factory):
    """The reference-written checkpoint saved to a file and read back with utils.load_checkpoint; (model in eval mode, fp32 state)."""
    from conftest import checkpoint_from_fixture
    blob = checkpoint_from_fixture(golden("checkpoint_2x64x96.npz"))
    path = tmp_path_factory.mktemp("ckpt") / "checkpoint_model_epoch_1_validation_0.5.pt"
    torch.save(blob, str(path))
    model = ea.FCDenseNet57(n_classes=1)
    state = ea.utils.load_checkpoint(path, model)
    assert state["epoch"] == blob["epoch"] and state["step"] == blob["step"]
    model = model.to(dev()).eval()
    return model, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def test_run_test_phase_on_the_example_sequence(sequence, trained, tmp_path):
    model, state = trained
    names = ea.utils.get_filenames_from_frame_indexes(os.path.dirname(sequence), ea.reader.read_visible_view_indexes(sequence))
    names = [str(p) for p in names]
    assert [os.path.basename(p) for p in names] == ["00004584.jpg", "00004594.jpg"]
    frames = ea.dataset.TestFrames(names, batch_size=2, suggested_h=256, suggested_w=320)
    assert len(frames) == 1
    (batch,) = list(frames)
    assert batch["names"] == ["00004584", "00004594"] and batch["colors"].shape == (2, 3, 256, 320)
    sh, eh, sw, ew = frames.sequences[sequence]["crop_positions"]
    for k, name in enumerate(names):
        want = ea.reader.get_test_color_img(name, sh, eh, sw, ew, 4.0).cpu().numpy()
        want -= np.float32(127.5)
        want *= np.reciprocal(np.float32(127.5))
        assert np.array_equal(batch["colors"][k].cpu().numpy(), want.transpose(2, 0, 1)), name
    b = batch["boundaries"].cpu().numpy()
    assert set(np.unique(b).tolist()) == {0.0, 1.0} and np.array_equal(b[0], b[1])
    with pytest.raises(RuntimeError, match="eval"):
        evaluate.test_outputs(model.train(), batch)
    model.eval()
    out = evaluate.test_outputs(model, batch)
    x = out["colors"].cpu()
    assert torch.equal(x, batch["boundaries"].cpu() * batch["colors"].cpu())
    state64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
    y32 = onet.forward(state, x, training=False)
    y64 = onet.forward(state64, x.double(), training=False)
    bt = torch.from_numpy(b)
    noise_aware(out["depth"], bt * y32, bt.double() * y64, "test-phase depth")
    depth = out["depth"].cpu().numpy()
    # the files: run_test_phase over the same frames, decoded / parsed back against the restatement of the GPU's own depth
    out_dir = tmp_path / "out"
    assert evaluate.run_test_phase(model, frames, out_dir) == 2
    Image = pytest.importorskip("PIL.Image")
    kk = batch["intrinsics"].cpu().numpy()
    c = x.numpy()
    for k, name in enumerate(batch["names"]):
        with Image.open(str(out_dir / (name + ".png"))) as im:
            png = np.asarray(im)
        want_panel = er.panel(c[k], b[k, 0], depth[k, 0])
        assert np.array_equal(png, want_panel[:, :, ::-1]), name
        assert np.array_equal(png, out["panels"][k].cpu().numpy()[:, :, ::-1]), name
        text = (out_dir / (name + ".ply")).read_text()
        head, body = text.split("end_header\n")
        want = er.point_cloud(depth[k, 0], want_panel[:, :320], b[k, 0], kk[k])
        assert "element vertex %d\n" % len(want) in head and len(want) > 1000
        back = np.array([[float(v) for v in line.split(" ")] for line in body.splitlines()], np.float64).reshape(-1, 6)
        assert np.array_equal(bits(back[:, :3].astype(np.float32)), bits(want[:, :3])) and np.array_equal(back[:, 3:], want[:, 3:]), name
    # batch size 1: the same frames one at a time
    single = ea.dataset.TestFrames(names, batch_size=1, suggested_h=256, suggested_w=320, prefetch=0, reader_threads=1)
    assert len(single) == 2
    depth1 = torch.cat([evaluate.test_outputs(model, part)["depth"] for part in single]).cpu()
    noise_aware(depth1, bt * y32, bt.double() * y64, "test-phase depth, batch size 1")
    print("batch sizes 1 and 2: depth bit-identical: %s (max abs difference %.3e)" % (
        torch.equal(depth1, out["depth"].cpu()), float((depth1 - out["depth"].cpu()).abs().max())))
    assert evaluate.run_test_phase(model, single, tmp_path / "one", ply_text=False) == 2
    for name in batch["names"]:
        assert (tmp_path / "one" / (name + ".png")).exists() and (tmp_path / "one" / (name + ".ply")).exists()
