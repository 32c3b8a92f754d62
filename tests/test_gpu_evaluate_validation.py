"""evaluate.py's validation phase on the device (reference evaluate.py:119-277): endo_depth_metrics and the AbsRelError / Threshold modules
against the reference's own outputs (tests/golden/depth_metrics_4x16x24.npz) and the numpy restatement, endo_evaluate_validation's panel bit
for bit against tests/evaluate_validation_restate.py, its point rows against endo_point_cloud, both entries under the workspace contract
(tests/guarded_alloc.py), and evaluate.run_validation_phase end to end on the committed example sequence with the reference-written
checkpoint.  Run with ``pytest -m gpu`` on an MI355X."""

import importlib
import os

import numpy as np
import pytest
import torch

import evaluate_validation_restate as evr
from guarded_alloc import guarded
from test_gpu_evaluate import SEQ_NAME, bits, sequence, trained  # noqa: F401 -- fixtures
from test_gpu_validation import display_inputs

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

PANEL_KEYS = ("colors_1", "colors_2", "boundaries", "depths_1", "depths_2", "sparse_depths_1", "sparse_depths_2", "masks_1", "masks_2",
              "warped_21", "warped_12", "sparse_flows_1", "sparse_flows_2", "flows_1", "flows_2", "intrinsics")


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def host(t):
    return t.detach().cpu().numpy()


def same_f32(a, b):
    """bit-identical float32 arrays, NaNs in the same places"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def validation_inputs(n, h, w, seed, constant=False):
    """test_gpu_validation.display_inputs' recipe (masked colours near truncation edges, depths with exact zeros, flows on both sides of
    atan2's branch cut), with what the validation panel adds:
      - sparse depths at about 5 % of the pixels and warped depths everywhere, a fifth of each below the dense range (negative: b * d has
        zeros in every frame) and a fifth above it, so both clamps act;
      - n >= 2: frame 0 holds the batch minimum of b * d (a negative depth inside the boundary) and frame n - 1 the maximum, in both halves;
      - constant=True (used at n = 1): the boundary is 1 everywhere and the depth one number, so min = max and the divisor is fl32(1e-5);
      - n = 1: the second half's dense flows are zero (max_v = 0: its sparse flows divide by zero)."""
    cols, depths, b, sparse, dense = display_inputs(n, h, w, seed)
    rng = np.random.default_rng(seed + 1000)
    if constant:
        b = np.ones_like(b)
        depths = [np.full_like(depths[0], 1.75), np.full_like(depths[1], 2.5)]
    inside = np.argwhere(b[0, 0] > 0.5)
    if n >= 2 and not constant:
        for half in range(2):
            y0, x0 = inside[3 + half]
            depths[half][0, 0, y0, x0] = -0.25
            y1, x1 = np.argwhere(b[n - 1, 0] > 0.5)[-5 - half]
            depths[half][n - 1, 0, y1, x1] = 40.0 + half
    if n == 1:
        dense[1][:] = 0.0
        sparse[1] = sparse[0].copy()          # (display_inputs zeroes them at n = 1)
    out = {"colors_1": cols[0], "colors_2": cols[1], "boundaries": b, "depths_1": depths[0], "depths_2": depths[1],
           "sparse_flows_1": sparse[0], "sparse_flows_2": sparse[1], "flows_1": dense[0], "flows_2": dense[1]}
    for half in range(2):
        lo, hi = evr.depth_range(depths[half], b)
        span = max(hi - lo, 1.0)

        def spread(shape):
            v = rng.uniform(lo, hi, shape) if hi > lo else np.full(shape, lo)
            side = rng.random(shape)
            v = np.where(side < 0.2, lo - rng.uniform(0.01, 1.0, shape) * span, np.where(side > 0.8, hi + rng.uniform(0.01, 1.0, shape) * span, v))
            return v.astype(np.float32)
        mask = (rng.random((n, 1, h, w)) < 0.05).astype(np.float32)
        out["masks_%d" % (half + 1)] = mask
        out["sparse_depths_%d" % (half + 1)] = (spread((n, 1, h, w)) * mask).astype(np.float32)
        warped = spread((n, 1, h, w))
        warped[rng.random(warped.shape) < 0.1] = 0.0          # pixels nothing was warped to
        out["warped_21" if half == 0 else "warped_12"] = warped
        assert (out["sparse_depths_%d" % (half + 1)] < lo).any() and (out["sparse_depths_%d" % (half + 1)] > hi).any()
        assert (warped < lo).any() and (warped > hi).any()
    kk = np.zeros((n, 3, 3), np.float32)
    kk[:, 0, 0] = rng.uniform(0.8, 1.2, n) * w
    kk[:, 1, 1] = rng.uniform(0.8, 1.2, n) * w
    kk[:, 0, 2] = rng.uniform(0.4, 0.6, n) * w
    kk[:, 1, 2] = rng.uniform(0.4, 0.6, n) * h
    kk[:, 2, 2] = 1.0
    out["intrinsics"] = kk
    return out


def device_outputs(x, ds=1, eps=1.0e-8):
    t = [torch.from_numpy(x[k]).to(dev()) for k in PANEL_KEYS]
    out = ea.display.validation_panels(*t, epsilon=eps, point_cloud_downsampling=ds)
    return {k: host(v) for k, v in out.items()}


def restated_panel(x):
    return evr.panel(x["colors_1"], x["colors_2"], x["boundaries"], x["depths_1"], x["depths_2"], x["sparse_depths_1"], x["sparse_depths_2"],
                     x["warped_21"], x["warped_12"], x["sparse_flows_1"], x["sparse_flows_2"], x["flows_1"], x["flows_2"])


# ---------------------------------------------------------------------------------------------
# the error measures
# ---------------------------------------------------------------------------------------------
def device_metrics(depths, sparse, masks, eps):
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in (depths, sparse, masks)]
    table = host(ea.losses.depth_metrics(*t, eps=eps))
    abs_rel = ea.losses.AbsRelError(eps=eps)(t)
    sigmas = ea.losses.Threshold(eps=eps)(t)
    n = depths.shape[0]
    assert isinstance(sigmas, list) and len(sigmas) == 3
    for v in [abs_rel] + sigmas:
        assert v.shape == (n,) and v.dtype == torch.float32 and not v.requires_grad and v.grad_fn is None
    assert same_f32(host(abs_rel), table[:, 0]) and all(same_f32(host(s), table[:, k + 1]) for k, s in enumerate(sigmas))
    return table


def test_metrics_match_the_reference(golden):
    """endo_depth_metrics and the two modules on the golden inputs: sigma 1, 2, 3 and the NaNs exactly as the reference's classes returned
    them, AbsRel within 1e-5 relative (the reference's pairwise float32 sum against one rounding of the exact sum)."""
    g = golden("depth_metrics_4x16x24.npz")
    table = device_metrics(g["depths"], g["sparse"], g["masks"], float(g["eps"]))
    print("\ndevice %s\nreference abs rel %s sigma %s %s %s" % (table.tolist(), g["abs_rel"], g["sigma_1"], g["sigma_2"], g["sigma_3"]))
    for k in range(3):
        assert same_f32(table[:, k + 1], g["sigma_%d" % (k + 1)]), k
    want = g["abs_rel"]
    assert np.array_equal(np.isnan(table[:, 0]), np.isnan(want)) and np.isnan(want).tolist() == [False, False, True, False]
    ok = ~np.isnan(want)
    assert np.all(np.abs(table[ok, 0] - want[ok]) <= 1e-5 * np.abs(want[ok]))
    assert same_f32(table, evr.metrics(g["depths"], g["sparse"], g["masks"], float(g["eps"])))


def test_metrics_match_the_restatement():
    """3 x 64 x 96: 24 strided passes of the block.  Sample 1's mask is emptied; the others hold about 300 points each (5 % of 6144: an
    empty draw has probability 1e-137).  sigma and the NaNs exactly; AbsRel within 2^-22 relative: the device's fp64 sum of non-negative
    float32 terms is within 6144 * 2^-53 of the exact sum, so after its one rounding it is at most one float32 step (2^-23 relative)
    from the restatement's, and the float32 quotients of two such neighbours differ by at most 2^-23 + 2 * 2^-24."""
    rng = np.random.default_rng(77)
    n, h, w = 3, 64, 96
    masks = (rng.random((n, 1, h, w)) < 0.05).astype(np.float32)
    masks[1] = 0.0
    sparse = (rng.uniform(0.5, 8.0, masks.shape).astype(np.float32) * masks).astype(np.float32)
    depths = np.where(rng.random(masks.shape) < 0.7, sparse * rng.uniform(0.7, 1.6, masks.shape), rng.uniform(0.5, 8.0, masks.shape)).astype(np.float32)
    depths[masks == 0] = rng.uniform(0.0, 8.0, int((masks == 0).sum())).astype(np.float32)
    assert masks[0].sum() > 100 and masks[2].sum() > 100
    table = device_metrics(depths, sparse, masks, 1.0e-8)
    want = evr.metrics(depths, sparse, masks, 1.0e-8)
    print("\ndevice %s\nrestated %s" % (table.tolist(), want.tolist()))
    assert np.all(np.isnan(table[1])) and np.all(np.isnan(want[1]))
    assert same_f32(table[:, 1:], want[:, 1:])
    for f in (0, 2):
        assert abs(float(table[f, 0]) - float(want[f, 0])) <= 2.0 ** -22 * abs(float(want[f, 0])), f
        assert 0.0 < table[f, 1] < table[f, 3] <= 1.0


def test_metrics_do_not_depend_on_alignment():
    """Planes that start one float behind a 16-byte boundary give the bits the aligned ones give (64 x 96), and 5 x 7 (35 pixels: fewer
    than a block's threads, sample 1 off every wider boundary) matches the restatement as test_metrics_match_the_restatement's sizes do."""
    rng = np.random.default_rng(78)
    for n, h, w in ((2, 64, 96), (2, 5, 7)):
        masks = (rng.random((n, 1, h, w)) < 0.3).astype(np.float32)
        sparse = (rng.uniform(0.5, 8.0, masks.shape).astype(np.float32) * masks).astype(np.float32)
        depths = (sparse * rng.uniform(0.7, 1.6, masks.shape) + (1 - masks) * 3.0).astype(np.float32)
        assert masks[0].sum() > 0 and masks[1].sum() > 0
        aligned = [torch.from_numpy(a).to(dev()) for a in (depths, sparse, masks)]
        shifted = []
        for a in aligned:
            flat = torch.zeros(a.numel() + 1, dtype=torch.float32, device=dev())
            flat[1:].copy_(a.reshape(-1))
            shifted.append(flat[1:].view(a.shape))
            assert shifted[-1].data_ptr() % 16 == 4 and shifted[-1].is_contiguous()
        got, moved = host(ea.losses.depth_metrics(*aligned)), host(ea.losses.depth_metrics(*shifted))
        assert same_f32(got, moved), (n, h, w)
        want = evr.metrics(depths, sparse, masks)
        assert same_f32(got[:, 1:], want[:, 1:])
        assert np.all(np.abs(got[:, 0] - want[:, 0]) <= 2.0 ** -22 * np.abs(want[:, 0])), (got, want)


# ---------------------------------------------------------------------------------------------
# the panel, the batch's measures and the point clouds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, h, w, constant", [(1, 64, 96, False), (1, 64, 96, True), (3, 64, 96, False), (9, 64, 96, False), (2, 20, 36, False)])
def test_panel_matches_restatement(n, h, w, constant):
    x = validation_inputs(n, h, w, seed=13 * n + h, constant=constant)
    out = device_outputs(x)
    got, want = out["panel"], restated_panel(x)
    assert got.shape == want.shape == ea.display.validation_panel_shape(n, h, w)
    bad = np.argwhere(np.any(got != want, axis=-1))
    assert len(bad) == 0, "%d pixels differ, first at %s: %s vs %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    gh, gw = ea.display.grid_shape(n, h, w)
    if constant:          # min = max: every depth section is JET entry 0
        for s in (1, 2, 3, 7, 8, 9):
            assert np.all(got[s * gh:(s + 1) * gh] == evr.JET[0][::-1])
    if n == 1:          # the second half's dense flows are zero: df2 black, sf2 at full value wherever a sparse flow is not zero
        assert np.all(got[11 * gh:] == 0) and got[10 * gh:11 * gh].max() == 255
    # the batch's measures: endo_depth_metrics' bits for both frames
    for half in range(2):
        t = [torch.from_numpy(x[k % (half + 1)]).to(dev()) for k in ("depths_%d", "sparse_depths_%d", "masks_%d")]
        assert same_f32(out["metrics"][:, half], host(ea.losses.depth_metrics(*t)))
    assert out["metrics"].shape == (n, 2, 4)


# (2, 9, 257): a second, one-pixel chunk of every row and a partial last band; (130, 64, 8): 130 * 8 = 1040 bands, more than the scan
# block's 1024 threads, so a thread owns two.  The first shape keeps the ids it had before the shape was a parameter.
CLOUD_SHAPES = [(3, 64, 96), (2, 9, 257), (130, 64, 8)]


@pytest.mark.parametrize("ds, shape", [pytest.param(ds, s, id=str(ds) if s == CLOUD_SHAPES[0] else "%d-%dx%dx%d" % ((ds,) + s))
                                       for s in CLOUD_SHAPES for ds in (1, 2)])
def test_points_match_point_cloud(ds, shape):
    """Point rows and offsets = utils.point_cloud_from_depth (endo_point_cloud) per frame on the unmasked scaled depth 1, the frame's own
    colour bytes, the boundary and the intrinsics."""
    n, h, w = shape
    x = validation_inputs(n, h, w, seed=5)
    out = device_outputs(x, ds)
    offsets = out["offsets"].tolist()
    assert offsets[0] == 0 and len(offsets) == n + 1 and out["points"].shape == (n * h * w, 6)
    for f in range(n):
        want = ea.utils.point_cloud_from_depth(x["depths_1"][f, 0], evr.cloud_colors(x["colors_1"][f]), x["boundaries"][f, 0],
                                               x["intrinsics"][f], ds)
        assert offsets[f + 1] - offsets[f] == len(want) > 0, f
        assert np.array_equal(bits(out["points"][offsets[f]:offsets[f + 1]]), bits(want)), f
    assert (x["depths_1"] * x["boundaries"] != x["depths_1"]).any()          # masked and unmasked depth differ: the rows hold the unmasked one


def test_workspace_contract():
    """Both entries on guarded buffers: NaN-poisoned workspace and outputs give the bits that zero-filled ones give, and no guard band is
    touched (guarded() checks them on exit).  `points` is compared up to offsets[N], its documented extent."""
    n, h, w = 3, 20, 36
    x = validation_inputs(n, h, w, seed=3)
    t = [torch.from_numpy(x[k]).to(dev()) for k in PANEL_KEYS]
    m = [torch.from_numpy(x[k]).to(dev()) for k in ("depths_1", "sparse_depths_1", "masks_1")]
    runs = {}
    for fill in ("poison", "zeros"):
        with guarded(device="cuda", fill=fill) as g:
            out = ea.display.validation_panels(*t, point_cloud_downsampling=1)
            table = ea.losses.depth_metrics(*m)
            torch.cuda.synchronize()
            assert len(g.blocks) == 6 and all(g.block_of(out[k]) is not None for k in ("panel", "metrics", "points", "offsets"))
            assert g.block_of(table) is not None
            runs[fill] = ({k: host(v) for k, v in out.items()}, host(table))
    (a, ta), (b, tb) = runs["poison"], runs["zeros"]
    total = int(a["offsets"][-1])
    assert np.array_equal(a["offsets"], b["offsets"]) and 0 < total < n * h * w
    assert np.array_equal(a["panel"], b["panel"]) and same_f32(a["metrics"], b["metrics"]) and same_f32(ta, tb)
    assert np.array_equal(bits(a["points"][:total]), bits(b["points"][:total])) and not np.isnan(a["points"][:total]).any()
    assert np.isnan(a["points"][total:]).all() and np.all(b["points"][total:] == 0)          # rows behind the extent are not written
    assert np.array_equal(a["panel"], restated_panel(x))


def test_error_cases():
    x = validation_inputs(1, 20, 36, seed=2)
    t = [torch.from_numpy(x[k]).to(dev()) for k in PANEL_KEYS]
    with pytest.raises(NotImplementedError, match="HSV"):
        ea.display.validation_panels(*t, is_hsv=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.display.validation_panels(*([t[0].cpu()] + t[1:]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.display.validation_panels(*(t[:5] + [t[5].cpu()] + t[6:]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.losses.AbsRelError()([t[3].cpu(), t[5], t[7]])
    with pytest.raises(ValueError):
        ea.display.validation_panels(*(t[:3] + [t[3][:, :, :10]] + t[4:]))
    lib = ea._lib.load()
    p, s = ea._lib.ptr, ea._lib.stream()
    need = int(lib.endo_evaluate_validation_workspace_bytes(1, 20, 36))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    panel = torch.zeros(ea.display.validation_panel_shape(1, 20, 36), dtype=torch.uint8, device=dev())
    metrics = torch.zeros((1, 2, 4), device=dev())
    points = torch.zeros((20 * 36, 6), device=dev())
    offsets = torch.zeros(2, dtype=torch.int64, device=dev())
    args = [p(a) for a in t] + [1, 20, 36, 1e-8, 0, 1, p(panel), p(metrics), p(points), p(offsets), p(ws), need, s]
    assert lib.endo_evaluate_validation(*args) == 0
    for i, bad in ((0, None), (15, None), (16, 0), (20, 1), (21, 0), (22, None), (27, need - 1)):          # 20: is_hsv = 1
        a = list(args)
        a[i] = bad
        assert lib.endo_evaluate_validation(*a) == -1, i
    assert lib.endo_depth_metrics(p(t[3]), p(t[5]), p(t[7]), 0, 20, 36, 1e-8, p(metrics), s) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
class _Writer(object):
    def __init__(self):
        self.calls = []

    def add_image(self, tag, img, step):
        self.calls.append((tag, np.array(img), step))


def test_run_validation_phase_on_the_example_sequence(sequence, trained, tmp_path, monkeypatch):  # noqa: F811 -- fixtures
    """dataset.TrainingBatches(transform=None, shuffle=False) over the committed example sequence, 2 batches of 2 pairs, through
    run_validation_phase with the reference-written checkpoint: the files' names, each PNG = utils.write_png of the restated panel of
    that batch's own intermediate tensors, the PLY's rows = offsets[1], the returned measures = the modules' on the same tensors."""
    model, _ = trained
    model.eval()
    first = os.path.join(sequence, sorted(f for f in os.listdir(sequence) if f.endswith(".jpg"))[0])
    batches = ea.dataset.TrainingBatches([sequence], adjacent_range=(10, 10), batch_size=2, image_file_names=[first], num_iter=4,
                                         shuffle=False, suggested_h=256, suggested_w=320, transform=None)
    # the folder holds the two frames of one pair (views 0 and 10): both directions of it, in a fixed order
    batches._draw = lambda idx: (sequence, 0, 10) if idx % 2 == 0 else (sequence, 10, -10)
    assert len(batches) == 2
    seen = []
    real = ea.evaluate.validation_outputs

    def recording(model, batch, **kw):
        out = real(model, batch, **kw)
        seen.append((batch, out))
        return out
    monkeypatch.setattr(ea.evaluate, "validation_outputs", recording)
    writer = _Writer()
    out_dir = tmp_path / "validation"
    res = ea.evaluate.run_validation_phase(model, batches, out_dir, writer=writer, step=7)
    monkeypatch.undo()
    assert sorted(os.listdir(str(out_dir))) == ["0.ply", "0.png", "1.ply", "1.png"]
    assert res["pairs"] == 4 and res["metrics"].shape == (4, 2, 4) and res["metrics"].dtype == np.float32 and len(seen) == 2
    assert res["non_finite"] == 0 and res["mean_metrics"].shape == (2, 4)
    assert np.array_equal(res["mean_metrics"], res["metrics"].astype(np.float64).mean(axis=0))
    print("\nexample sequence: mean [abs rel, sigma 1, 2, 3] frame 1 %s, frame 2 %s" % tuple(res["mean_metrics"].tolist()))
    assert [c[0] for c in writer.calls] == ["validation/Images/Results (c1, sd1, d1, wd1, sf1, df1, c2, sd2, d2, wd2, sf2, df2)"] * 2
    for index, (batch, out) in enumerate(seen):
        x = {"colors_1": out["colors_1"], "colors_2": out["colors_2"], "boundaries": batch["boundaries"],
             "depths_1": out["scaled_depths_1"], "depths_2": out["scaled_depths_2"], "sparse_depths_1": batch["sparse_depths_1"],
             "sparse_depths_2": batch["sparse_depths_2"], "warped_21": out["warped_depths_2_to_1"], "warped_12": out["warped_depths_1_to_2"],
             "sparse_flows_1": out["sparse_flows_1"], "sparse_flows_2": out["sparse_flows_2"], "flows_1": out["flows_1"], "flows_2": out["flows_2"]}
        x = {k: host(v) for k, v in x.items()}
        assert np.array_equal(x["colors_1"], host(batch["boundaries"]) * host(batch["colors_1"]))
        want_panel = restated_panel(x)
        assert want_panel.shape == ea.display.validation_panel_shape(2, 256, 320)
        assert np.array_equal(host(out["panel"]), want_panel), index
        ea.utils.write_png(tmp_path / "want.png", want_panel[:, :, ::-1])
        assert (out_dir / ("%d.png" % index)).read_bytes() == (tmp_path / "want.png").read_bytes(), index
        tag, img, step = writer.calls[index]
        assert step == 7 and np.array_equal(img, want_panel.transpose(2, 0, 1))
        head = (out_dir / ("%d.ply" % index)).read_text().split("end_header\n")[0]
        offsets = out["offsets"]
        assert len(offsets) == 3 and offsets[0] == 0 and offsets[1] > 1000
        assert "element vertex %d\n" % offsets[1] in head, index
        for half in range(2):
            t = [out["scaled_depths_%d" % (half + 1)], batch["sparse_depths_%d" % (half + 1)], batch["sparse_depth_masks_%d" % (half + 1)]]
            want = torch.stack([ea.losses.AbsRelError(1.0e-8)(t)] + ea.losses.Threshold(1.0e-8)(t), dim=1)
            assert same_f32(res["metrics"][2 * index:2 * index + 2, half], host(want)), (index, half)
            assert same_f32(host(out["metrics"])[:, half], host(want))
    # every sample's cloud, binary PLY, no panel
    res_all = ea.evaluate.run_validation_phase(model, batches, tmp_path / "all", write_png=False, ply_text=False, all_samples=True)
    assert sorted(os.listdir(str(tmp_path / "all"))) == ["0.ply", "0_1.ply", "1.ply", "1_1.ply"] and res_all["pairs"] == 4
    with pytest.raises(RuntimeError, match="eval"):
        ea.evaluate.validation_outputs(model.train(), seen[0][0])
    model.eval()
    with pytest.raises(NotImplementedError, match="HSV"):
        ea.evaluate.validation_outputs(model, seen[0][0], is_hsv=True)
