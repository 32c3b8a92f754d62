"""The validation pass and the display panels on the device (reference train.py:353-371, 375-492): endo_display (csrc/display.hip) bit for bit
against the numpy restatement (tests/display_restate.py), TrainingStep.validation_losses against the reference-generated losses of
train_step_2x64x96.npz and against a training step, endo_validation_accumulate against train.py's Python recurrence, display_panels() against
the loss head's planes and the modules, and train_step.validate end to end on the committed example sequence with the reference-written
checkpoint.  Run with ``pytest -m gpu`` on an MI355X."""

import ctypes
import importlib
import math
import os

import numpy as np
import pytest
import torch

import display_restate as dr
from oracle import network as onet
from test_gpu_evaluate import SEQ_NAME, sequence, trained  # noqa: F401 -- fixtures
from test_gpu_parity import assert_close, noise_aware, to_dev

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
synthetic = ea.synthetic


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def host(t):
    return t.detach().cpu().numpy()


def display_inputs(n, h, w, seed):
    """Inputs as the loss head leaves them: an elliptical {0, 1} boundary with holes; masked colours in [-1, 1], a quarter of them within an
    ulp of a truncation edge (255 (0.5 c + 0.5) = k); positive depths with exact zeros, frame 2 constant (n >= 3); sparse flows mostly zero
    (a sparse set of points), dense flows everywhere, both masked by the boundary so that negative components become -0; frame 1's sparse
    flows all zero (n >= 3); with n = 1 the second half's sparse flows are all zero (max_v = 0)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    b = (((yy - h / 2) / (0.45 * h)) ** 2 + ((xx - w / 2) / (0.48 * w)) ** 2 <= 1.0).astype(np.float32)
    b = np.broadcast_to(b, (n, 1, h, w)).copy()
    b[rng.random(b.shape) < 0.05] = 0.0
    cols = []
    for _ in range(2):
        c = rng.uniform(-1.0, 1.0, (n, 3, h, w)).astype(np.float32)
        k = rng.integers(0, 256, size=c.shape).astype(np.float32)
        edge = (k / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
        step = rng.integers(-1, 2, size=c.shape)
        edge = np.where(step < 0, np.nextafter(edge, np.float32(-2)), np.where(step > 0, np.nextafter(edge, np.float32(2)), edge))
        c = np.where(rng.random(c.shape) < 0.25, np.clip(edge, -1.0, 1.0), c).astype(np.float32)
        cols.append((b * c).astype(np.float32))
    depths = []
    for _ in range(2):
        d = (np.abs(rng.standard_normal((n, 1, h, w))) * 3.0 + 0.5).astype(np.float32)
        d[rng.random(d.shape) < 0.02] = 0.0
        if n >= 3:
            d[2] = 1.75
        depths.append(d)
    sparse, dense = [], []
    for half in range(2):
        s = (rng.standard_normal((n, 2, h, w)) * 4.0).astype(np.float32)
        s[np.broadcast_to(rng.random((n, 1, h, w)) < 0.9, s.shape)] = 0.0
        s[:, :, 3, :] = np.float32(-0.0)
        s[:, 1, 5, ::2] = np.float32(-0.0)
        s[:, 1, 5, 1::2] = -2.0          # (-2 Hg / Wg, -0 / +0): the two sides of atan2's branch cut
        s[:, 0, 5, :] = -1.0
        if n >= 3:
            s[1] = 0.0
        if n == 1 and half == 1:
            s[:] = 0.0
        sparse.append((b * s).astype(np.float32))
        f = (rng.standard_normal((n, 2, h, w)) * 6.0).astype(np.float32)
        dense.append((b * f).astype(np.float32))
    return cols, depths, b, sparse, dense


def device_panel(cols, depths, b, sparse, dense):
    t = lambda a: torch.from_numpy(a).to(dev())
    out = ea.display.panels(t(cols[0]), t(cols[1]), t(depths[0]), t(depths[1]), t(b), t(sparse[0]), t(sparse[1]), t(dense[0]), t(dense[1]))
    return host(out)


@pytest.mark.parametrize("n, h, w", [(1, 64, 96), (3, 64, 96), (8, 64, 96), (9, 64, 96), (8, 256, 320)])
def test_display_matches_restatement(n, h, w):
    cols, depths, b, sparse, dense = display_inputs(n, h, w, seed=11 * n + h)
    got = device_panel(cols, depths, b, sparse, dense)
    want = dr.panel(cols[0], cols[1], depths[0], depths[1], b, sparse[0], sparse[1], dense[0], dense[1])
    assert got.shape == want.shape == ea.display.panel_shape(n, h, w)
    bad = np.argwhere(np.any(got != want, axis=-1))
    assert len(bad) == 0, "%d pixels differ, first at %s: %s vs %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    gh, gw = dr.grid_shape(n, h, w)
    if n == 1:          # the second half's sparse flows are zero: max_v = 0, sf2 black
        assert np.all(got[6 * gh:7 * gh] == 0)
    # the literal float32 formula of draw_flow (libm's atan2f) moves a hue by one step at most; V is the same
    for half in range(2):
        hsv, top = dr.flow_hsv(sparse[half])
        lit, lit_top = dr.flow_hsv(sparse[half], literal=True)
        assert top == lit_top and np.array_equal(hsv[..., 2], lit[..., 2])
        for flows, max_v in ((sparse[half], None), (dense[half], top)):
            a, _ = dr.flow_hsv(flows, max_v)
            c, _ = dr.flow_hsv(flows, max_v, literal=True)
            assert np.abs(a[..., 0].astype(int) - c[..., 0].astype(int)).max() <= 1


def test_display_argument_errors():
    lib = ea._lib.load()
    assert lib.endo_display_workspace_bytes(0, 8, 8) == -1 and lib.endo_display_workspace_bytes(2, 8, -1) == -1
    rows, cols = ctypes.c_int(), ctypes.c_int()
    assert lib.endo_display_panel_shape(9, 64, 96, ctypes.byref(rows), ctypes.byref(cols)) == 0
    assert (rows.value, cols.value) == (8 * (2 * 66 + 2), 8 * 98 + 2)
    x = torch.zeros(64, device=dev())
    p = ea._lib.ptr(x)
    need = int(lib.endo_display_workspace_bytes(1, 2, 2))
    assert lib.endo_display(*([p] * 9), 1, 2, 2, p, p, need - 1, ea._lib.stream()) == -1
    assert lib.endo_display(*([p] * 8), None, 1, 2, 2, p, p, need, ea._lib.stream()) == -1
    offsets = (ctypes.c_int64 * 6)()
    assert lib.endo_loss_head_planes(0, 2, 2, offsets) == -1
    assert lib.endo_validation_accumulate(p, -1, p, None, ea._lib.stream()) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# validation_losses
# ---------------------------------------------------------------------------------------------
def golden_setup(g, **kw):
    n, h, w, seed = (int(g[k]) for k in ("n", "h", "w", "seed"))
    state = onet.keep_depth_positive(onet.perturb_affine(onet.synthetic_state(seed), seed + 1))
    model = ea.FCDenseNet57(1)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    opt = ea.optim.FusedClipSGD(model, lr=float(g["max_lr"]))
    sched = ea.scheduler.CyclicLR(opt, base_lr=float(g["base_lr"]), max_lr=float(g["max_lr"]), step_size=int(g["step_size"]))
    step = ea.train_step.TrainingStep(model, opt, h, w, **kw)
    batches = [synthetic.make_batch(n, h, w, seed=seed + 10 + it, sparse_points=min(500, h * w // 6)) for it in range(2)]
    return state, model, opt, sched, step, batches


def snapshot(model, opt):
    grads = model.flat_gradient_bucket().clone()
    mom = opt._momentum.clone() if opt._momentum is not None else None
    return model.flat_parameters().clone(), grads, mom, [p.grad.clone() if p.grad is not None else None for p in model.parameters()]


def assert_same_snapshot(a, b):
    assert torch.equal(a[0], b[0]), "parameters changed"
    assert torch.equal(a[1], b[1]), "gradient bucket changed"
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2]), "momentum changed"
    for x, y in zip(a[3], b[3]):
        assert (x is None and y is None) or torch.equal(x, y), ".grad changed"


def test_validation_losses_golden(golden):
    """validation_losses = the train-mode forward losses train_step_2x64x96.npz recorded from the reference (step0_* on the initial state,
    step1_* after one training step), within the bounds of test_train_step_golden; nothing but the BatchNorm running statistics changes."""
    g = golden("train_step_2x64x96.npz")
    state, model, opt, sched, step, batches = golden_setup(g)
    n = int(g["n"])
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    before = snapshot(model, opt)
    v0 = host(step.validation_losses(to_dev(batches[0])))
    assert v0.shape == (4,) and v0[3] == 0.0
    for i, key in enumerate(("loss", "dcl", "sfl")):
        want = float(g["step0_" + key])
        assert abs(float(v0[i]) - want) <= 1e-4 * abs(want), (key, float(v0[i]), want)
    assert_same_snapshot(before, snapshot(model, opt))
    # the running statistics: the oracle's two train-mode forwards (frame 1, then frame 2), fp32 and fp64
    st32 = {k: v.clone() for k, v in state.items()}
    st64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    b = batches[0]["boundaries"]
    for x in (b * batches[0]["colors_1"], b * batches[0]["colors_2"]):
        onet.forward(st32, x, training=True)
        onet.forward(st64, x.double(), training=True)
    sd = model.state_dict()
    for name in ("denseBlocksDown.0.layers.0.norm", "transDownBlocks.2.norm", "bottleneck.bottleneck.layers.3.norm", "denseBlocksUp.4.layers.3.norm"):
        for stat in (".running_mean", ".running_var"):
            noise_aware(sd[name + stat], st32[name + stat], st64[name + stat], name + stat)
        assert int(sd[name + ".num_batches_tracked"]) == int(sd0[name + ".num_batches_tracked"]) + 2
    # one training step on batch 0, then validation of batch 1 = step1_* of the reference
    sched.batch_step(batch_iteration=0)
    out = step(to_dev(batches[0]))
    assert not out["skipped"]
    sched.batch_step(batch_iteration=1)
    before = snapshot(model, opt)
    assert before[2] is not None
    v1 = host(step.validation_losses(to_dev(batches[1])))
    for i, key in enumerate(("loss", "dcl", "sfl")):
        want = float(g["step1_" + key])
        assert abs(float(v1[i]) - want) <= 1e-3 * abs(want), (key, float(v1[i]), want)
    torch.cuda.synchronize()
    assert_same_snapshot(before, snapshot(model, opt))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_validation_losses_equal_training_losses(golden, mode):
    """validation_losses on a batch = the StepOutput losses of a training step on the same batch and state: the same kernels.  The bound is
    the spread of two identical training steps (0 when they are bit-identical)."""
    g = golden("train_step_2x64x96.npz")
    kw = {"bf16_storage": True} if mode == "bf16" else {}
    runs = [golden_setup(g, **kw) for _ in range(3)]
    batch = to_dev(runs[0][5][0])
    outs = [runs[i][4](batch) for i in range(2)]
    train = [np.array([o["loss"], float(o["dcl"]), float(o["sfl"])], np.float32) for o in outs]
    val = host(runs[2][4].validation_losses(batch))[:3]
    spread = np.abs(train[0] - train[1])
    print("\n%s: training %s / %s, validation %s, spread of two training steps %s" % (mode, train[0], train[1], val, spread))
    assert np.all(np.abs(val - train[0]) <= spread), (val, train[0], spread)


def test_validation_losses_module_path(golden):
    """fused_head=False: losses() under no_grad, the same four numbers within the fused-head bound of test_fused_loss_head_matches_modules;
    no autograd graph is left behind."""
    g = golden("train_step_2x64x96.npz")
    _, _, _, _, fused, batches = golden_setup(g)
    _, model, opt, _, modular, _ = golden_setup(g, fused_head=False)
    batch = to_dev(batches[0])
    a = fused.validation_losses(batch)
    bt = modular.validation_losses(batch)
    assert not bt.requires_grad and bt.shape == (4,)
    assert_close(bt[:3], a[:3], 1e-5, "module-path validation losses")
    assert float(bt[3]) == 0.0
    with pytest.raises(RuntimeError, match="fused"):
        modular.display_panels()


# ---------------------------------------------------------------------------------------------
# running means
# ---------------------------------------------------------------------------------------------
def recurrence(losses, initial=(math.nan,) * 3):
    """train.py:446-456 in Python floats: returns the means after each batch."""
    m = list(initial)
    out = []
    for batch, (loss, dcl, sfl) in enumerate(losses):
        loss, dcl, sfl = float(np.float32(loss)), float(np.float32(dcl)), float(np.float32(sfl))
        if not np.isnan(loss):
            if batch == 0:
                m = [loss, dcl, sfl]
            else:
                m = [(m[0] * batch + loss) / (batch + 1.0), (m[1] * batch + dcl) / (batch + 1.0), (m[2] * batch + sfl) / (batch + 1.0)]
        out.append(list(m))
    return np.array(out, np.float64).reshape(-1, 3)


def same_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def device_recurrence(losses, initial=(math.nan,) * 3, with_history=True):
    lib = ea._lib.load()
    count = len(losses)
    t = torch.from_numpy(np.concatenate([np.asarray(losses, np.float32), np.zeros((count, 1), np.float32)], axis=1)).to(dev())
    means = torch.tensor(initial, dtype=torch.float64, device=dev())
    hist = torch.full((count, 3), -1.0, dtype=torch.float64, device=dev())
    for i in range(count):
        ea._lib.check(lib.endo_validation_accumulate(ea._lib.ptr(t[i]), i, ea._lib.ptr(means), ea._lib.ptr(hist) if with_history else None,
                                                     ea._lib.stream()), "endo_validation_accumulate")
    return host(means), host(hist)


def test_validation_accumulate_matches_recurrence():
    rng = np.random.default_rng(5)
    nan, inf = math.nan, math.inf
    cases = {
        "nan at batch 0": ([(nan, 1.0, nan), (2.5, 0.5, 2.0), (3.0, 0.25, 2.75)], (nan,) * 3),
        "nan at batch 0, initial": ([(nan, 1.0, nan), (2.5, 0.5, 2.0), (3.0, 0.25, 2.75)], (1.5, 0.125, 1.375)),
        "nan mid-pass": ([(1.25, 0.25, 1.0), (nan, nan, 0.5), (2.0, 0.5, 1.5), (1.0, 0.1, 0.9)], (nan,) * 3),
        "inf": ([(1.25, 0.25, 1.0), (inf, 0.5, inf), (2.0, 0.5, 1.5)], (nan,) * 3),
        "-inf dcl": ([(1.25, 0.25, 1.0), (-inf, -inf, 0.5)], (0.0, 0.0, 0.0)),
        "1000 batches": ([tuple(v) for v in (rng.lognormal(0.0, 1.0, (1000, 3)) * [1.0, 0.05, 1.0]).astype(np.float32)], (nan,) * 3),
    }
    for name, (losses, initial) in cases.items():
        want = recurrence(losses, initial)
        means, hist = device_recurrence(losses, initial)
        assert same_f64(hist, want), name
        assert same_f64(means, want[-1]), name
    means, hist = device_recurrence(cases["nan mid-pass"][0], with_history=False)
    assert same_f64(means, recurrence(cases["nan mid-pass"][0])[-1]) and np.all(hist == -1.0)


def test_validate_over_batches():
    """validate over 5 synthetic batches: means bit-identical to the Python recurrence applied to the per-batch losses it returns, each batch's
    losses = validation_losses of the same batch on a twin (the bound of a training step's spread), panels every second batch = the
    restatement of the head planes at that moment, parameters untouched."""
    n, h, w = 2, 64, 96
    state = onet.keep_depth_positive(onet.perturb_affine(onet.synthetic_state(21), 22))
    steps = []
    for _ in range(2):
        model = ea.FCDenseNet57(1)
        model.load_state_dict(state)
        model = model.to(dev()).train()
        steps.append(ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1e-3), h, w))
    batches = [to_dev(synthetic.make_batch(n, h, w, seed=40 + i, sparse_points=500)) for i in range(5)]
    params = steps[0].model.flat_parameters().clone()
    shown = []

    def on_display(index, panel):
        x, b = steps[0]._display_source
        s1, s2, f1, f2, sf1, sf2 = [host(t) for t in head_planes(steps[0], n, h, w)]
        want = dr.panel(host(x[:n]), host(x[n:]), s1, s2, host(b), sf1, sf2, f1, f2)
        shown.append((index, panel, want))
    res = ea.train_step.validate(steps[0], batches, display_each=2, on_display=on_display)
    assert res.losses.shape == (5, 3) and res.losses.dtype == np.float32 and res.running_means.shape == (5, 3)
    want = recurrence(res.losses)
    assert same_f64(res.running_means, want)
    assert same_f64([res.mean_loss, res.mean_depth_consistency_loss, res.mean_sparse_flow_loss], want[-1])
    assert all(isinstance(v, float) for v in res[:3]) and all(np.isfinite(res[:3]))
    twin = np.stack([host(steps[1].validation_losses(batch))[:3] for batch in batches])
    print("\nvalidate: per-batch losses bit-identical to a twin's validation_losses: %s" % np.array_equal(twin, res.losses))
    assert_close(torch.from_numpy(twin), torch.from_numpy(res.losses), 1e-5, "per-batch losses vs a twin")
    assert [i for i, _, _ in shown] == [0, 2, 4]
    for i, panel, want_panel in shown:
        assert panel.dtype == torch.uint8 and tuple(panel.shape) == ea.display.panel_shape(n, h, w)
        assert np.array_equal(host(panel), want_panel), i
    assert torch.equal(steps[0].model.flat_parameters(), params)
    # a generator (no len()) grows the history on the device
    res_gen = ea.train_step.validate(steps[0], (b for b in batches), initial=(1.0, 2.0, 3.0))
    assert same_f64(res_gen.running_means, recurrence(res_gen.losses, (1.0, 2.0, 3.0)))


# ---------------------------------------------------------------------------------------------
# display_panels
# ---------------------------------------------------------------------------------------------
def head_planes(step, n, h, w):
    offsets = (ctypes.c_int64 * 6)()
    assert ea._lib.load().endo_loss_head_planes(n, h, w, offsets) == 0
    p = n * h * w
    ws = step._head_ws
    return [ws[offsets[i]:offsets[i] + c * p].view(n, c, h, w).clone() for i, c in zip(range(6), (1, 1, 2, 2, 2, 2))]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_display_panels_after_a_training_step(mode):
    """display_panels() after a training step = the restatement of the head workspace's planes and the masked input; the planes = the
    modules' own tensors on the same predictions (scaled depths, masked flows from depth, masked sparse flows)."""
    n, h, w = 3, 64, 96
    state = onet.keep_depth_positive(onet.perturb_affine(onet.synthetic_state(23), 24))
    model = ea.FCDenseNet57(1)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    kw = {"bf16_storage": True} if mode == "bf16" else {}
    step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1e-3), h, w, **kw)
    with pytest.raises(RuntimeError, match="no training or validation call"):
        step.display_panels()
    batch = to_dev(synthetic.make_batch(n, h, w, seed=50, sparse_points=400))
    step(batch)
    panel = host(step.display_panels())
    s1, s2, f1, f2, sf1, sf2 = [host(t) for t in head_planes(step, n, h, w)]
    b = host(batch["boundaries"])
    c1, c2 = b * host(batch["colors_1"]), b * host(batch["colors_2"])
    assert np.array_equal(panel, dr.panel(c1, c2, s1, s2, b, sf1, sf2, f1, f2))
    # the planes against the modules on the same predictions (what test_fused_loss_head_matches_modules does for the losses)
    losses_t, x, _, pred, _ = step._fused_iteration(batch)
    assert np.array_equal(host(x), np.concatenate([c1, c2]))
    planes = head_planes(step, n, h, w)
    mm = ea.train_step.mask_mul
    scaled_1, _ = step.depth_scaling_layer([pred[:n], batch["sparse_depths_1"], batch["sparse_depth_masks_1"]])
    scaled_2, _ = step.depth_scaling_layer([pred[n:], batch["sparse_depths_2"], batch["sparse_depth_masks_2"]])
    bt = batch["boundaries"]
    flow_1 = mm(step.flow_from_depth_layer([scaled_1, bt, batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"], batch["intrinsics"]]), bt)
    flow_2 = mm(step.flow_from_depth_layer([scaled_2, bt, batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"], batch["intrinsics"]]), bt)
    modules = [scaled_1, scaled_2, flow_1, flow_2, mm(batch["sparse_flows_1"], bt), mm(batch["sparse_flows_2"], bt)]
    same = [torch.equal(a, m.detach()) for a, m in zip(planes, modules)]
    print("\n%s: head planes bit-identical to the modules': %s" % (mode, same))
    for a, m, name in zip(planes, modules, ("scaled_1", "scaled_2", "flow_1", "flow_2", "sparse_flow_1", "sparse_flow_2")):
        assert_close(a, m.detach(), 1e-6, name)
    assert all(same[4:])          # the masked sparse flows are one multiplication each way


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def test_validate_on_the_example_sequence(sequence, trained, tmp_path):  # noqa: F811 -- fixtures
    """dataset.TrainingBatches(transform=None, shuffle=False) over the committed example sequence -> validate(display_each=1) with the
    reference-written checkpoint in train mode: finite means, parameters unchanged, every panel = the restatement of its head planes, and
    the PNG written with utils.write_png decodes (Pillow) to the device panel."""
    model, _ = trained
    model.train()
    first = os.path.join(sequence, sorted(f for f in os.listdir(sequence) if f.endswith(".jpg"))[0])
    batches = ea.dataset.TrainingBatches([sequence], adjacent_range=(10, 10), batch_size=2, image_file_names=[first], num_iter=4,
                                         shuffle=False, suggested_h=256, suggested_w=320, transform=None)
    # the folder holds the two frames of one pair (views 0 and 10): both directions of it, in a fixed order
    batches._draw = lambda idx: (sequence, 0, 10) if idx % 2 == 0 else (sequence, 10, -10)
    assert len(batches) == 2
    step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1e-4), 256, 320)
    params = model.flat_parameters().clone()
    shown = []

    def on_display(index, panel):
        planes = [host(t) for t in head_planes(step, 2, 256, 320)]
        x, b = step._display_source
        shown.append((index, host(panel), host(x), host(b), planes))
    res = ea.train_step.validate(step, batches, display_each=1, on_display=on_display)
    print("\nexample sequence: means %.6f %.6f %.6f, per batch %s" % (res.mean_loss, res.mean_depth_consistency_loss, res.mean_sparse_flow_loss,
                                                                     res.losses.tolist()))
    assert np.all(np.isfinite(res[:3])) and res.losses.shape == (2, 3)
    assert torch.equal(model.flat_parameters(), params)
    name = "checkpoint_model_epoch_{}_validation_{}.pt".format(3, res.mean_sparse_flow_loss)
    assert name.startswith("checkpoint_model_epoch_3_validation_") and "nan" not in name
    assert [i for i, *_ in shown] == [0, 1]
    Image = pytest.importorskip("PIL.Image")
    for index, panel, x, b, (s1, s2, f1, f2, sf1, sf2) in shown:
        assert panel.shape == ea.display.panel_shape(2, 256, 320)
        assert np.array_equal(panel, dr.panel(x[:2], x[2:], s1, s2, b, sf1, sf2, f1, f2)), index
        path = tmp_path / ("validation_%d.png" % index)
        ea.utils.write_png(path, panel[:, :, ::-1])
        with Image.open(str(path)) as im:
            assert np.array_equal(np.asarray(im), panel), index
