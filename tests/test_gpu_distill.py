"""GPU checks of teacher-student distillation: endo_distill_head (csrc/distill.hip), train_step.DistillationStep and
utils.learn_from_teacher.

  * the head against what the reference's own functions gave (tests/golden/distill.npz, written by tests/golden/make_distill_golden.py)
    and against the fp32 restatement (tests/distill_restate.py) at the smallest shapes on both sides of the kernels' constants: less
    than one block; odd hw with unaligned sample starts (the scalar form); hw = 2047 / 2048 / 2049 / 2052 around the reduce block of
    2048 elements and the vector width of 4; a full block plus a tail; pointers one float off 16 bytes; and the two sizes past the apply
    pass's cap of 1024 blocks (x 256 threads, x 4 elements in the vector form), where its threads loop.  Bounds: the project's for the
    loss kernels (tests/test_gpu_parity.py::test_losses), value 2e-5 and gradient 1e-4 of max |ref|;
  * the head against the existing endo_scale_inv_* kernels on the device (non-negative inputs), and ``accumulate = 1`` against an
    endo_loss_head plus the ``accumulate = 0`` call: the fused-against-modules bounds, 1e-6 value and 2e-6 gradient;
  * the workspace contract of the entry (tests/guarded_alloc.py);
  * DistillationStep against the fixture's ``step`` and ``combined`` records with tests/test_gpu_parity.py::test_train_step_golden's
    bounds, against utils.learn_from_teacher + the fused optimizer on a twin student, its guard, and train_step.validate.
Run with ``pytest -m gpu`` on an MI355X."""

import importlib

import numpy as np
import pytest
import torch

import distill_restate as dr
from guarded_alloc import guarded
from oracle import network as onet

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
synthetic = ea.synthetic
_lib = ea._lib

FIXTURE = "distill.npz"
HEAD_SEED, EDGE_SEED = 20241101, 20241102          # make_distill_golden.py's
KEYS = ("pred_1", "pred_2", "goal_1", "goal_2", "boundaries")
VALUE_TOL, GRAD_TOL = 2e-5, 1e-4
FUSED_VALUE_TOL, FUSED_GRAD_TOL = 1e-6, 2e-6
# (n, H, W) -> hw: 96 (less than one block); 117 (odd: scalar form, unaligned sample starts, odd sample count); 2240 (a full reduce
# block and a tail); 6144; 2047 / 2048 / 2049 / 2052 (one element either side of the reduce block; one float4 past it)
SHAPES = [(1, 8, 12), (3, 9, 13), (2, 40, 56), (2, 64, 96), (1, 23, 89), (2, 32, 64), (1, 3, 683), (2, 27, 76)]
# past the apply pass's cap, where its threads loop: 263 165 (odd, scalar form: cap 262 144) and 1 049 600 (vector form: cap 1 048 576)
LARGE = [(1, 515, 511), (1, 1025, 1024)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def assert_close(got, want, tol, what):
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))
    err = rel_err(got, want)
    print("%s: max abs err / max |ref| = %.3e (bound %.1e)" % (what, err, tol))
    assert err <= tol, "%s: max abs err / max |ref| = %.3e > %.1e" % (what, err, tol)


def to_dev(d):
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(dev()) for k, v in d.items()}


def distill_head(x, weight=1.0, eps=1.0e-8, accumulate=0, losses=None, grads=None, stats=None):
    """endo_distill_head on device tensors x[KEYS]; returns (losses, grad_pred_1, grad_pred_2), the buffers given or fresh ones."""
    n, _, h, w = x["pred_1"].shape
    losses = torch.empty(5, dtype=torch.float32, device=dev()) if losses is None else losses
    g1, g2 = (torch.empty_like(x["pred_1"]), torch.empty_like(x["pred_2"])) if grads is None else grads
    stats = torch.empty(6 * n, dtype=torch.float64, device=dev()) if stats is None else stats
    p = _lib.ptr
    rc = _lib.load().endo_distill_head(p(x["pred_1"]), p(x["pred_2"]), p(x["goal_1"]), p(x["goal_2"]), p(x["boundaries"]), weight, eps,
                                       accumulate, p(losses), p(g1), p(g2), p(stats), n, h * w, _lib.stream())
    assert rc == 0, rc
    return losses, g1, g2


def check_against_restatement(x_host, what, weight=1.0):
    x = to_dev(x_host)
    losses, g1, g2 = distill_head(x, weight=weight)
    want, w1, w2 = dr.head(*[torch.from_numpy(x_host[k]) for k in KEYS], weight=weight)
    losses = losses.cpu()
    print("%s: distill %.7f, restatement %.7f" % (what, float(losses[4]), float(want[4])))
    assert abs(float(losses[4]) - float(want[4])) <= VALUE_TOL * abs(float(want[4])), what
    assert float(losses[0]) == float(losses[4]) and losses[1:4].tolist() == [0.0, 0.0, 0.0]
    assert_close(g1, w1, GRAD_TOL, what + " grad_pred_1")
    assert_close(g2, w2, GRAD_TOL, what + " grad_pred_2")
    for key, g in (("pred_1", g1), ("pred_2", g2)):
        zero = torch.from_numpy((x_host[key] == 0) & (x_host["boundaries"] > 0))
        if bool(zero.any()):          # sgn(0) = 0 as torch.abs differentiates
            assert float(g.cpu()[zero].abs().max()) == 0.0, key
    return losses, g1, g2


# ---- 1: the head against the record and the restatement -------------------------------------------
def test_head_record(golden):
    g = golden(FIXTURE)
    x_host = dr.head_inputs(3, 24, 40, HEAD_SEED)
    losses, g1, g2 = check_against_restatement(x_host, "record shape")
    want = float(g["head::loss"])
    assert abs(float(losses[4]) - want) <= VALUE_TOL * abs(want)
    assert_close(g1, torch.from_numpy(np.array(g["head::grad_pred_1"])), GRAD_TOL, "record grad_pred_1")
    assert_close(g2, torch.from_numpy(np.array(g["head::grad_pred_2"])), GRAD_TOL, "record grad_pred_2")
    assert int(((x_host["pred_1"] == 0) & (x_host["boundaries"] > 0)).sum()) == 6


@pytest.mark.parametrize("shape", SHAPES + LARGE, ids=lambda s: "%dx%dx%d" % s)
def test_head_against_restatement(shape):
    n, h, w = shape
    check_against_restatement(dr.head_inputs(n, h, w, 100 + h), "%dx%dx%d" % shape, weight=0.75)


def test_head_with_pointers_off_sixteen_bytes():
    """hw a multiple of 4 but every map one float past a 16-byte boundary: the scalar form, same values as the aligned call."""
    x_host = dr.head_inputs(2, 32, 64, 7)
    x = to_dev(x_host)
    aligned = distill_head(x)
    off = {}
    for k in KEYS:
        buf = torch.zeros(x[k].numel() + 1, dtype=torch.float32, device=dev())
        buf[1:].copy_(x[k].reshape(-1))
        off[k] = buf[1:].view(x[k].shape)
        assert off[k].data_ptr() % 16 == 4
    gbuf = [torch.zeros(x["pred_1"].numel() + 2, dtype=torch.float32, device=dev()) for _ in range(2)]
    grads = tuple(b[1:-1].view(x["pred_1"].shape) for b in gbuf)
    losses, g1, g2 = distill_head(off, grads=grads)
    assert_close(losses[4:5], aligned[0][4:5], FUSED_VALUE_TOL, "unaligned distill")
    assert_close(g1, aligned[1], FUSED_GRAD_TOL, "unaligned grad_pred_1")
    assert_close(g2, aligned[2], FUSED_GRAD_TOL, "unaligned grad_pred_2")
    assert all(float(b[0]) == 0.0 and float(b[-1]) == 0.0 for b in gbuf)


# ---- 2: the head against the existing kernels ------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 9, 13), (2, 64, 96)], ids=lambda s: "%dx%dx%d" % s)
def test_head_matches_scale_inv_kernels(shape):
    n, h, w = shape
    weight, eps = 0.75, 1.0e-8
    x = to_dev(dr.head_inputs(n, h, w, 11, zeros=0, non_negative=True))
    losses, g1, g2 = distill_head(x, weight=weight, eps=eps)
    lib, p, s = _lib.load(), _lib.ptr, _lib.stream()
    upstream = torch.tensor([weight * 0.5], dtype=torch.float32, device=dev())
    total = 0.0
    for k, got in (("1", g1), ("2", g2)):
        loss = torch.empty(1, dtype=torch.float32, device=dev())
        stats = torch.empty(3 * n, dtype=torch.float64, device=dev())
        grad = torch.empty_like(x["pred_" + k])
        assert lib.endo_scale_inv_fwd(p(x["pred_" + k]), p(x["goal_" + k]), p(x["boundaries"]), p(loss), p(stats), n, h * w, eps, s) == 0
        assert lib.endo_scale_inv_bwd(p(upstream), p(x["pred_" + k]), p(x["goal_" + k]), p(x["boundaries"]), p(stats), p(grad), None, n,
                                      h * w, eps, s) == 0
        total = total + loss
        assert_close(got, grad, FUSED_GRAD_TOL, "grad_pred_" + k)
    assert_close(losses[4:5], 0.5 * weight * total, FUSED_VALUE_TOL, "distill")


# ---- 3: accumulate ------------------------------------------------------------------------------------
def loss_head(batch, pred_1, pred_2, losses, g1, g2):
    lib, p = _lib.load(), _lib.ptr
    n, _, h, w = pred_1.shape
    ws = torch.empty(int(lib.endo_loss_head_workspace_floats(n, h, w)), dtype=torch.float32, device=dev())
    f = lambda key: p(batch[key])
    pose = lambda key, cols: p(batch[key].reshape(n, cols))
    rc = lib.endo_loss_head(p(pred_1), p(pred_2), f("boundaries"), f("sparse_depths_1"), f("sparse_depths_2"), f("sparse_depth_masks_1"),
                            f("sparse_depth_masks_2"), f("sparse_flows_1"), f("sparse_flows_2"), f("sparse_flow_masks_1"),
                            f("sparse_flow_masks_2"), pose("translations_1_wrt_2", 3), pose("rotations_1_wrt_2", 9),
                            pose("translations_2_wrt_1", 3), pose("rotations_2_wrt_1", 9), pose("intrinsics", 9), 20.0, 0.1, 1.0e-8,
                            p(losses), p(g1), p(g2), p(ws), n, h, w, _lib.stream())
    assert rc == 0, rc
    return ws


def test_accumulate_after_a_loss_head():
    n, h, w = 2, 64, 96
    batch = to_dev(synthetic.make_batch(n, h, w, seed=21, sparse_points=300))
    x = {"pred_1": synthetic.smooth_depth(n, h, w, seed=1).to(dev()), "pred_2": synthetic.smooth_depth(n, h, w, seed=2).to(dev()),
         "goal_1": synthetic.smooth_depth(n, h, w, seed=3, lo=0.2, hi=1.4).to(dev()),
         "goal_2": synthetic.smooth_depth(n, h, w, seed=4, lo=0.2, hi=1.4).to(dev()), "boundaries": batch["boundaries"]}
    alone = distill_head(x, weight=0.5)
    losses = torch.full((5,), float("nan"), dtype=torch.float32, device=dev())
    g1, g2 = torch.empty_like(x["pred_1"]), torch.empty_like(x["pred_2"])
    ws = loss_head(batch, x["pred_1"], x["pred_2"], losses, g1, g2)
    head_losses, h1, h2 = losses[:4].clone(), g1.clone(), g2.clone()
    assert bool(torch.isfinite(head_losses).all()) and float(head_losses[3]) == 0.0 and float(h1.abs().max()) > 0
    distill_head(x, weight=0.5, accumulate=1, losses=losses, grads=(g1, g2))
    del ws
    assert_close(losses[0:1], head_losses[0:1] + alone[0][4:5], FUSED_VALUE_TOL, "total")
    assert torch.equal(losses[1:3], head_losses[1:3]) and float(losses[3]) == 0.0
    assert_close(losses[4:5], alone[0][4:5], FUSED_VALUE_TOL, "distill")
    assert_close(g1, h1 + alone[1], FUSED_GRAD_TOL, "accumulated grad_pred_1")
    assert_close(g2, h2 + alone[2], FUSED_GRAD_TOL, "accumulated grad_pred_2")
    assert float(alone[1].abs().max()) > 1e-3 * float(h1.abs().max())          # the term is visible in the sum


def test_flag_under_accumulate_and_on_an_empty_boundary():
    x = to_dev(dr.head_inputs(2, 24, 40, 5))
    zeros = lambda: (torch.zeros_like(x["pred_1"]), torch.zeros_like(x["pred_2"]))
    # a NaN head total keeps flag 1
    losses = torch.tensor([float("nan"), 1.0, 2.0, 1.0, 0.0], device=dev())
    distill_head(x, accumulate=1, losses=losses, grads=zeros())
    out = losses.cpu()
    assert bool(torch.isnan(out[0])) and out[1:4].tolist() == [1.0, 2.0, 1.0] and bool(torch.isfinite(out[4]))
    # a finite head total with the flag raised keeps it; with the flag down it stays down
    for flag in (1.0, 0.0):
        losses = torch.tensor([3.0, 1.0, 2.0, flag, 0.0], device=dev())
        distill_head(x, accumulate=1, losses=losses, grads=zeros())
        assert float(losses[3]) == flag and bool(torch.isfinite(losses[0]))
    # an empty-boundary sample: NaN total and flag 1 in both modes (the fixture's edge record)
    e = to_dev(dr.head_inputs(2, 24, 40, EDGE_SEED, empty_sample=1))
    out = distill_head(e)[0].cpu()
    assert [bool(v) for v in torch.isnan(out)] == [True, False, False, False, True] and out[1:4].tolist() == [0.0, 0.0, 1.0]
    losses = torch.tensor([3.0, 1.0, 2.0, 0.0, 0.0], device=dev())
    distill_head(e, accumulate=1, losses=losses, grads=zeros())
    out = losses.cpu()
    assert bool(torch.isnan(out[0])) and out[1:4].tolist() == [1.0, 2.0, 1.0] and bool(torch.isnan(out[4]))


# ---- 4: the workspace contract ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 9, 13), (2, 32, 64)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_workspace_contract(shape, accumulate):
    """Guard bands stay intact, and NaN-poisoned stats / losses / (accumulate = 0) gradients give the zero-filled run's results bit for
    bit: one reduce block per row at these shapes, so the sums have one order."""
    n, h, w = shape
    x = to_dev(dr.head_inputs(n, h, w, 3))
    results = []
    for fill in ("poison", "zeros"):
        with guarded(device="cuda", fill=fill) as g:
            losses = torch.empty(5, dtype=torch.float32, device=dev())
            stats = torch.empty(6 * n, dtype=torch.float64, device=dev())
            g1, g2 = torch.empty_like(x["pred_1"]), torch.empty_like(x["pred_2"])
            if fill == "poison":
                assert bool(torch.isnan(losses).all()) and bool(torch.isnan(stats).all()) and bool(torch.isnan(g1).all())
            if accumulate:          # what a loss head left: these are inputs
                losses[:4].copy_(torch.tensor([3.0, 1.0, 2.0, 0.0]))
                g1.fill_(0.25)
                g2.fill_(-0.5)
            distill_head(x, weight=0.5, accumulate=accumulate, losses=losses, grads=(g1, g2), stats=stats)
            torch.cuda.synchronize()
            assert g.check() == 4
            results.append((losses.clone(), g1.clone(), g2.clone(), stats.clone()))
    for a, b in zip(*results):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    stats = results[0][3].reshape(2 * n, 3)
    assert torch.equal(stats[:n, 2], x["boundaries"].double().sum((1, 2, 3))) and torch.equal(stats[n:, 2], stats[:n, 2])


def test_bad_arguments_on_device_buffers():
    x = to_dev(dr.head_inputs(1, 8, 12, 3))
    lib, p = _lib.load(), _lib.ptr
    losses = torch.zeros(5, device=dev())
    g1, g2 = torch.zeros_like(x["pred_1"]), torch.zeros_like(x["pred_2"])
    stats = torch.zeros(6, dtype=torch.float64, device=dev())
    good = [p(x[k]) for k in KEYS] + [1.0, 1.0e-8, 0, p(losses), p(g1), p(g2), p(stats), 1, 96, _lib.stream()]
    assert lib.endo_distill_head(*good) == 0
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11):
        bad = list(good)
        bad[i] = None
        assert lib.endo_distill_head(*bad) == -1, i
    for i, value in ((12, 0), (12, -1), (13, 0), (13, -5), (5, -0.5), (5, float("nan")), (7, 2), (7, -1)):
        bad = list(good)
        bad[i] = value
        assert lib.endo_distill_head(*bad) == -1, (i, value)
    torch.cuda.synchronize()
    assert float(losses[3]) == 0.0 and bool(torch.isfinite(losses).all())


# ---- 5 - 9: the step ----------------------------------------------------------------------------------------
def network(seed, train):
    model = ea.FCDenseNet57(1)
    model.load_state_dict(onet.keep_depth_positive(onet.perturb_affine(onet.synthetic_state(seed), seed + 1)))
    model = model.to(dev())
    return model.train() if train else model.eval()


def fixture_networks(g):
    _, _, _, teacher_seed, student_seed, _ = (int(v) for v in np.array(g["step::shape"]))
    return network(teacher_seed, False), network(student_seed, True)


def teacher_state(teacher):
    return teacher.flat_parameters().clone(), teacher._flat_bn.clone(), teacher._nbt.clone()


def assert_teacher_untouched(teacher, before):
    for now, was in zip(teacher_state(teacher), before):
        assert torch.equal(now, was)
    assert teacher.flat_gradients(create=False) is None and all(q.grad is None for q in teacher.parameters())


def pure_batch(n, h, w, seed):
    batch = synthetic.make_batch(n, h, w, seed=seed, sparse_points=500)
    return to_dev({k: batch[k] for k in ("colors_1", "colors_2", "boundaries")})


def test_step_record(golden):
    g = golden(FIXTURE)
    n, h, w, _, _, batch_seed = (int(v) for v in np.array(g["step::shape"]))
    teacher, student = fixture_networks(g)
    before = teacher_state(teacher)
    opt = ea.optim.FusedClipSGD(student, lr=1.0e-3)
    step = ea.train_step.DistillationStep(student, teacher, opt, h, w)
    preds = []
    inner = step._fused_iteration

    def keep_predictions(batch):
        result = inner(batch)
        preds.append(result[3])
        return result
    step._fused_iteration = keep_predictions
    for it in range(2):
        tag = "step::%d::" % it
        flat_before = student.flat_parameters().double().clone()
        out = step(pure_batch(n, h, w, batch_seed + it))
        want = float(g[tag + "loss"])
        tol = 1e-4 if it == 0 else 1e-3
        print("iteration %d: loss %.7f (record %.7f), grad norm %.4f (record %.4f)" % (it, out["loss"], want, float(out["grad_norm"]),
                                                                                      float(g[tag + "grad_norm"])))
        assert abs(out["loss"] - want) <= tol * abs(want)
        assert abs(float(out["distill"]) - want) <= tol * abs(want) and float(out["dcl"]) == 0.0 and float(out["sfl"]) == 0.0
        assert out["skipped"] is False and sorted(out.keys()) == ["dcl", "distill", "grad_norm", "loss", "sfl", "skipped"]
        assert_close(out["grad_norm"], torch.from_numpy(np.array(g[tag + "grad_norm"])).double(), 5e-3, "grad norm")
        norms = np.array([float(q.detach().double().norm()) for q in student.parameters()])
        np.testing.assert_allclose(norms, np.array(g[tag + "param_norms"]), rtol=1e-4, atol=1e-5)
        if it == 0:
            n_half = preds[0].shape[0] // 2
            assert_close(preds[0][:n_half], torch.from_numpy(np.array(g[tag + "pred_1"])), 1e-4, "pred_1")
            update = float((student.flat_parameters().double() - flat_before).norm())
            want_update = float(g[tag + "update_norm"])
            print("update norm %.6e (record %.6e)" % (update, want_update))
            assert abs(update - want_update) <= 5e-3 * want_update
    assert_teacher_untouched(teacher, before)
    with pytest.raises(RuntimeError, match="pure mode"):
        step.display_panels()


def test_combined_record(golden):
    g = golden(FIXTURE)
    n, h, w, _, _, batch_seed = (int(v) for v in np.array(g["step::shape"]))
    teacher, student = fixture_networks(g)
    before = teacher_state(teacher)
    sfl_weight, dcl_weight, distill_weight = (float(v) for v in np.array(g["combined::weights"]))
    opt = ea.optim.FusedClipSGD(student, lr=1.0e-3)
    step = ea.train_step.DistillationStep(student, teacher, opt, h, w, distill_weight=distill_weight, sfl_weight=sfl_weight,
                                          dcl_weight=dcl_weight)
    flat_before = student.flat_parameters().double().clone()
    out = step(to_dev(synthetic.make_batch(n, h, w, seed=batch_seed, sparse_points=500)))
    want = np.array(g["combined::losses"], dtype=np.float64)
    got = np.array([out["loss"], float(out["dcl"]), float(out["sfl"]), float(out["distill"])])
    print("combined [total, dcl, sfl, distill]: %s (record %s)" % (got, want))
    assert (np.abs(got - want) <= 1e-4 * np.abs(want)).all()
    assert abs(got[0] - got[1:].sum()) <= 1e-6 * got[0]
    assert_close(out["grad_norm"], torch.from_numpy(np.array(g["combined::grad_norm"])).double(), 5e-3, "grad norm")
    norms = np.array([float(q.detach().double().norm()) for q in student.parameters()])
    np.testing.assert_allclose(norms, np.array(g["combined::param_norms"]), rtol=1e-4, atol=1e-5)
    update = float((student.flat_parameters().double() - flat_before).norm())
    assert abs(update - float(g["combined::update_norm"])) <= 5e-3 * float(g["combined::update_norm"])
    assert_teacher_untouched(teacher, before)
    panel = step.display_panels()
    assert panel.dtype == torch.uint8 and panel.dim() == 3 and panel.shape[2] == 3


def test_step_against_learn_from_teacher():
    n, h, w = 2, 64, 96
    teacher, student, twin = network(24, False), network(4, True), network(4, True)
    before = teacher_state(teacher)
    batch = pure_batch(n, h, w, 100)
    step = ea.train_step.DistillationStep(student, teacher, ea.optim.FusedClipSGD(student, lr=1.0e-3), h, w)
    out = step(batch)
    twin_opt = ea.optim.FusedClipSGD(twin, lr=1.0e-3)
    b = batch["boundaries"]
    c1, c2 = ea.train_step.mask_mul(batch["colors_1"], b), ea.train_step.mask_mul(batch["colors_2"], b)
    loss, p1, p2, g1, g2 = ea.utils.learn_from_teacher(b, c1, c2, teacher, twin, ea.ScaleInvariantLoss(epsilon=1.0e-8))
    assert loss.requires_grad and p1.shape == p2.shape == g1.shape == g2.shape == (n, 1, h, w) and not g1.requires_grad
    assert float(p1.min()) >= 0 and float(g1.min()) >= 0
    twin_opt.zero_grad()
    loss.backward()
    norm = twin_opt.step()
    print("loss %.8f / %.8f, grad norm %.6f / %.6f" % (out["loss"], float(loss), float(out["grad_norm"]), float(norm)))
    assert abs(out["loss"] - float(loss)) <= 1e-6 * abs(float(loss))
    assert_close(out["grad_norm"], norm.cpu(), 5e-5, "grad norm")
    assert_close(student.flat_parameters(), twin.flat_parameters(), 1e-6, "parameters after one iteration")
    # the module form of the same loss: ScaleInvariantLoss on each frame (the reference's own composition)
    sil = ea.ScaleInvariantLoss(epsilon=1.0e-8)
    with torch.no_grad():
        module = 0.5 * (sil([p1, g1, b]) + sil([p2, g2, b]))
    assert abs(float(module) - float(loss)) <= 1e-6 * abs(float(loss))
    assert_teacher_untouched(teacher, before)


def test_guard_skips_the_step():
    n, h, w = 2, 64, 96
    teacher, student = network(24, False), network(4, True)
    opt = ea.optim.FusedClipSGD(student, lr=1.0e-3)
    step = ea.train_step.DistillationStep(student, teacher, opt, h, w)
    first = step(pure_batch(n, h, w, 100))
    assert first["skipped"] is False
    params, momentum = student.flat_parameters().clone(), opt._momentum.clone()
    assert float(momentum.abs().max()) > 0
    batch = pure_batch(n, h, w, 101)
    batch["boundaries"][1] = 0.0
    out = step(batch)
    assert out["skipped"] is True and not np.isfinite(out["loss"]) and bool(torch.isnan(out["distill"]))
    assert torch.equal(student.flat_parameters(), params) and torch.equal(opt._momentum, momentum)


def test_validate_in_pure_mode():
    n, h, w = 2, 64, 96
    teacher, student = network(24, False), network(4, True)
    opt = ea.optim.FusedClipSGD(student, lr=1.0e-3)
    step = ea.train_step.DistillationStep(student, teacher, opt, h, w)
    batches = [pure_batch(n, h, w, 100), pure_batch(n, h, w, 101)]
    params = student.flat_parameters().clone()
    each = [step.validation_losses(batch).cpu() for batch in batches]          # train mode: batch statistics, so a repeat gives the same totals
    assert all(v.shape == (5,) and float(v[3]) == 0.0 and float(v[0]) == float(v[4]) and v[1:3].tolist() == [0.0, 0.0] for v in each)
    result = ea.train_step.validate(step, batches)
    mean = 0.5 * (float(each[0][0]) + float(each[1][0]))
    assert abs(result.mean_loss - mean) <= 1e-6 * mean and result.mean_depth_consistency_loss == 0.0 and result.mean_sparse_flow_loss == 0.0
    assert result.losses.shape == (2, 3) and abs(float(result.running_means[0, 0]) - float(each[0][0])) <= 1e-6 * mean
    assert torch.equal(student.flat_parameters(), params)
    grads = student.flat_gradients(create=False)
    assert grads is None or float(grads.abs().max()) == 0.0
    assert opt._momentum is None


def test_constructor_refuses_models_on_different_devices():
    teacher, student = ea.FCDenseNet57(1), network(4, True)
    with pytest.raises(ValueError, match="student on"):
        ea.train_step.DistillationStep(student, teacher, ea.optim.FusedClipSGD(student, lr=1.0e-3), 64, 96)
