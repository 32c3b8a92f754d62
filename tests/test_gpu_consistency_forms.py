"""The consistency-loss choice on the device: endo_loss_head_forms, endo_warp_consistency_forms (losses.warp_consistency(form=...)) and
TrainingStep(consistency_loss=...) with NormalizedL2Loss, NormalizedL1Loss and NormalizedWeightedMaskedL2Loss inside the fused kernels
of csrc/geometry.hip.

Bounds.  Against the reference's records (tests/golden/consistency_forms.npz, fp64 values): 4 x the reference's own fp32-against-fp64
error stored beside them, never tighter than 1e-6 of max |ref| (consistency_forms_restate.record_bound) -- the device adds its sums
by atomics in another order than torch.  The same kernels on the same arguments (form 0 through the new entries against the old ones;
poisoned against zero-filled buffers; the fused head against the module path): 1e-6 of max |ref| on every output, each loss term on
its own scale -- only the order of the atomic adds differs.  The stand-alone entry against DepthWarpingLayer -> loss module under
autograd, which adds a gradient's contributions in a fixed order: the bounds of tests/test_gpu_parity.py::test_warp_consistency_call
for that comparison, 1e-6 for the loss and d / d depth 1, 1e-5 for d / d depth 2.

Measured on an MI355X (max abs error / max |ref| against the fp64 record; the reference's own fp32 error -> bound in brackets; also DESIGN.md 4.5):
    head record, l2 / l1 / weighted_l2:  losses 1.30e-7 / 1.29e-7 / 1.30e-7 (2.6e-8 / 4.9e-8 / 2.6e-8 -> 1.0e-6),
        d total / d pred_1 8.1e-7 / 8.7e-7 / 9.1e-7 (1.19e-6 / 1.14e-6 / 1.12e-6 -> 4.8e-6 / 4.6e-6 / 4.5e-6), d total / d pred_2 5.4e-7 (5.5e-7 -> 2.2e-6)
    weighted_l2 step record, iteration 0 / 1:  losses 4.1e-7 / 7.7e-8 (3.8e-7 / 3.0e-7 -> 1.5e-6 / 1.2e-6),
        gradient norm 3.7e-5 / 1.8e-4 (1.1e-4 / 2.0e-4 -> 4.4e-4 / 7.8e-4), pred_1 4.9e-7 / 6.0e-6 (6.7e-7 / 6.2e-6 -> 2.7e-6 / 2.5e-5)
    fused head against fused_head=False at 2 x 64 x 96: identical in all four numbers, every form.
    form 0 through the new entries against the old ones: losses 0, gradients <= 9.3e-8; poisoned against zero-filled buffers <= 5.2e-8.
    stand-alone entry against the device chain, sixteen cases: loss <= 2.3e-7, d / d depth 1 <= 1.8e-7, d / d depth 2 <= 3.5e-7."""

import ctypes
import importlib

import numpy as np
import pytest
import torch

import consistency_forms_restate as cr
import test_gpu_bf16 as t16
import test_gpu_parity as tp
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
_lib = ea._lib
FIXTURE = "consistency_forms.npz"
CODES = {name: entry[0] for name, entry in ea.losses.CONSISTENCY_FORMS.items()}          # ENDO_CONSISTENCY_*
SAME_ARITHMETIC, SCATTER = 1e-6, 1e-5


def ptr(t):
    return _lib.ptr(t)


def head_arguments(db, p1, p2):
    n = p1.shape[0]
    pose = lambda key, cols: db[key].reshape(n, cols).contiguous()
    keep = [p1, p2, db["boundaries"], db["sparse_depths_1"], db["sparse_depths_2"], db["sparse_depth_masks_1"], db["sparse_depth_masks_2"],
            db["sparse_flows_1"], db["sparse_flows_2"], db["sparse_flow_masks_1"], db["sparse_flow_masks_2"], pose("translations_1_wrt_2", 3),
            pose("rotations_1_wrt_2", 9), pose("translations_2_wrt_1", 3), pose("rotations_2_wrt_1", 9), pose("intrinsics", 9)]
    return keep


def call_head(form, db, p1, p2, eps=None, entry="forms"):
    """endo_loss_head_forms (photo_weight 0, null colours) or endo_loss_head on device tensors: ([total, dcl, sfl, flag], g1, g2).
    Buffers come from torch.empty, so inside guarded() they are guarded and poisoned."""
    lib = _lib.load()
    n, _, h, w = p1.shape
    keep = head_arguments(db, p1.contiguous(), p2.contiguous())
    ws = torch.empty(int(lib.endo_loss_head_workspace_floats(n, h, w)), dtype=torch.float32, device=p1.device)
    losses = torch.empty(4, dtype=torch.float32, device=p1.device)
    g1, g2 = torch.empty_like(keep[0]), torch.empty_like(keep[1])
    out = [ptr(losses), ptr(g1), ptr(g2), ptr(ws), n, h, w]
    if entry == "forms":
        eps = cr.DEFAULT_EPS[form] if eps is None else eps
        _lib.check(lib.endo_loss_head_forms(*[ptr(t) for t in keep], None, None, cr.SFL_WEIGHT, cr.DCL_WEIGHT, 0.0, cr.EPSILON, 0, *out,
                                            CODES[form], eps, _lib.stream()), "endo_loss_head_forms")
    else:
        _lib.check(lib.endo_loss_head(*[ptr(t) for t in keep], cr.SFL_WEIGHT, cr.DCL_WEIGHT, cr.EPSILON, *out, _lib.stream()), "endo_loss_head")
    torch.cuda.synchronize()
    return losses, g1, g2


def consistency(form, db, d1, d2, **kw):
    return ea.losses.warp_consistency(d1, d2, db["boundaries"], db["translations_1_wrt_2"], db["rotations_1_wrt_2"],
                                      db["translations_2_wrt_1"], db["rotations_2_wrt_1"], db["intrinsics"], form=form, **kw)


def module_of(form, h, w):
    return ea.train_step.consistency_loss_spec(form, h, w)[1]


def device_chain(form, db, d1, d2, dcl_weight):
    """DepthWarpingLayer -> the loss module of ``form`` under autograd on the device: (loss, d / d d1, d / d d2)."""
    n, _, h, w = d1.shape
    g1, g2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
    warp, loss = ea.DepthWarpingLayer(), module_of(form, h, w)
    p12 = [db["translations_1_wrt_2"], db["rotations_1_wrt_2"], db["intrinsics"]]
    p21 = [db["translations_2_wrt_1"], db["rotations_2_wrt_1"], db["intrinsics"]]
    w21, i1 = warp([g1, g2, db["boundaries"]] + p12)
    w12, i2 = warp([g2, g1, db["boundaries"]] + p21)
    fourth = {"distance": ([db["intrinsics"]], [db["intrinsics"]]), "weighted_l2": ([p12[0]], [p21[0]])}.get(form, ([], []))
    value = dcl_weight * 0.5 * (loss([g1, w21, i1] + fourth[0]) + loss([g2, w12, i2] + fourth[1]))
    value.backward()
    return value.detach(), g1.grad, g2.grad, (i1, i2)


def spin_batch(n, h, w, seed, angle):
    """make_batch with an in-plane rotation of ``angle`` rad put in front of every pose: a 16 x 32 output tile's source box then grows by
    ~32 sin(angle) rows, past the staging buffers' margin of 8 -- the blocks take the gather fallback."""
    batch = ea.synthetic.make_batch(n, h, w, seed=seed, sparse_points=min(500, h * w // 6))
    c, s = float(np.cos(angle)), float(np.sin(angle))
    spin = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    r12 = torch.matmul(spin, batch["rotations_1_wrt_2"])
    batch["rotations_1_wrt_2"] = r12.contiguous()
    batch["rotations_2_wrt_1"] = r12.transpose(1, 2).contiguous()
    batch["translations_2_wrt_1"] = torch.matmul(-r12.transpose(1, 2), batch["translations_1_wrt_2"]).contiguous()
    return batch


@pytest.mark.parametrize("form", cr.NEW_FORMS)
def test_head_forms_against_record(golden, form):
    """endo_loss_head_forms against the reference's head record (N = 4, 24 x 40): [total, dcl, sfl] and d total / d prediction of both
    frames, held to the record's fp64 values within 4 x the reference's own fp32 error (>= 1e-6 of max |ref|).
    Measured on an MI355X, max abs error / max |ref| (bound), l2 / l1 / weighted_l2: losses 1.30e-7 / 1.29e-7 / 1.30e-7 (1.0e-6),
    d total / d pred_1 8.1e-7 / 8.7e-7 / 9.1e-7 (4.8e-6 / 4.6e-6 / 4.5e-6), d total / d pred_2 5.4e-7 (2.2e-6)."""
    g = golden(FIXTURE)
    db = tp.to_dev(cr.head_batch())
    p1 = torch.from_numpy(np.array(g["head::pred_1"])).to(tp.dev())
    p2 = torch.from_numpy(np.array(g["head::pred_2"])).to(tp.dev())
    losses, g1, g2 = call_head(form, db, p1, p2)
    assert float(losses[3]) == 0.0
    problems = []
    for name, got in (("losses", losses[:3]), ("grad_pred_1", g1), ("grad_pred_2", g2)):
        want64, want32 = np.array(g["head::%s::%s_f64" % (form, name)]), np.array(g["head::%s::%s_f32" % (form, name)])
        err = float(np.abs(got.double().cpu().numpy() - want64).max())
        bound, scale = cr.record_bound(want64, want32), float(np.abs(want64).max())
        print("head %-11s %-11s device against fp64 %.2e of max |ref| (bound %.2e; the reference's fp32 %.2e)" % (
            form, name, err / scale, bound / scale, float(np.abs(want32.astype(np.float64) - want64).max()) / scale))
        if err > bound:
            problems.append("%s %s: %.3e > %.3e" % (form, name, err / scale, bound / scale))
    assert not problems, "\n".join(problems)


def test_form_zero_through_new_entries():
    """ENDO_CONSISTENCY_DISTANCE through endo_loss_head_forms / endo_warp_consistency_forms runs endo_loss_head's /
    endo_warp_consistency's kernels: every output equal within the atomics' order, 1e-6 of max |ref|."""
    n, h, w = 3, 40, 72
    batch, p1, p2, _ = tp.geometry_inputs(n, h, w, 61)
    db = tp.to_dev(batch)
    p1, p2 = p1.to(tp.dev()), p2.to(tp.dev())
    old, new = call_head("distance", db, p1, p2, entry="plain"), call_head("distance", db, p1, p2)
    assert float(new[0][3]) == 0.0 and float(new[0][1]) > 0
    for got, want, what in zip(new, old, ("losses", "grad pred 1", "grad pred 2")):
        tp.assert_close(got, want, SAME_ARITHMETIC, "form 0 through endo_loss_head_forms: " + what)
    lib = _lib.load()
    ws = torch.empty(int(lib.endo_warp_consistency_workspace_floats(n, h, w)), dtype=torch.float32, device=tp.dev())
    results = []
    for forms in (False, True):
        loss = torch.empty((), dtype=torch.float32, device=tp.dev())
        g1, g2 = torch.empty_like(p1), torch.empty_like(p2)
        pose = lambda key, cols: db[key].reshape(n, cols).contiguous()
        args = [ptr(p1), ptr(p2), ptr(db["boundaries"]), ptr(pose("translations_1_wrt_2", 3)), ptr(pose("rotations_1_wrt_2", 9)),
                ptr(pose("translations_2_wrt_1", 3)), ptr(pose("rotations_2_wrt_1", 9)), ptr(pose("intrinsics", 9)), 0.7, cr.EPSILON,
                ptr(loss), ptr(g1), ptr(g2), ptr(ws), n, h, w]
        if forms:
            _lib.check(lib.endo_warp_consistency_forms(*args, 0, 1.0e-5, _lib.stream()), "endo_warp_consistency_forms")
        else:
            _lib.check(lib.endo_warp_consistency(*args, _lib.stream()), "endo_warp_consistency")
        torch.cuda.synchronize()
        results.append((loss, g1, g2))
    print("form 0 through the new entries against the old ones: head %s, stand-alone %s" % (
        ["%.1e" % tp.rel_err(a, b) for a, b in zip(new, old)], ["%.1e" % tp.rel_err(a, b) for a, b in zip(results[1], results[0])]))
    for got, want, what in zip(results[1], results[0], ("loss", "grad 1", "grad 2")):
        tp.assert_close(got, want, SAME_ARITHMETIC, "form 0 through endo_warp_consistency_forms: " + what)


# (n, h, w, seed, in-plane spin): exactly one 16 x 32 tile; one row and one column more; the finalize's lane loop (2 n = 66 > 64 lanes);
# a pose that makes the blocks' taps leave the staged tile
CHAIN_CASES = [(1, 16, 32, 71, 0.0), (1, 17, 33, 72, 0.0), (33, 16, 32, 73, 0.0), (2, 48, 64, 74, 0.6)]


@pytest.mark.parametrize("form", cr.FORMS)
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: "%dx%dx%d%s" % (c[0], c[1], c[2], "-spin" if c[4] else ""))
def test_warp_consistency_forms_against_device_chain(case, form):
    """losses.warp_consistency(form=...) against DepthWarpingLayer -> the form's loss module under autograd on the device: the same
    arithmetic per pixel, sums and scatter-adds in another order.  Bounds of test_gpu_parity.py::test_warp_consistency_call for this
    comparison: loss and d / d depth 1 1e-6 of max |ref|, d / d depth 2 1e-5.  Measured (printed): DESIGN.md 4.5."""
    n, h, w, seed, spin = case
    batch = spin_batch(n, h, w, seed, spin) if spin else ea.synthetic.make_batch(n, h, w, seed=seed, sparse_points=min(500, h * w // 6))
    if n > 1:          # translations of different norms: the weighted form's weights differ across the batch
        batch = cr.scale_translations(batch, [0.5 + 1.5 * (i % 4) for i in range(n)])
    db = tp.to_dev(batch)
    d1 = ea.synthetic.smooth_depth(n, h, w, seed=seed + 100).to(tp.dev())
    d2 = ea.synthetic.smooth_depth(n, h, w, seed=seed + 200).to(tp.dev())
    want, w1, w2, (i1, i2) = device_chain(form, db, d1, d2, 0.7)
    assert float(i1.sum()) > 0 and float(i2.sum()) > 0 and bool(torch.isfinite(want))
    lib = _lib.load()
    fwd, bwd = ctypes.c_longlong(), ctypes.c_longlong()
    assert lib.endo_warp_fallback_blocks(None, None, 1) == 0
    loss, g1, g2 = consistency(form, db, d1, d2, dcl_weight=0.7)
    torch.cuda.synchronize()
    assert lib.endo_warp_fallback_blocks(ctypes.byref(fwd), ctypes.byref(bwd), 1) == 0
    print("%s %s: %d forward / %d backward blocks took the gather fallback" % (form, case[:3], fwd.value, bwd.value))
    if spin:
        assert fwd.value > 0 and bwd.value > 0, "the spun pose did not exercise the gather fallback"
    print("    against the device chain: loss %.1e, grad 1 %.1e, grad 2 %.1e" % (tp.rel_err(loss, want), tp.rel_err(g1, w1), tp.rel_err(g2, w2)))
    tp.assert_close(loss, want, SAME_ARITHMETIC, "%s loss vs the device chain %s" % (form, case[:3]))
    tp.assert_close(g1, w1, SAME_ARITHMETIC, "%s grad 1 vs the device chain %s" % (form, case[:3]))
    tp.assert_close(g2, w2, SCATTER, "%s grad 2 vs the device chain %s" % (form, case[:3]))
    assert float(g1.abs().max()) > 0 and float(g2.abs().max()) > 0


def one_pixel_batch(n, h, w, seed):
    """A batch whose intersect masks hold ONE pixel per sample and direction: a 2 x 2 boundary under a pose of 1e-3 sideways (the
    sample location of a pixel is half a pixel off the grid, so only the pixel whose four taps are the block passes the 0.9 threshold).
    There sum m = 1 and the eps of NormalizedL2Loss / NormalizedL1Loss, which only enters mu = sum m a / (eps + sum m) under the factor
    1e-5, moves the value by ~1e-5 of itself between eps = 1e-3 and eps = 50 (1e-5 / sum m): visible in fp32."""
    batch = ea.synthetic.make_batch(n, h, w, seed=seed, sparse_points=20)
    mask = torch.zeros(n, 1, h, w)
    mask[:, :, 6:8, 10:12] = 1.0
    batch["boundaries"] = mask
    batch["rotations_1_wrt_2"] = torch.eye(3).repeat(n, 1, 1)
    batch["rotations_2_wrt_1"] = torch.eye(3).repeat(n, 1, 1)
    t = torch.tensor([1.0e-3, 0.0, 0.0]).reshape(1, 3, 1).repeat(n, 1, 1)
    batch["translations_1_wrt_2"], batch["translations_2_wrt_1"] = t, -t
    return batch


def test_custom_eps_reaches_the_kernels():
    """form_eps is the module's eps: value and gradients are the module's with that eps (1e-6 / 1e-6 / 1e-5, as against the device chain),
    and differ from the default eps's -- weighted_l2 on an ordinary batch (eps is added to the depth mass: > 1e-2 of the value), l2 and
    l1 on one_pixel_batch (> 4e-6 of the value, where the CPU restatement gives 9.1e-6 and 9.6e-6)."""
    for form, eps, module, n, h, w in (("l2", 50.0, ea.losses.NormalizedL2Loss(eps=50.0), 1, 16, 32),
                                       ("l1", 50.0, ea.losses.NormalizedL1Loss(eps=50.0), 1, 16, 32),
                                       ("weighted_l2", 7.0, ea.losses.NormalizedWeightedMaskedL2Loss(epsilon=7.0), 2, 24, 40)):
        batch = ea.synthetic.make_batch(n, h, w, seed=75, sparse_points=100) if form == "weighted_l2" else one_pixel_batch(n, h, w, 76)
        db = tp.to_dev(batch)
        d1 = ea.synthetic.smooth_depth(n, h, w, seed=176).to(tp.dev())
        d2 = ea.synthetic.smooth_depth(n, h, w, seed=276).to(tp.dev())
        default, _, _ = consistency(form, db, d1, d2)
        loss, g1, g2 = consistency(form, db, d1, d2, form_eps=eps)
        c1, c2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
        warp = ea.DepthWarpingLayer()
        w21, i1 = warp([c1, c2, db["boundaries"], db["translations_1_wrt_2"], db["rotations_1_wrt_2"], db["intrinsics"]])
        w12, i2 = warp([c2, c1, db["boundaries"], db["translations_2_wrt_1"], db["rotations_2_wrt_1"], db["intrinsics"]])
        if form != "weighted_l2":
            assert float(i1.sum()) == float(i2.sum()) == float(n)
        fourth = ([db["translations_1_wrt_2"]], [db["translations_2_wrt_1"]]) if form == "weighted_l2" else ([], [])
        want = 0.5 * (module([c1, w21, i1] + fourth[0]) + module([c2, w12, i2] + fourth[1]))
        want.backward()
        moved = abs(float(loss) - float(default)) / abs(float(default))
        print("%s eps %g: against the module %.1e / %.1e / %.1e, value moved from the default eps's by %.2e" % (
            form, eps, tp.rel_err(loss, want), tp.rel_err(g1, c1.grad), tp.rel_err(g2, c2.grad), moved))
        tp.assert_close(loss, want.detach(), SAME_ARITHMETIC, form + " with its own eps")
        tp.assert_close(g1, c1.grad, SAME_ARITHMETIC, form + " with its own eps, grad 1")
        tp.assert_close(g2, c2.grad, SCATTER, form + " with its own eps, grad 2")
        assert moved > (1e-2 if form == "weighted_l2" else 4e-6), (form, moved)


def test_empty_intersect_record(golden):
    """The record whose sample 1 leaves the frame: NaN and guard flag 1 for l2 / l1 (0 / 0, as the reference), flag 0 and the
    reference's finite value for weighted_l2 (its fp32 record, so 1e-5 of max |ref|: the loss bound of test_warp_consistency_call)."""
    g = golden(FIXTURE)
    db = tp.to_dev(cr.empty_batch())
    p1 = torch.from_numpy(np.array(g["head::pred_1"])).to(tp.dev())
    p2 = torch.from_numpy(np.array(g["head::pred_2"])).to(tp.dev())
    for form, nan in zip(cr.NEW_FORMS, np.array(g["empty::nan"]).tolist()):
        losses, g1, g2 = call_head(form, db, p1, p2)
        want = torch.from_numpy(np.array(g["empty::%s::losses_f32" % form]))
        assert float(losses[3]) == float(nan), form
        if nan:
            assert bool(torch.isnan(losses[0])) and bool(torch.isnan(losses[1])) and bool(torch.isfinite(losses[2]))
        else:
            tp.assert_close(losses[:3], want, 1e-5, "weighted_l2 on the empty-intersect record")
            assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all())


@pytest.mark.parametrize("form", cr.NEW_FORMS)
def test_step_skips_an_empty_intersect_and_recovers(form):
    """A batch one of whose samples leaves the frame: l2 / l1 skip the step (flag 1, no parameter change), weighted_l2 trains on it.  The
    next clean step ends where a twin without the first step ends (bounds of test_gpu_parity.py::test_clean_step_after_a_skipped_step)."""
    n, h, w = 2, 64, 96
    bad = cr.throw_out_of_frame(ea.synthetic.make_batch(n, h, w, seed=82, sparse_points=300), 1)
    good = ea.synthetic.make_batch(n, h, w, seed=83, sparse_points=300)
    results = []
    for with_first_step in (True, False):
        _, model = tp.make_model(58, positive_depth=True)
        model.train()
        step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-3), h, w, consistency_loss=form)
        running0 = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}
        if with_first_step:
            before = model.flat_parameters().clone()
            out = step(tp.to_dev(bad), lr=1.0e-3)
            if form == "weighted_l2":
                assert not out["skipped"] and np.isfinite(out["loss"]) and not torch.equal(before, model.flat_parameters())
                return
            assert out["skipped"] and np.isnan(out["loss"]) and torch.equal(before, model.flat_parameters())
            model.load_state_dict(running0, strict=False)          # the skipped forward updated the running statistics, as the reference's
        out = step(tp.to_dev(good), lr=1.0e-3)
        torch.cuda.synchronize()
        assert not out["skipped"]
        results.append((out["loss"], float(out["grad_norm"]), model.flat_parameters().clone()))
    (l_a, g_a, p_a), (l_b, g_b, p_b) = results
    assert np.isfinite(l_a) and np.isfinite(g_a) and bool(torch.isfinite(p_a).all())
    assert abs(l_a - l_b) <= 1e-6 * abs(l_b), (l_a, l_b)
    assert abs(g_a - g_b) <= 5e-5 * g_b, (g_a, g_b)
    tp.assert_close(p_a, p_b, 1e-6, "parameters after the clean step")


def step_bound(g, i, name):
    want64, want32 = np.array(g["step::%d::%s_f64" % (i, name)]), np.array(g["step::%d::%s_f32" % (i, name)])
    return want64, cr.record_bound(want64, want32)


@pytest.mark.parametrize("form", cr.NEW_FORMS)
def test_training_step_fused_against_module_path(golden, form):
    """TrainingStep(consistency_loss=form) at 2 x 64 x 96: validation_losses of the fused head against the module path
    (fused_head=False) on the same network.  Both run the same arithmetic on the same predictions, so each of total, dcl and sfl is held
    to 1e-6 of ITSELF: never looser than 4 x the reference's fp32 error with its floor of 1e-6, and a difference in dcl alone shows.
    Measured: identical in every number, every form.  Then display_panels() and validate() on the non-default step."""
    g = golden(FIXTURE)
    n, h, w, seed, batch_seed = (int(v) for v in np.array(g["step::shape"]))
    batch = tp.to_dev(ea.synthetic.make_batch(n, h, w, seed=batch_seed, sparse_points=500))
    state, model = tp.make_model(seed, positive_depth=True)
    model.train()
    running0 = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}
    fused = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-3), h, w, consistency_loss=form)
    plain = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-3), h, w, consistency_loss=form, fused_head=False)
    assert fused.fused_head and not plain.fused_head
    got = fused.validation_losses(batch)
    panel = fused.display_panels()
    model.load_state_dict(running0, strict=False)
    want = plain.validation_losses(batch)
    torch.cuda.synchronize()
    print("%s: fused [total, dcl, sfl, flag] %s, module path %s" % (form, got.tolist(), want.tolist()))
    assert got.shape == want.shape == (4,) and float(got[3]) == 0.0 and float(got[1]) > 0
    for i, name in enumerate(("total", "dcl", "sfl")):          # each on its own scale: dcl is 1 / 170 of the total
        tp.assert_close(got[i], want[i], SAME_ARITHMETIC, "%s: %s of the fused head against the module path" % (form, name))
    assert panel.dtype == torch.uint8 and panel.dim() == 3 and panel.shape[2] == 3 and int(panel.max()) > 0
    batches = [batch, tp.to_dev(ea.synthetic.make_batch(n, h, w, seed=batch_seed + 1, sparse_points=500))]
    shown = []
    result = ea.train_step.validate(fused, batches, display_each=1, on_display=lambda i, p: shown.append((i, tuple(p.shape))))
    assert result.losses.shape == (2, 3) and np.isfinite(result.losses).all() and np.isfinite(result.mean_loss)
    assert [i for i, _ in shown] == [0, 1] and shown[0][1] == tuple(panel.shape)
    model.load_state_dict(running0, strict=False)
    assert abs(float(result.losses[0, 0]) - float(got[0])) <= 1e-6 * abs(float(got[0]))


def test_weighted_step_against_the_reference_record(golden):
    """Two TrainingStep(consistency_loss="weighted_l2") iterations against the reference's two iterations with
    NormalizedWeightedMaskedL2Loss (the form that couples the samples): losses, pre-clip gradient norm and pred_1 of each iteration,
    held to the record's fp64 values within 4 x the reference's own fp32 error (>= 1e-6 of max |ref|).
    Measured on an MI355X, iteration 0 / 1 (bound): losses 4.1e-7 / 7.7e-8 (1.5e-6 / 1.2e-6), gradient norm 3.7e-5 / 1.8e-4
    (4.4e-4 / 7.8e-4), pred_1 4.9e-7 / 6.0e-6 (2.7e-6 / 2.5e-5)."""
    g = golden(FIXTURE)
    n, h, w, seed, batch_seed = (int(v) for v in np.array(g["step::shape"]))
    state, model = tp.make_model(seed, positive_depth=True)
    model.train()
    step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-3), h, w, consistency_loss="weighted_l2")
    problems = []
    for i in range(2):
        batch = tp.to_dev(ea.synthetic.make_batch(n, h, w, seed=batch_seed + i, sparse_points=500))
        losses_t, x, tape, pred, grad_pred = step._fused_iteration(batch)
        pred_1 = pred[:n].clone()
        del losses_t, x, tape, pred, grad_pred
        out = step(batch, lr=1.0e-3)          # (the forward above updated the running statistics once more; training mode does not read them)
        torch.cuda.synchronize()
        assert not out["skipped"]
        got = {"losses": np.array([out["loss"], float(out["dcl"]), float(out["sfl"])]), "grad_norm": np.array(float(out["grad_norm"])),
               "pred_1": pred_1.double().cpu().numpy()}
        for name in ("losses", "grad_norm", "pred_1"):
            want64, bound = step_bound(g, i, name)
            err, scale = float(np.abs(got[name] - want64).max()), float(np.abs(want64).max())
            want32 = np.array(g["step::%d::%s_f32" % (i, name)]).astype(np.float64)
            print("weighted_l2 step %d %-9s device against fp64 %.2e of max |ref| (bound %.2e; the reference's fp32 %.2e)" % (
                i, name, err / scale, bound / scale, float(np.abs(want32 - want64).max()) / scale))
            if err > bound:
                problems.append("iteration %d %s: %.3e > %.3e" % (i, name, err / scale, bound / scale))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("storage", ["bf16", "fp16"])
def test_l2_step_under_16bit_storage(storage):
    """TrainingStep(consistency_loss="l2") under bf16_storage / fp16_storage runs through endo_loss_head_forms and stays finite; its
    losses against the fp32 step's on the same weights and batch within tests/test_gpu_bf16.py's own STEP16_BOUNDS (loss, terms, norm)."""
    n, h, w = 1, 64, 96
    b = t16.STEP16_BOUNDS[storage]
    batch = tp.to_dev(ea.synthetic.make_batch(n, h, w, seed=3, sparse_points=300))
    outs = []
    for kw in ({}, {"bf16_storage": storage == "bf16", "fp16_storage": storage == "fp16"}):
        _, model = tp.make_model(7, positive_depth=True)
        model.train()
        step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-3), h, w, consistency_loss="l2", **kw)
        out = step(batch, lr=1.0e-3)
        torch.cuda.synchronize()
        assert not out["skipped"] and np.isfinite(out["loss"]) and bool(torch.isfinite(model.flat_parameters()).all())
        outs.append(out)
    ref, out = outs
    rel = lambda a, c: abs(float(a) - float(c)) / max(abs(float(c)), 1e-12)
    print("%s-storage l2 step: loss rel %.2e, dcl rel %.2e, sfl rel %.2e, gradient norm rel %.2e" % (
        storage, rel(out["loss"], ref["loss"]), rel(out["dcl"], ref["dcl"]), rel(out["sfl"], ref["sfl"]), rel(out["grad_norm"], ref["grad_norm"])))
    assert rel(out["loss"], ref["loss"]) <= b["loss"]
    assert rel(out["dcl"], ref["dcl"]) <= b["terms"] and rel(out["sfl"], ref["sfl"]) <= b["terms"]
    assert rel(out["grad_norm"], ref["grad_norm"]) <= b["norm"]


def test_photometric_term_with_a_chosen_form():
    """photometric_weight > 0 with a non-default form: endo_loss_head_forms writes five losses; dcl is the form's, sfl and photo are
    those of the default step on the same weights (1e-6: the same kernels)."""
    n, h, w = 2, 64, 96
    batch = tp.to_dev(ea.synthetic.make_batch(n, h, w, seed=11, sparse_points=300))
    got = {}
    for form in ("distance", "l1"):
        _, model = tp.make_model(58, positive_depth=True)
        model.train()
        step = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-3), h, w, consistency_loss=form, photometric_weight=0.5)
        got[form] = step.validation_losses(batch).clone()
        plain = ea.train_step.TrainingStep(model, ea.optim.FusedClipSGD(model, lr=1.0e-3), h, w, consistency_loss=form)
        got[form + "-plain"] = plain.validation_losses(batch).clone()
    torch.cuda.synchronize()
    a, b = got["distance"], got["l1"]
    assert a.shape == b.shape == (5,) and float(b[3]) == 0.0 and float(b[4]) > 0
    tp.assert_close(b[2], a[2], SAME_ARITHMETIC, "sfl")
    tp.assert_close(b[4], a[4], SAME_ARITHMETIC, "photo")
    tp.assert_close(b[1], got["l1-plain"][1], SAME_ARITHMETIC, "dcl with and without the photometric term")
    assert abs(float(b[0]) - float(b[1] + b[2] + b[4])) <= 1e-6 * float(b[0]) and abs(float(b[1]) - float(a[1])) > 1e-3 * float(a[1])


def test_distillation_step_passes_the_form_on():
    """DistillationStep(consistency_loss=...) in combined mode: dcl is that of a TrainingStep with the same form on the student."""
    n, h, w = 1, 64, 96
    batch = tp.to_dev(ea.synthetic.make_batch(n, h, w, seed=12, sparse_points=300))
    _, student = tp.make_model(4, positive_depth=True)
    _, teacher = tp.make_model(24, positive_depth=True)
    student.train()
    teacher.eval()
    running0 = {k: v.clone() for k, v in student.state_dict().items() if "running" in k}
    distill = ea.train_step.DistillationStep(student, teacher, ea.optim.FusedClipSGD(student, lr=1.0e-3), h, w, distill_weight=0.5,
                                             sfl_weight=20.0, dcl_weight=0.1, consistency_loss="weighted_l2")
    got = distill.validation_losses(batch).clone()
    student.load_state_dict(running0, strict=False)
    plain = ea.train_step.TrainingStep(student, ea.optim.FusedClipSGD(student, lr=1.0e-3), h, w, consistency_loss="weighted_l2")
    want = plain.validation_losses(batch).clone()
    torch.cuda.synchronize()
    assert got.shape == (5,) and float(got[3]) == 0.0 and float(got[4]) > 0
    tp.assert_close(got[1:3], want[1:3], SAME_ARITHMETIC, "dcl and sfl of the combined distillation step")
    assert distill.display_panels().dtype == torch.uint8


@pytest.mark.parametrize("form", cr.FORMS)
def test_workspace_contract(form):
    """Both new entries on NaN-poisoned workspaces and outputs (tests/guarded_alloc.py) against zero-filled ones: the same results
    within the atomics' order, and every guard byte intact -- no write lands outside a buffer."""
    n, h, w = 3, 40, 72
    batch, p1, p2, _ = tp.geometry_inputs(n, h, w, 91)
    batch = cr.scale_translations(batch, (0.5, 1.0, 3.0))
    db = tp.to_dev(batch)
    p1, p2 = p1.to(tp.dev()), p2.to(tp.dev())
    results = {}
    for fill in ("poison", "zeros"):
        saved = dict(ea.losses._consistency_ws)
        ea.losses._consistency_ws.clear()          # the cached workspace is allocated inside the context: guarded, and filled with `fill`
        try:
            with guarded(device="cuda", fill=fill) as alloc:
                head = call_head(form, db, p1, p2)
                alone = consistency(form, db, p1, p2, dcl_weight=0.7)
                torch.cuda.synchronize()
                alloc.check()
                results[fill] = [t.clone() for t in head + tuple(alone)]
        finally:
            ea.losses._consistency_ws.clear()
            ea.losses._consistency_ws.update(saved)
    print("%s on poisoned against zero-filled buffers: %s" % (form, ["%.1e" % tp.rel_err(a, b) for a, b in zip(results["poison"], results["zeros"])]))
    for got, want, tol, what in zip(results["poison"], results["zeros"], (SAME_ARITHMETIC,) * 6,
                                    ("head losses", "head grad 1", "head grad 2", "loss", "grad 1", "grad 2")):
        assert bool(torch.isfinite(got).all()), what
        tp.assert_close(got, want, tol, "%s: %s on poisoned buffers against zero-filled ones" % (form, what))
