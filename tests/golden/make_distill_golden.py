"""Writes tests/golden/distill.npz: inputs and the outputs of the reference's own teacher-student code -- utils.learn_from_teacher
(utils.py:1462-1482) over losses.ScaleInvariantLoss (losses.py:17-32), and utils.calculate_outlier_robust_validation_loss
(utils.py:1734-1744) -- evaluated on the CPU by the reference's unmodified functions under autograd.

    python tests/golden/make_distill_golden.py <directory of the reference checkout>

Needs the reference, so it is run where that exists and not by the test suite; only inputs and recorded outputs are written, no
reference source is stored.  ``.cuda()`` and the missing imports are stubbed as make_golden.py does (its import_reference).  Network
weights come from oracle.network.synthetic_state seeds, not from stored tensors.

Records, keys ``<record>::<name>``:

  head (N = 3, 24 x 40): distill_restate.head_inputs(3, 24, 40, HEAD_SEED) -- predictions and goals of both signs, six exact zeros in
      each prediction map on boundary pixels, a {0, 1} boundary at about 60 %; value and d / d pred of
      0.5 * (SIL(|p1|, |g1|, b) + SIL(|p2|, |g2|, b)) by the reference's class.  All finite; the gradient at the zeros is 0.
  edge (N = 2, 24 x 40): the same with sample 1's boundary empty; the value only, NaN.
  step (2 x 64 x 96): teacher (eval) from TEACHER_SEED, student (train) from STUDENT_SEED, both keep_depth_positive(perturb_affine(.));
      two iterations of learn_from_teacher on the masked colours of synthetic.make_batch(seed = BATCH_SEED + i) + clip_grad_norm_(10) +
      SGD(1e-3, 0.9).  Per iteration: loss, pre-clip gradient norm, the student's pred_1, parameter norms and sums after the update,
      the norm of the whole parameter update, the teacher's output checksum (sum and sum of squares of both goal maps, fp64).
      The seeds are chosen so that both networks' outputs stay above 0.1 on the boundary: the loss differentiates log |p|, and with
      most seeds of random weights the student's output crosses zero somewhere, where the reference's own fp32 gradient norm is
      off its fp64 value by 0.3 % to 4 % at iteration 0 and by 24 % to 600 % at iteration 1 (five seed triples tried) -- no record
      to hold anything to.  With these seeds the reference's fp32 and fp64 runs agree to 1e-6 in loss and gradient norm (asserted
      below for iteration 0 and 1), and iteration 0 clips (norm 10.4) while iteration 1 does not (8.0).
  combined: the same student and teacher, one iteration of train.py's body (weights 20 / 0.1) plus 0.5 x learn_from_teacher's loss:
      [total, dcl, sfl, distill], gradient norm, parameter norms.
  robust: calculate_outlier_robust_validation_loss on distill_restate.robust_inputs()."""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (import_reference's stubs, load_reference_net, the deterministic weights)
import distill_restate as dr  # noqa: E402

HEAD_SEED, EDGE_SEED = 20241101, 20241102
TEACHER_SEED, STUDENT_SEED, BATCH_SEED = 24, 4, 100
N, H, W = 2, 64, 96
F32 = np.float32


def tensors(x, *keys):
    return [torch.from_numpy(x[k]) for k in keys]


def head_records(ref, out):
    sil = ref["losses"].ScaleInvariantLoss(epsilon=1.0e-8)
    x = dr.head_inputs(3, 24, 40, HEAD_SEED)
    p1, p2, g1, g2, b = tensors(x, "pred_1", "pred_2", "goal_1", "goal_2", "boundaries")
    p1.requires_grad_(True)
    p2.requires_grad_(True)
    value = 0.5 * (sil([torch.abs(p1), torch.abs(g1), b]) + sil([torch.abs(p2), torch.abs(g2), b]))
    d1, d2 = torch.autograd.grad(value, (p1, p2))
    on = x["boundaries"] > 0
    for key, d in (("pred_1", d1), ("pred_2", d2)):
        zero = (x[key] == 0) & on
        assert int(zero.sum()) == 6 and float(d.numpy()[zero].__abs__().max()) == 0.0
        assert (x[key] < 0).any() and (x[key] > 0).any()
        assert bool(torch.isfinite(d).all()) and float(d.abs().max()) > 0
    assert (x["goal_1"] < 0).any() and (x["goal_2"] < 0).any() and 0.5 < x["boundaries"].mean() < 0.7
    assert set(np.unique(x["boundaries"]).tolist()) == {0.0, 1.0} and bool(torch.isfinite(value))
    for key, v in x.items():
        out["head::" + key] = v
    out["head::loss"] = value.detach().numpy().astype(F32)
    out["head::grad_pred_1"] = d1.numpy().astype(F32)
    out["head::grad_pred_2"] = d2.numpy().astype(F32)
    e = dr.head_inputs(2, 24, 40, EDGE_SEED, empty_sample=1)
    assert e["boundaries"][1].sum() == 0 and e["boundaries"][0].sum() > 0
    with torch.no_grad():
        p1, p2, g1, g2, b = tensors(e, "pred_1", "pred_2", "goal_1", "goal_2", "boundaries")
        value = 0.5 * (sil([torch.abs(p1), torch.abs(g1), b]) + sil([torch.abs(p2), torch.abs(g2), b]))
    assert bool(torch.isnan(value))
    out["edge::loss"] = value.numpy().astype(F32)


def networks(ref):
    make = lambda seed: mg.load_reference_net(ref, mg.onet.keep_depth_positive(mg.onet.perturb_affine(mg.onet.synthetic_state(seed), seed + 1)))
    return make(TEACHER_SEED).eval(), make(STUDENT_SEED).train()


def flat(net):
    return torch.cat([p.detach().double().reshape(-1) for p in net.parameters()])


def summary(out, tag, net, before, gnorm):
    out[tag + "grad_norm"] = mg.t2n(gnorm)
    out[tag + "param_norms"] = np.array([float(p.double().norm()) for p in net.parameters()])
    out[tag + "param_sums"] = np.array([float(p.double().sum()) for p in net.parameters()])
    out[tag + "update_norm"] = np.float64((flat(net) - before).norm())


def iterate(ref, teacher, student, opt, i, dtype=torch.float32):
    """One iteration of the reference's teacher-student loop body; returns (loss, pre-clip gradient norm, the four depth maps)."""
    sil = ref["losses"].ScaleInvariantLoss(epsilon=1.0e-8)
    sil.epsilon = sil.epsilon.to(dtype)
    batch = mg.synthetic.make_batch(N, H, W, seed=BATCH_SEED + i, sparse_points=500)
    b = batch["boundaries"].to(dtype)
    loss, p1, p2, g1, g2 = ref["utils"].learn_from_teacher(b, b * batch["colors_1"].to(dtype), b * batch["colors_2"].to(dtype), teacher,
                                                           student, sil)
    opt.zero_grad()
    loss.backward()
    gnorm = torch.nn.utils.clip_grad_norm_(student.parameters(), 10.0)
    opt.step()
    for t in (p1, p2, g1, g2):
        assert float(t[b > 0].min()) > 0.1          # log |.| and 1 / |.| stay well conditioned (the module docstring)
    return loss, gnorm, (p1, p2, g1, g2)


def step_record(ref, out):
    teacher, student = networks(ref)
    opt = torch.optim.SGD(student.parameters(), lr=1.0e-3, momentum=0.9)
    teacher_before = flat(teacher)
    teacher64, student64 = (m.double() for m in networks(ref))          # the same two iterations in fp64: the reference's own error
    opt64 = torch.optim.SGD(student64.parameters(), lr=1.0e-3, momentum=0.9)
    for i in range(2):
        before = flat(student)
        loss, gnorm, (p1, p2, g1, g2) = iterate(ref, teacher, student, opt, i)
        loss64, gnorm64, _ = iterate(ref, teacher64, student64, opt64, i, torch.float64)
        assert abs(float(loss) - float(loss64)) <= 1e-5 * float(loss64) and abs(float(gnorm) - float(gnorm64)) <= 1e-5 * float(gnorm64)
        tag = "step::%d::" % i
        out[tag + "loss"] = mg.t2n(loss)
        out[tag + "pred_1"] = mg.t2n(p1).astype(F32)
        both = torch.cat([g1, g2]).detach().double()
        out[tag + "teacher_checksum"] = np.array([float(both.sum()), float((both * both).sum())])
        summary(out, tag, student, before, gnorm)
        assert bool(torch.isfinite(loss)) and float(gnorm) > 0
    assert bool(torch.equal(flat(teacher), teacher_before))
    out["step::shape"] = np.array([N, H, W, TEACHER_SEED, STUDENT_SEED, BATCH_SEED])


def combined_record(ref, out):
    teacher, student = networks(ref)
    sil = ref["losses"].ScaleInvariantLoss(epsilon=1.0e-8)
    scaling = ref["models"].DepthScalingLayer(epsilon=1.0e-8)
    flow_layer = ref["models"].FlowfromDepthLayer()
    warp_layer = ref["models"].DepthWarpingLayer(epsilon=1.0e-8)
    sfl_fn = ref["losses"].SparseMaskedL1Loss()
    dcl_fn = ref["losses"].NormalizedDistanceLoss(height=H, width=W)
    opt = torch.optim.SGD(student.parameters(), lr=1.0e-3, momentum=0.9)
    batch = mg.synthetic.make_batch(N, H, W, seed=BATCH_SEED, sparse_points=500)
    b = batch["boundaries"]
    before = flat(student)
    term, p1, p2, _, _ = ref["utils"].learn_from_teacher(b, b * batch["colors_1"], b * batch["colors_2"], teacher, student, sil)
    distill = 0.5 * term
    s1, _ = scaling([p1, batch["sparse_depths_1"], batch["sparse_depth_masks_1"]])
    s2, _ = scaling([p2, batch["sparse_depths_2"], batch["sparse_depth_masks_2"]])
    f1 = flow_layer([s1, b, batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"], batch["intrinsics"]]) * b
    f2 = flow_layer([s2, b, batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"], batch["intrinsics"]]) * b
    sfl = 20.0 * 0.5 * (sfl_fn([batch["sparse_flows_1"] * b, f1, batch["sparse_flow_masks_1"] * b]) +
                        sfl_fn([batch["sparse_flows_2"] * b, f2, batch["sparse_flow_masks_2"] * b]))
    w21, i1 = warp_layer([s1, s2, b, batch["translations_1_wrt_2"], batch["rotations_1_wrt_2"], batch["intrinsics"]])
    w12, i2 = warp_layer([s2, s1, b, batch["translations_2_wrt_1"], batch["rotations_2_wrt_1"], batch["intrinsics"]])
    dcl = 0.1 * 0.5 * (dcl_fn([s1, w21, i1, batch["intrinsics"]]) + dcl_fn([s2, w12, i2, batch["intrinsics"]]))
    loss = dcl + sfl + distill
    opt.zero_grad()
    loss.backward()
    gnorm = torch.nn.utils.clip_grad_norm_(student.parameters(), 10.0)
    opt.step()
    out["combined::losses"] = np.array([float(loss), float(dcl), float(sfl), float(distill)], dtype=F32)
    out["combined::weights"] = np.array([20.0, 0.1, 0.5], dtype=F32)
    summary(out, "combined::", student, before, gnorm)
    assert bool(torch.isfinite(loss)) and float(dcl) > 0 and float(sfl) > 0 and float(distill) > 0


def robust_record(ref, out):
    fn = ref["utils"].calculate_outlier_robust_validation_loss
    values = [float(fn(a, b)) for a, b in dr.robust_inputs()]
    assert values[1] == -1.0 and values[2] == 1.0 and values[0] not in (0.0, -1.0, 1.0)
    out["robust::values"] = np.array(values, dtype=np.float64)


def main(reference):
    mg.REF = reference
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = mg.import_reference()
    assert os.path.dirname(os.path.abspath(ref["utils"].__file__)) == os.path.abspath(reference)
    out = {}
    head_records(ref, out)
    robust_record(ref, out)
    step_record(ref, out)
    combined_record(ref, out)
    path = os.path.join(HERE, "distill.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 200 * 1000, os.path.getsize(path)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))
    print("  head %s  edge %s  robust %s" % (out["head::loss"], out["edge::loss"], out["robust::values"]))
    for i in range(2):
        print("  step %d: loss %s  grad norm %s  update norm %s" % (i, out["step::%d::loss" % i], out["step::%d::grad_norm" % i],
                                                                     out["step::%d::update_norm" % i]))
    print("  combined: %s  grad norm %s" % (out["combined::losses"], out["combined::grad_norm"]))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "utils.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
