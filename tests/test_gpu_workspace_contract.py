"""The workspace contract of the C ABI (include/endo_hip.h, "Workspace contract") on the device:

  1. a call writes nothing outside the buffers it was given, sized as its ``endo_*_floats`` / ``endo_*_bytes`` query returned;
  2. a call does not depend on what a scratch or output buffer held on entry.

Every case runs inside tests/guarded_alloc.py's context: each ``torch.empty`` / ``torch.empty_like`` of the product code gets 64 KiB of
guard bytes on either side and an interior of 0xFF bytes (NaN in every float format, -1 / 255 in the integer ones), and every cached
workspace -- ``model._gradws``, ``TrainingStep._head_ws``, ``losses._consistency_ws``, the JPEG decoder's slots -- is poisoned again before
every call that uses it.  Two kinds of case, both ending with every guard byte intact:

  (a) the suite's own oracle comparisons, called as they are (their assertions are the project's, unchanged): fp64 oracle on the pass's
      pattern, restatement bit-identity, goldens -- now on poisoned buffers;
  (b) twin runs where no oracle is affordable: one TrainingStep iteration on poisoned buffers against the same iteration on zero-filled
      ones, plus the backward pass a second time on re-poisoned workspaces, held to the bounds test_clean_step_after_a_skipped_step
      states for "the same step twice, atomics in another order" -- at the benchmark grids, at portrait grids (h > w: no other test
      has one), at the shapes that come closest to the fixed scratch bounds of endo_net_create_grouped, and with 3 and 4 sample groups.

Nothing here writes out of bounds or provokes a fault: a violated guard is an assertion failure that names the allocation site, the
side and the offsets (GuardViolation), to be investigated from that report."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_augment as t_aug
import test_gpu_bf16 as t_16
import test_gpu_evaluate as t_eval
import test_gpu_parity as tp
import test_plan_coverage as cov
import test_gpu_scatter as t_scat
import test_gpu_validation as t_val
import test_reader as t_read
from device_pattern import pattern_from_tape
from guarded_alloc import guarded
from oracle import network as onet
from test_gpu_augment import batch3, batch16, fixture  # noqa: F401 -- fixtures (batch16 asks for `fixture` by that name)
from test_gpu_augment import sequence as augment_sequence  # noqa: F401 -- fixture
from test_reader import golden as reader_golden, sequence as reader_sequence  # noqa: F401 -- fixtures

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
models = importlib.import_module("endoscopydepthestimation-pytorch_amd.models")
losses = importlib.import_module("endoscopydepthestimation-pytorch_amd.losses")
train_step = importlib.import_module("endoscopydepthestimation-pytorch_amd.train_step")
reader = importlib.import_module("endoscopydepthestimation-pytorch_amd.reader")

OPT_FINAL_VIRTUAL, OPT_TD_PERSIST = 8, 9          # include/endo_hip.h ENDO_OPT_*; the first eight ids: test_gpu_parity.OPT_*


# ---------------------------------------------------------------------------------------------
# the context every case runs in
# ---------------------------------------------------------------------------------------------
class _PoisoningDict(dict):
    """losses._consistency_ws for the duration of a case: a cached workspace is poisoned again every time it is looked up."""

    def __init__(self, alloc):
        dict.__init__(self)
        self.alloc = alloc

    def get(self, key, default=None):
        ws = dict.get(self, key, default)
        self.alloc.repoison(ws)
        return ws


class contract(object):
    """``with contract() as g:`` = ``guarded("cuda")`` plus: caches of workspaces made before the block are set aside (so that the block
    allocates its own, guarded), and every cached workspace is refilled with the context's fill before each call that uses it -- the
    documented meaning of all of them is scratch (include/endo_hip.h).  Only workspaces the context handed out are refilled: a test that
    installs a buffer of its own (test_16bit_backward_partial_buffer_shapes' guard word) keeps it.  One exception, by name: the loss
    head's workspace is refilled before endo_loss_head only -- between that call and TrainingStep.display_panels it is STATE (the planes
    endo_loss_head_planes describes; include/endo_hip.h says so)."""

    def __init__(self, fill="poison"):
        self.alloc = guarded(device="cuda", fill=fill)
        self.saved = None

    def _owned(self, what):
        items = what.values() if isinstance(what, dict) else what
        return [t for t in items if t is not None and self.alloc.block_of(t) is not None]

    def __enter__(self):
        alloc, owned = self.alloc, self._owned
        net, step_cls, dec = models.FCDenseNet, train_step.TrainingStep, reader.FrameDecoder
        self.saved = (net._run_backward, net._run_backward16, step_cls._fused_iteration, dec._slot, losses._consistency_ws, reader._default_decoder)
        run_backward, run_backward16, fused_iteration, slot_of = self.saved[:4]

        def _run_backward(model, *args, **kw):
            alloc.repoison(owned(model._gradws))
            return run_backward(model, *args, **kw)

        def _run_backward16(model, *args, **kw):
            alloc.repoison(owned(model._gradws))
            return run_backward16(model, *args, **kw)

        def _fused_iteration(step, batch):
            alloc.repoison(owned([step._head_ws]))
            return fused_iteration(step, batch)

        def _slot(decoder, nbytes):
            slot = slot_of(decoder, nbytes)          # (has waited for the slot's previous use)
            alloc.repoison(owned([slot["workspace"]]))
            return slot

        net._run_backward, net._run_backward16, step_cls._fused_iteration, dec._slot = _run_backward, _run_backward16, _fused_iteration, _slot
        losses._consistency_ws = _PoisoningDict(alloc)
        reader._default_decoder = None
        return alloc.__enter__()

    def __exit__(self, *exc):
        net, step_cls, dec = models.FCDenseNet, train_step.TrainingStep, reader.FrameDecoder
        net._run_backward, net._run_backward16, step_cls._fused_iteration, dec._slot, losses._consistency_ws, reader._default_decoder = self.saved
        self.saved = None
        torch.cuda.synchronize()
        return self.alloc.__exit__(*exc)


def test_the_context_poisons_and_restores():
    """The harness on the device: alignment, poison, the hooks' restoration, and that product allocations are seen with their site."""
    real = (torch.empty, torch.empty_like, models.FCDenseNet._run_backward, losses._consistency_ws)
    with contract() as g:
        t = torch.empty((3, 5), dtype=torch.float32, device=tp.dev())
        assert t.data_ptr() % 512 == 0 and bool(torch.isnan(t).all()) and g.block_of(t).base.data_ptr() % 512 == 0
        assert bool((torch.empty(4, dtype=torch.int32, device="cuda") == -1).all())
        assert g.block_of(torch.empty(4)) is None          # host memory is not this context's
        _, model = tp.make_model(52)
        x = torch.zeros((1, 3, 32, 32), device=tp.dev())
        model.train()
        model(x).sum().backward()
        sites = [b.site for b in g.blocks]
        assert any(s.startswith("endoscopydepthestimation-pytorch_amd/models.py:") for s in sites), sites
        assert all(g.block_of(ws) is not None for ws in model._gradws.values()) and len(model._gradws) == 1
    now = (torch.empty, torch.empty_like, models.FCDenseNet._run_backward, losses._consistency_ws)
    assert all(a is b for a, b in zip(now, real))


# ---------------------------------------------------------------------------------------------
# (a) the suite's oracle comparisons on poisoned buffers
# ---------------------------------------------------------------------------------------------
def _case(_module, _test, _fixtures=(), ident=None, **kw):
    """One case: the test function `_test` of `_module`, called with the keyword arguments `kw` and the named fixtures.  A fixture is given by
    the name the body asks for, or as (argument, the name the fixture is imported under in this module)."""
    if ident is None:
        ident = ",".join("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in kw.values())
    return pytest.param(_module, _test, tuple(_fixtures), kw, id="%s[%s]" % (_test, ident) if ident else _test)


FUSIONS = [(forced, extra, "%s-%s" % (fname, ename)) for forced, fname in ((False, "default-forms"), (True, "winograd-forms"))
           for extra, ename in (({}, "fp32"), ({4: 1}, "bf16-operands"), ({2: 0}, "dgrad-vec-0"), ({2: 1}, "dgrad-vec-1"))]
CONV16_IDS = ["%dx%dx%d_cin%d_cout%d_ks%d%s" % (c[0], c[1], c[2], c[5], c[6], c[9], "_ups" if c[10] else "") for c in t_16.CASES]

ORACLE_CASES = (
    # geometry and losses
    [_case(tp, nm, shape=s) for nm in ("test_depth_scaling", "test_flow_from_depth", "test_depth_warping") for s in ((2, 37, 53), (1, 256, 320))] +
    [_case(tp, "test_warp_edge_cases"), _case(tp, "test_warp_tiles_agree_and_fall_back"), _case(tp, "test_warp_consistency_call")] +
    [_case(tp, "test_losses", shape=s) for s in ((2, 16, 20), (1, 256, 320))] +
    [_case(tp, "test_depth_warping_tiles_512x640", tile=t) for t in tp.WARP_TILES] +
    [_case(tp, "test_geometry_and_losses_512x640")] +
    [_case(tp, "test_fused_loss_head_matches_modules", shape=s) for s in ((3, 32, 64), (1, 256, 320))] +
    # fp32 network
    [_case(tp, "test_network_backward_kernel_forms", shape=s, which=wh) for wh in ("winograd", "winograd4", "direct") for s in ((2, 64, 96), (1, 64, 128))] +
    [_case(tp, "test_network_backward_kernel_forms", shape=(2, 128, 256), which="nsplit"), _case(tp, "test_network_backward_eval_mode"),
     _case(tp, "test_forward_pair_is_two_calls", shape=(3, 32, 64))] +
    [_case(tp, "test_final_conv_fusions_are_transparent", forced=f, extra=e, ident=i) for f, e, i in FUSIONS] +
    [_case(tp, nm, shape=(3, 96, 160)) for nm in ("test_persistent_new_map_passes_match_the_per_tile_blocks", "test_persistent_base_pass_matches_the_per_tile_kernel",
                                                  "test_persistent_transition_down_dgrad_matches_the_per_tile_kernel",
                                                  "test_persistent_transition_down_forward_matches_the_per_tile_kernel")] +
    [_case(tp, "test_wgrad_overlap_is_transparent", shape=(2, 64, 96)), _case(tp, "test_bf16_operand_mode_on_pattern", shape=(2, 64, 96)),
     _case(tp, "test_train_step_vs_oracle"), _case(tp, "test_optimizer_step")] +
    # 16-bit storage
    [_case(t_16, "test_bf16_conv_against_fp64", case=c, blk=b, ident="%s-%s" % (i, "blk32" if b else "nhwc")) for c, i in zip(t_16.CASES, CONV16_IDS) for b in (0, 32)] +
    [_case(t_16, "test_bf16_storage_backward", shape=(2, 64, 96), mode="train", storage=s) for s in ("bf16", "fp16")] +
    [_case(t_16, "test_16bit_training_step_against_oracle", storage=s) for s in ("bf16", "fp16")] +
    [_case(t_16, "test_16bit_backward_partial_buffer_shapes", shape=sh, storage=s) for sh, s in (((1, 256, 320), "bf16"), ((4, 128, 160), "fp16"))] +
    # display, validation, evaluate
    [_case(t_val, "test_display_matches_restatement", ident="%dx%dx%d" % s, n=s[0], h=s[1], w=s[2]) for s in ((9, 64, 96), (8, 256, 320))] +
    [_case(t_val, "test_validation_accumulate_matches_recurrence"), _case(t_val, "test_validate_over_batches")] +
    [_case(t_eval, "test_outputs_match_restatement", ident="%d-%dx%d-%s" % (n, s[0], s[1], "hsv" if hsv else "rgb"), n=n, size=s, is_hsv=hsv)
     for n, s in ((3, (64, 96)), (8, (256, 320))) for hsv in (False, True)] +
    [_case(t_eval, "test_points_match_point_cloud_from_depth")] +
    # augment (one size each; the noise statistics stay where they are), reader, scatter
    [_case(t_aug, "test_jpeg_compression_is_libjpeg_turbo", ("fixture",), name=nm) for nm in ("256x320", "37x53")] +
    [_case(t_aug, "test_box_and_median_blur_match_restatements", ("batch16", "batch3")), _case(t_aug, "test_motion_blur_matches_restatement", ("batch16", "batch3")),
     _case(t_aug, "test_brightness_contrast_gamma_matches_restatement", ("batch16",)), _case(t_aug, "test_shift_hsv_matches_restatement", ("batch16",)),
     _case(t_aug, "test_training_augmentation_is_the_composition_of_its_ops", ("batch16",)), _case(t_aug, "test_forced_expensive_plan_runs"),
     _case(t_aug, "test_training_batches_with_the_transform", (("sequence", "augment_sequence"),))] +
    [_case(t_read, "test_device_decode_matches_oracle_on_generated_files", layout=l, ident=l[0]) for l in t_read.LAYOUTS] +
    [_case(t_read, "test_hsv_full_on_device_matches_oracle"),
     _case(t_read, "test_point_brightness_and_clean_points_on_device", (("golden", "reader_golden"), ("sequence", "reader_sequence")))] +
    [_case(t_scat, "test_scatter_golden_batched", ("pkg", "golden")), _case(t_scat, "test_scatter_dropin_signature", ("pkg", "golden"))] +
    [_case(t_scat, "test_scatter_vs_oracle_collisions", ("pkg",), ident="%d-%dx%dx%d" % (c[0], c[3], c[1], c[2]), n_points=c[0], height=c[1], width=c[2], batch=c[3], use_clean=c[4])
     for c in ((6000, 32, 40, 3, True), (500, 256, 320, 2, False), (1, 8, 8, 1, True))] +
    [_case(t_scat, "test_scatter_empty_cloud_and_multiplier", ("pkg",)), _case(t_scat, "test_point_cloud_golden_and_oracle", ("pkg", "golden")),
     _case(t_scat, "test_training_batch_on_device", ("pkg", "golden"))]
)


@pytest.mark.parametrize("module,name,fixtures,kw", ORACLE_CASES)
def test_oracle_case_on_poisoned_buffers(request, module, name, fixtures, kw):
    """The named test of the suite, called as it is inside the poisoning, guarded context: its own assertions must hold on buffers that
    entered every call as NaN, and no guard byte may have changed when it returns."""
    args = dict(kw)
    for fx in fixtures:          # a fixture by the name the body asks for, or (argument, the name it is imported under here)
        arg, source = fx if isinstance(fx, tuple) else (fx, fx)
        args[arg] = request.getfixturevalue(source)
    with contract() as g:
        getattr(module, name)(**args)
        torch.cuda.synchronize()
        g.check()


# ---------------------------------------------------------------------------------------------
# (b) twin runs: poisoned against zero-filled buffers
# ---------------------------------------------------------------------------------------------
FORMS = {
    "default": {},
    "winograd": {tp.OPT_WINO_MIN_TILES: 1, tp.OPT_WINO_FWD: 1},
    "winograd4": {tp.OPT_WINO_MIN_TILES: 1, tp.OPT_WINO_FWD: 5},
    # every kernel form that has a switch, off: the plain kernels
    "direct": {tp.OPT_WINO_FWD: 0, tp.OPT_WINO_DGRAD: 0, tp.OPT_DGRAD_VEC: 0, tp.OPT_WGRAD_F34: 0, OPT_FINAL_VIRTUAL: 0, OPT_TD_PERSIST: 0},
}


def _finite(what, t):
    t = torch.as_tensor(t)
    bad = int((~torch.isfinite(t)).sum())
    assert bad == 0, "%s: %d of %d values are not finite" % (what, bad, t.numel())


def run_iteration(fill, shape, form, storage, seed=58):
    """One TrainingStep iteration (grouped pair forward, fused loss head, backward, clip + SGD) on a fresh model inside contract(fill), with
    the backward pass run a second time from the same tape on re-poisoned workspaces.  Everything read back, as host tensors."""
    n, h, w = shape
    kw = {"bf16": {"bf16_storage": True}, "fp16": {"fp16_storage": True}}.get(storage, {})
    batch = ea.synthetic.make_batch(n, h, w, seed=73, sparse_points=min(300, h * w // 6))
    kept = {}
    with contract(fill) as g:
        with tp.kernel_options(FORMS[form]):
            _, model = tp.make_model(seed, positive_depth=True)
        model.train()
        opt = ea.optim.FusedClipSGD(model, lr=1.0e-3)
        step = ea.train_step.TrainingStep(model, opt, h, w, **kw)
        inner, backward = step._fused_iteration, step._fused_backward

        def keep(b):          # what the step hands from its forward half to its backward half
            kept["out"] = inner(b)
            return kept["out"]

        def backward_twice(x, tape, grad_pred):
            # the backward pass, and -- before the optimizer changes the parameters -- the same pass again: same tape, same d loss / d prediction,
            # gradient accumulator cleared, workspaces poisoned again (by the context's hook; said here once more for the reader)
            backward(x, tape, grad_pred)
            kept["grads_first"] = model.flat_gradients().clone()
            model.flat_gradients().zero_()
            g.repoison([ws for ws in model._gradws.values() if g.block_of(ws) is not None])
            backward(x, tape, grad_pred)
            kept["grads_again"] = model.flat_gradients().clone()

        step._fused_iteration, step._fused_backward = keep, backward_twice
        out = step(tp.to_dev(batch), lr=1.0e-3)
        torch.cuda.synchronize()
        _, x, tape, pred, grad_pred = kept["out"]
        res = {"loss": float(out["loss"]), "dcl": float(out["dcl"]), "sfl": float(out["sfl"]), "grad_norm": float(out["grad_norm"]),
               "skipped": bool(out["skipped"]), "depth": pred.cpu(), "grad_pred": grad_pred.cpu(), "grads": model.flat_gradients().cpu(),
               "grads_first": kept["grads_first"].cpu(), "grads_again": kept["grads_again"].cpu(),
               "params": model.flat_parameters().detach().cpu(),
               "running": {k: v.cpu() for k, v in model.state_dict().items() if "running" in k}}
    return res


def assert_all_finite(res, what):
    assert not res["skipped"], "%s: the step's guard skipped the update (loss %r)" % (what, res["loss"])
    for key in ("loss", "dcl", "sfl", "grad_norm", "depth", "grad_pred", "grads", "grads_first", "grads_again", "params"):
        _finite("%s: %s" % (what, key), res[key])
    for key, val in res["running"].items():
        _finite("%s: %s" % (what, key), val)


def assert_twins_agree(a, b, storage, what):
    """The bounds test_clean_step_after_a_skipped_step states for the same step run twice (atomics in another order), not tuned here."""
    tol = 5e-5 if storage == "fp32" else 2e-3
    figures = {"loss": abs(a["loss"] - b["loss"]) / abs(b["loss"]), "grad_norm": abs(a["grad_norm"] - b["grad_norm"]) / b["grad_norm"],
               "grads": tp.rel_err(a["grads"], b["grads"]), "grads_again": tp.rel_err(a["grads_again"], a["grads_first"]),
               "params": tp.rel_err(a["params"], b["params"]),
               "running": max(tp.rel_err(a["running"][k], b["running"][k]) for k in b["running"])}
    print("%s: poisoned vs zero-filled twin: %s" % (what, "  ".join("%s %.2e" % kv for kv in figures.items())))
    assert figures["loss"] <= 1e-6, (what, a["loss"], b["loss"])
    assert figures["grad_norm"] <= tol, (what, a["grad_norm"], b["grad_norm"])
    assert figures["grads"] <= 20 * tol, (what, "gradients", figures["grads"])
    assert figures["grads_again"] <= 20 * tol, (what, "gradients of the second backward pass over the same tape", figures["grads_again"])
    assert figures["params"] <= (1e-6 if storage == "fp32" else 1e-5), (what, "parameters", figures["params"])
    assert figures["running"] <= 1e-6, (what, "running statistics", figures["running"])


def twin_run(shape, form, storage):
    what = "%s %s %s" % ("x".join(str(i) for i in shape), form, storage)
    poisoned = run_iteration("poison", shape, form, storage)
    assert_all_finite(poisoned, what + " (poisoned)")
    zeroed = run_iteration("zeros", shape, form, storage)
    assert_all_finite(zeroed, what + " (zero-filled)")
    assert_twins_agree(poisoned, zeroed, storage, what)


# The benchmark grids in their default kernel forms, through the grouped pair forward (groups = 2).  These are also the inputs that come
# closest to three of the fixed scratch bounds of endo_net_create_grouped (csrc/net.hip), by the launch code's own arithmetic:
#   * 4 * kF34ScratchFloats (F(3x3, 4x4) weight-gradient partials, four slices): a launch uses groups * 9 * 8 * spb * 256 floats of its slice with
#     groups * wpg <= 256 waves per XCD; 16 x 256 x 320 gives every group more row segments than waves, so cin = 60 ... 64 (4 groups x 64 waves)
#     fills its slice to 256 / 256 = 100 %, cin = 48 (3 x 85) to 99.6 %;
#   * kSpScratchFloats (sub-pixel transition-up weight gradient): blocks <= 384; at 16 x 128 x 160 low-resolution pixels 10 240 chunks -> 27 per block
#     -> 380 blocks = 99 % (the 6 x 128 x 160 case below reaches 384 = 100 %);
#   * kBiasPartChannels * n * groups * 32 (bias-gradient partials): a launch takes count * n * groups * bx floats, bx = min(32, plane / 4096): 32 only at
#     level 0 of 512 x 640, and the network has 1 776 of the 2 048 channels, so no input passes 86.7 %; prep_dy checks every launch against the size and
#     returns ENDO_E_UNSUPPORTED rather than write past it.
BENCH_TWINS = [((8, 256, 320), "fp32"), ((4, 512, 640), "fp32"), ((8, 256, 320), "bf16"), ((8, 256, 320), "fp16")]


@pytest.mark.parametrize("shape,storage", BENCH_TWINS, ids=["%dx%dx%d-%s" % (s + (st,)) for s, st in BENCH_TWINS])
def test_twin_run_at_the_benchmark_grids(shape, storage):
    twin_run(shape, "default", storage)


# Portrait grids (h > w): the shape predicates of the kernels are asymmetric in h and w (w % 32, h % 8, h % 16, 32 x 8 and 64 x 16 tiles) and
# every other shape in the suite has w >= h.
PORTRAIT_TWINS = ([((2, 160, 96), f, "fp32") for f in ("default", "winograd", "winograd4", "direct")] +
                  [(s, f, "fp32") for s in ((1, 160, 128), (2, 320, 256)) for f in ("default", "winograd", "winograd4")] +
                  [((2, 160, 96), "default", "bf16"), ((2, 160, 96), "default", "fp16")])


@pytest.mark.parametrize("shape,form,storage", PORTRAIT_TWINS, ids=["%dx%dx%d-%s-%s" % (s + (f, st)) for s, f, st in PORTRAIT_TWINS])
def test_twin_run_at_portrait_grids(shape, form, storage):
    twin_run(shape, form, storage)


PORTRAIT_FORMS = {          # what each form of test_portrait_network_backward_on_pattern runs at 2 x 160 x 96 (tp.assert_plan: takes, lacks)
    "default": ([("dense_fwd", "SplitK", 1), ("dense_wgrad", "F34", 0), ("dense_wgrad", "F34", 1), ("dense_wgrad", "Taps", 2), ("base_pass", "Block8", 0), ("newmap", "Persistent", 0),
                 ("td_dgrad", "Persistent", 0), ("td_fwd", "Persistent", 0), ("tu_dgrad", "Subpix16x4", 0), ("first_wgrad", "F34Prep", 0)], [("dense_fwd", "Wino4", None)]),
    "winograd": ([("dense_fwd", "Wino2_32x16", l) for l in (0, 1, 2, 3)] + [("base_pass", "Wino3Persistent", 0), ("base_pass", "Block8", 1), ("dense_wgrad", "F34", 1)], [("dense_fwd", "Wino4", None)]),
    "winograd4": ([("dense_fwd", "Wino4", l) for l in (0, 1, 2, 3)] + [("base_pass", "Wino3Persistent", 0), ("fuse_final", 1, -1)], [("dense_fwd", "Wino2_32x16", None)]),
    "direct": ([("dense_fwd", "SplitK", 1), ("dense_wgrad", "Taps", 0), ("base_pass", "Block8", 0), ("newmap", "Dword", 0), ("td_dgrad", "Dma", 0), ("td_fwd", "PerTile", 0),
                ("use_virt", 0, -1), ("materialise", 192, -1), ("first_wgrad", "Taps", 0)],
               [("dense_wgrad", "F34", None), ("newmap", "Persistent", None), ("td_dgrad", "Persistent", None), ("td_dgrad", "Runs128", None), ("td_fwd", "Persistent", None)]),
}


@pytest.mark.parametrize("form", [c.tag for c in cov.cases("test_gpu_workspace_contract.test_portrait_network_backward_on_pattern")])
def test_portrait_network_backward_on_pattern(form):
    """2 x 160 x 96 -- a portrait grid -- through the fp64 oracle on the pass's own activation pattern, with the bounds of
    test_network_backward_kernel_forms (depth 1e-5; gradients GRAD_TOL, 5e-5 for the F(4x4, 3x3) forward, as there), on poisoned buffers.
    What each form runs here is asserted from the pass's plan (PORTRAIT_FORMS)."""
    case = cov.case("test_gpu_workspace_contract.test_portrait_network_backward_on_pattern", form)
    assert case.options == FORMS[form]
    n, h, w = case.shape
    with contract():
        with tp.kernel_options(case.options):
            state, model = tp.make_model(62)
        rng = np.random.default_rng(16)
        x = torch.from_numpy(rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float32))
        cot = torch.from_numpy(rng.standard_normal((n, 1, h, w)).astype(np.float32))
        model.train()
        y = model(x.to(tp.dev()))
        (pattern,) = tp.pattern_of(y, model, n, h, w)
        (y * cot.to(tp.dev())).sum().backward()
        torch.cuda.synchronize()
        tp.assert_plan(model, n, h, w, 1, *PORTRAIT_FORMS[form], what="portrait %s" % form)
    g64p = tp.reference_grads(state, x, cot, torch.float64, pattern)
    y64 = onet.forward(tp.state_as(state, torch.float64), x.double(), training=True, pattern=pattern)
    print("portrait %s: depth max err / max |depth| = %.2e" % (form, tp.rel_err(y, y64)))
    tp.assert_close(y, y64, 1e-5, "depth, %s kernels, portrait" % form)
    tp.assert_grads_on_pattern(dict(model.named_parameters()), g64p, None, 5e-5 if form == "winograd4" else tp.GRAD_TOL,
                               "network backward 2 x 160 x 96, %s kernels" % form)


# One shape per fixed scratch bound of endo_net_create_grouped that a SMALL input reaches better than the benchmark grids do (poison and guard
# runs: a forward and a backward pass, everything finite, every guard intact).  (shape, kernel forms, the plan entries the use rests on -- asserted --, bound, use):
BOUND_CASES = [
    # kGrowth * 163840 floats of split-K partials (dense_fwd): ksplit * n * plane floats per output channel.  The split form is taken with
    # tiles_small = ceil(w / 16) * ceil(h / 8) * n < 512 and ksplit = ceil(768 / tiles_small) from 256 tiles on: 3 slices up to 383 tiles, 2 from 384.
    # 383 x 32 x 64: level 2 is 8 x 16 = one whole tile per sample, 383 tiles, cin 144 ... 276 (9 ... 18 K-chunks) -> ksplit = 3:
    # 3 * 383 * 128 = 147 072 of 163 840 floats per channel = 89.8 %.  No input comes closer: 511 tiles x 2 slices is 130 816 (79.8 %).
    pytest.param((383, 32, 64), "default", [("dense_fwd_ksplit", 3, 2), ("dense_fwd", "SplitK", 2)], id="split-k-partials-383x32x64-89.8pct"),
    # kNsScratchFloats (n-split weight gradient, 1024 * 12 block-groups): a launch uses blocks * groups with (blocks, groups) <= (1024, 4), (768, 8),
    # (512, 12) or (256, 24): 6 144 of 12 288 = 50 % at most, whatever the input.  8 x 128 x 160 with the F(3x3, 4x4) form off: level 0 has
    # 5 120 row chunks (>= 2 048: the n-split kernel), denseBlocksUp.4's last layer cin = 180 -> 12 groups x 512 blocks = 50 %.
    pytest.param((8, 128, 160), "direct", [("dense_wgrad", "NSplit", 0), ("dense_wgrad", "Taps", 1)], id="nsplit-partials-8x128x160-50pct"),
    # kSpScratchFloats (sub-pixel transition-up weight gradient, 384 blocks): 6 x 128 x 160 -> the 64 x 80 low-resolution grid of the last transition
    # up has 3 * 64 * 6 = 1 152 = 3 * 384 chunks -> 384 blocks = 100 % of kSpScratchFloats.  (The region holds max(kNs, kSp, 4 * kF34) = kNs floats:
    # 64 % of the region; nothing reaches its end, the n-split form that sized it stops at 50 %.)
    # kFwPartBlocks * 192 doubles (final-conv weight partials of the persistent base pass at level 0): blocks x count doubles with
    # min(CU count, 512) = 256 blocks on an MI355X and count = the up block's 144 base channels = 37.5 %, whatever the input; every default-form
    # run at a size that takes the persistent base pass uses them (with ONE sample group they are the last thing in the workspace).
    pytest.param((6, 128, 160), "default", [("tu_wgrad", "Subpix", 0), ("base_pass", "Block8", 0)], id="subpixel-partials-6x128x160-100pct"),
]


@pytest.mark.parametrize("shape,form,takes", BOUND_CASES)
def test_shapes_closest_to_the_fixed_scratch_bounds(shape, form, takes):
    n, h, w = shape
    with contract() as g:
        with tp.kernel_options(FORMS[form]):
            _, model = tp.make_model(62)
        rng = np.random.default_rng(23)
        x = torch.from_numpy(rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float32)).to(tp.dev())
        cot = torch.from_numpy(rng.standard_normal((n, 1, h, w)).astype(np.float32)).to(tp.dev())
        model.train()
        y = model(x)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        g.check()
        tp.assert_plan(model, n, h, w, 1, takes, what="%s %s" % (shape, form))
        _finite("depth", y.detach().cpu())
        first = model.flat_gradients().cpu()
        _finite("gradients", first)
        _finite("running statistics", torch.cat([v.reshape(-1).float().cpu() for k, v in model.state_dict().items() if "running" in k]))
        # the same passes again on re-poisoned workspaces accumulate the same gradient (bound: test_network_backward's accumulated gradient)
        y = model(x)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        tp.assert_close(model.flat_gradients(), 2.0 * first, 1e-5, "accumulated gradient of two passes")


@pytest.mark.parametrize("groups", [c.groups for c in cov.cases("test_gpu_workspace_contract.test_three_and_four_sample_groups")])
def test_three_and_four_sample_groups(groups):
    """endo_net_create_grouped allows up to 4 sample groups and the kernels size LDS by kMaxGroups; no other test goes past 2.  With the bounds of
    test_forward_pair_is_two_calls: each group's depth equals a separate single-group call on that group's input to 2e-5 of the maximum, and the
    parameter gradient is the sum over the groups -- held, as there, to GRAD_TOL against the fp64 oracle evaluated on the activation pattern each
    group took.  The sum of the separate calls' own gradients is compared as well, but on the flat vector and at the round-1 "own patterns" criterion
    only (noise_aware): the grouped pass and a separate call sum their BatchNorm statistics in another order and so take different ReLU branches at
    a handful of borderline elements (measured: 13 of 5.7e7 bits with 3 groups, 19 of 7.5e7 with 4; the flat gradients then differ by 1.9e-3 / 7e-4 of their maximum), each an O(1) change of that pixel's gradient
    (device_pattern.py) -- the number of such bits is held to the 1e-5 of all bits that test_network_backward allows two evaluations."""
    n, h, w = cov.case("test_gpu_workspace_contract.test_three_and_four_sample_groups", str(groups)).shape
    rng = np.random.default_rng(31)
    x = torch.from_numpy(rng.uniform(-1, 1, (groups * n, 3, h, w)).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((groups * n, 1, h, w)).astype(np.float32))
    names = onet.trainable_names()
    with contract():
        state, model = tp.make_model(61)
        model.train()
        with torch.no_grad():
            y, tape = model._run_forward(x.to(tp.dev()), groups)
            model._run_backward(x.to(tp.dev()), tape, cot.to(tp.dev()), True, groups)
        torch.cuda.synchronize()
        patterns = pattern_from_tape(model, tape, n, h, w, groups)
        _finite("depth of the grouped call", y.cpu())
        summed, flips, bits = None, 0, 0
        for grp in range(groups):
            _, single = tp.make_model(61)
            single.train()
            xs, cs = x[grp * n:(grp + 1) * n].to(tp.dev()), cot[grp * n:(grp + 1) * n].to(tp.dev())
            with torch.no_grad():
                ys, tape_s = single._run_forward(xs, 1)
                single._run_backward(xs, tape_s, cs, True, 1)
            torch.cuda.synchronize()
            tp.assert_close(y[grp * n:(grp + 1) * n], ys, 2e-5, "depth of group %d of %d vs a separate call" % (grp, groups))
            (own,) = pattern_from_tape(single, tape_s, n, h, w, 1)
            flips += sum(int((own[k] != patterns[grp][k]).sum()) for k in own if k.startswith("relu::"))
            bits += sum(own[k].numel() for k in own if k.startswith("relu::"))
            grads = {k: p.grad.detach().double().cpu() for k, p in single.named_parameters()}
            summed = grads if summed is None else {k: summed[k] + grads[k] for k in grads}
    print("groups = %d: %d of %d ReLU bits differ between the grouped pass and the separate calls" % (groups, flips, bits))
    assert flips <= 1e-5 * bits
    g64 = None
    for grp in range(groups):
        part = tp.reference_grads(state, x[grp * n:(grp + 1) * n], cot[grp * n:(grp + 1) * n], torch.float64, patterns[grp])
        g64 = part if g64 is None else {k: g64[k] + part[k] for k in names}
    tp.assert_grads_on_pattern(dict(model.named_parameters()), g64, None, tp.GRAD_TOL, "%d sample groups" % groups)
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in names])
    flat64 = flat(g64)
    print("groups = %d: flat gradient vs the sum of the separate calls' gradients: max err / max %.2e" % (groups, tp.rel_err(model.flat_gradients(), flat(summed))))
    tp.noise_aware(model.flat_gradients(), flat(summed), flat64, "flat gradient of %d groups against the separate calls' sum" % groups, factor=4.0)
