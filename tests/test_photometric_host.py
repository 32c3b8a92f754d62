"""CPU-only checks of the photometric term (losses.PhotometricLoss, TrainingStep(photometric_weight=...)): the plain-torch restatement
(tests/photometric_restate.py) reproduces what the reference's own functions gave (tests/golden/photometric.npz, written by
tests/golden/make_photometric_golden.py), the fixture holds the conditions it was built under, and the host side -- the exported
name, the C entry points in the ctypes table, the header and the library, refusals, argument validation -- behaves.  No GPU compute is
launched here."""

import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import image_warp_restate as iwr
import photometric_restate as pr

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "photometric.npz"
ENTRY_POINTS = ("endo_photometric_workspace_floats", "endo_photometric_fwd", "endo_photometric_bwd",
                "endo_loss_head_photo_workspace_floats", "endo_loss_head_photo")


def arr(g, key):
    return torch.from_numpy(np.array(g[key]))


def rel(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("mode", pr.MODES)
def test_restatement_reproduces_module_record(golden, mode):
    """Loss and depth gradient to 1e-6 (max abs error / max |ref|): the same ATen calls."""
    g = golden(FIXTURE)
    x = iwr.chain_batch()
    loss, grad = pr.value_and_grad(arr(g, "module::colors_1"), arr(g, "module::colors_2"), arr(g, "module::depth"), x["mask"],
                                   arr(g, "module::intersect_masks"), x["t"], x["R"], x["K"], 1.0, mode)
    want = arr(g, "module::%s::grad_depth" % mode)
    assert rel(loss, arr(g, "module::%s::loss" % mode)) <= 1e-6
    assert grad.shape == want.shape == (2, 1, 32, 64) and float(want.abs().max()) > 0
    assert rel(grad, want) <= 1e-6, "%s: %.3e" % (mode, rel(grad, want))


def test_fixture_holds_the_conditions_it_records(golden):
    """What make_photometric_golden.py asserts as it writes, read back from the file."""
    g = golden(FIXTURE)
    x = iwr.chain_batch()
    depth, inter = arr(g, "module::depth"), np.array(g["module::intersect_masks"])
    assert set(np.unique(inter).tolist()) <= {0.0, 1.0} and inter.shape == (2, 1, 32, 64)
    on = inter[:, 0] > 0.5
    u, v = pr.coordinates(depth, x["mask"], x["t"], x["R"], x["K"])
    ix, iy = u.astype(np.float64) - 0.5, v.astype(np.float64) - 0.5
    dist = np.minimum(np.abs(ix - np.round(ix)), np.abs(iy - np.round(iy)))
    assert dist[on].min() > pr.KINK_MARGIN and float(on.mean()) >= 0.30
    cond = np.array(g["module::conditions"])
    assert cond[0] > pr.KINK_MARGIN and cond[1] >= 0.30 and cond[2] >= 0.04
    assert abs(cond[0] - dist[on].min()) <= 1e-6 and cond[1] == float(on.mean())
    c1, c2 = np.array(g["module::colors_1"]), np.array(g["module::colors_2"])
    assert c1.shape == c2.shape == (2, 3, 32, 64) and max(iwr.adjacent_difference(c2)) <= 0.05
    with torch.no_grad():
        for mode in pr.MODES:
            warped = iwr.images_warping(torch.from_numpy(c2), torch.from_numpy(u), torch.from_numpy(v), mode).numpy()
            diff = np.abs(c1 - warped)[np.broadcast_to(on[:, None], c1.shape)]
            assert 0.04 <= diff.min() and diff.max() <= 0.51, (mode, diff.min(), diff.max())
    losses = np.array(g["head::losses"])
    assert losses.shape == (4,) and abs(losses[0] - losses[1:].sum()) <= 1e-6 * losses[0] and losses[3] > 0
    assert np.array(g["head::weights"]).tolist() == np.array([20.0, 0.1, 0.5], np.float32).tolist() and np.array(g["head::batch"]).tolist() == [2, 64, 96, 11, 300]
    for k in ("1", "2"):
        assert float(np.array(g["head::pred_" + k]).min()) > 0
        gp = np.array(g["head::grad_pred_" + k])
        assert gp.shape == (2, 1, 64, 96) and np.isfinite(gp).all() and np.abs(gp).max() > 0


def test_names_and_entry_points():
    assert ea.PhotometricLoss is ea.losses.PhotometricLoss
    text = open(os.path.join(ROOT, "include", "endo_hip.h")).read()
    declared = set(re.findall(r"\b(endo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = ea._lib.load()
    for name in ENTRY_POINTS:
        assert name in ea._lib.SIGNATURES and name in declared, name
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define ENDO_ABI_VERSION (\d+)", text).group(1)) == 7 == lib.endo_abi_version()
    assert lib.endo_photometric_workspace_floats(2, 5, 7) == 72 and lib.endo_photometric_workspace_floats(0, 5, 7) == -1
    assert lib.endo_loss_head_photo_workspace_floats(2, 8, 8) >= lib.endo_loss_head_workspace_floats(2, 8, 8) + 2 * 128
    assert lib.endo_loss_head_photo_workspace_floats(2, 0, 8) == -1


def test_entry_points_validate_before_any_device_work():
    lib = ea._lib.load()
    nul = [None] * 11
    assert lib.endo_photometric_fwd(*nul, 1, 3, 4, 4, 1.0, 0, None) == -1
    assert lib.endo_photometric_bwd(None, None, None, None, 0, 1, 4, 4, 1.0, None) == -1
    # sizes, modes, the accumulate switch and the alignment are checked before a pointer is touched: these are host addresses
    buf = ctypes.create_string_buffer(128)
    base = ctypes.addressof(buf)
    base += (-base) % 16
    a, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    for n, c, h, w, mode in ((0, 3, 4, 4, 0), (1, 0, 4, 4, 0), (1, 3, 0, 4, 0), (1, 3, 4, -1, 0), (1, 3, 4, 4, 3), (1, 3, 4, 4, -1),
                             (1, 3, 1 << 16, 1 << 16, 0)):
        assert lib.endo_photometric_fwd(*([a] * 11), n, c, h, w, 1.0, mode, None) == -1, (n, c, h, w, mode)
    assert lib.endo_photometric_fwd(*([a] * 10), odd, 1, 3, 4, 4, 1.0, 0, None) == -1          # misaligned workspace
    for acc, n, h, w in ((2, 1, 4, 4), (-1, 1, 4, 4), (0, 0, 4, 4), (0, 1, 0, 4), (1, 1, 4, 0), (0, 1, 1 << 16, 1 << 16)):
        assert lib.endo_photometric_bwd(a, a, a, a, acc, n, h, w, 1.0, None) == -1, (acc, n, h, w)
    assert lib.endo_photometric_bwd(a, a, odd, a, 0, 1, 4, 4, 1.0, None) == -1
    head = lambda colors, weight, mode, ws: lib.endo_loss_head_photo(*([a] * 16), colors, colors, 20.0, 0.1, weight, 1e-8, mode, a, a, a, ws,
                                                                     1, 4, 4, None)
    assert head(None, 0.5, 0, a) == -1 and head(a, -0.5, 0, a) == -1 and head(a, float("nan"), 0, a) == -1
    assert head(a, 0.5, 3, a) == -1 and head(a, 0.5, -1, a) == -1 and head(a, 0.5, 0, odd) == -1


def inputs(n=2, c=3, h=4, w=5):
    d = torch.ones(n, 1, h, w)
    return [torch.zeros(n, c, h, w), torch.zeros(n, c, h, w), d, d.clone(), d.clone(), torch.zeros(n, 3, 1), torch.eye(3).repeat(n, 1, 1),
            torch.eye(3).repeat(n, 1, 1)]


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.PhotometricLoss()(inputs())


def test_only_the_depth_is_differentiated():
    names = ("colors_1", "colors_2", None, "masks", "intersect_masks", "translations", "rotations", "intrinsics")
    for i, name in enumerate(names):
        if name is None:
            continue
        x = inputs()
        x[i] = x[i].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="no gradient"):
            ea.PhotometricLoss()(x)


def test_bad_arguments_raise_value_error():
    with pytest.raises(ValueError, match="padding_mode"):
        ea.PhotometricLoss(padding_mode="mirror")
    loss = ea.PhotometricLoss(epsilon=2.0, padding_mode="border")
    assert loss.epsilon == 2.0 and loss.padding_mode == "border"
    for i, bad in ((0, torch.zeros(2, 3, 4)), (1, torch.zeros(2, 1, 4, 5)), (2, torch.ones(2, 4, 5, 1)), (2, torch.ones(2, 3, 4, 5)),
                   (3, torch.ones(1, 1, 4, 5)), (4, torch.ones(2, 3, 4, 5)), (5, torch.zeros(2, 4)), (6, torch.eye(3).reshape(1, 3, 3)),
                   (7, torch.zeros(2, 3, 4))):
        x = inputs()
        x[i] = bad
        with pytest.raises(ValueError):
            loss(x)
    with pytest.raises(ValueError):
        loss(inputs()[:7])
    for kw in ({"photometric_weight": -0.1}, {"photometric_weight": float("nan")}, {"photometric_weight": 0.5, "photometric_padding": "mirror"},
               {"photometric_padding": "nearest"}):
        with pytest.raises(ValueError, match="photometric"):
            ea.train_step.TrainingStep(None, None, 4, 5, **kw)


def test_step_output_gains_photo_only_with_the_term():
    """StepOutput over host tensors (the glue's CPU form): four losses give today's keys, five add "photo"."""
    flag, norm = torch.zeros(1), torch.tensor([1.5], dtype=torch.float64)
    old = ea.train_step.StepOutput(torch.tensor([3.0, 1.0, 2.0, 0.0]), flag, norm, None)
    assert sorted(old.keys()) == ["dcl", "grad_norm", "loss", "sfl", "skipped"] and "photo" not in old
    new = ea.train_step.StepOutput(torch.tensor([3.5, 1.0, 2.0, 0.0, 0.5]), flag, norm, None)
    assert sorted(new.keys()) == ["dcl", "grad_norm", "loss", "photo", "sfl", "skipped"] and "photo" in new
    assert new["loss"] == 3.5 and float(new["photo"]) == 0.5 and float(new["sfl"]) == 2.0 and new["skipped"] is False
    skipped = ea.train_step.StepOutput(torch.tensor([float("nan"), 1.0, 2.0, 1.0, 0.5]), torch.ones(1), norm, None)
    assert skipped["skipped"] is True and bool(torch.isnan(skipped["photo"]))
