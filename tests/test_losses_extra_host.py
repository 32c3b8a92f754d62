"""CPU-only checks of the six loss modules that finish the reference's losses.py (NormalizedWeightedMaskedL2Loss,
SparseMaskedL1LossDisplay, MaskedL1Loss, NormalizedL2Loss, NormalizedL1Loss, MaskedScaleInvariantLoss): the plain-torch restatement
(tests/losses_restate.py) reproduces what the reference's own classes gave (tests/golden/losses_extra_4x16x24.npz, written by
tests/golden/make_losses_golden.py), and the host side of the modules -- names, constructor defaults, refusals, argument validation of
the C entry points -- behaves.  No GPU compute is launched here."""

import importlib
import inspect

import numpy as np
import pytest
import torch

import losses_restate as lr

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

FIXTURE = "losses_extra_4x16x24.npz"


def record(g, which, names):
    return [torch.from_numpy(np.array(g["%s::%s" % (which, k)])) for k in names]


def rel(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("name", sorted(lr.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    """Values and gradients of the main record to 1e-6 relative (max abs error / max |ref|); the edge record's NaNs in the same
    places and its finite values to 1e-6."""
    g = golden(FIXTURE)
    _, names, ndiff, _ = lr.CASES[name]
    upstream = torch.from_numpy(np.array(g["main::display_upstream"])) if name == "SparseMaskedL1LossDisplay" else None
    value, grads = lr.value_and_grads(name, record(g, "main", names), upstream)
    want = torch.from_numpy(np.array(g["main::%s::loss" % name]))
    assert bool(torch.isfinite(want).all()) and value.dtype == torch.float32 and value.shape == want.shape
    assert rel(value, want) <= 1e-6, "%s value: %.3e" % (name, rel(value, want))
    assert len(grads) == ndiff
    for i, got in enumerate(grads):
        ref = torch.from_numpy(np.array(g["main::%s::grad%d" % (name, i)]))
        assert bool(torch.isfinite(ref).all()) and got.shape == ref.shape
        assert rel(got, ref) <= 1e-6, "%s gradient %d: %.3e" % (name, i, rel(got, ref))
    with torch.no_grad():
        edge = lr.CASES[name][0](*record(g, "edge", names)).reshape(-1)
    want = torch.from_numpy(np.array(g["edge::%s::loss" % name])).reshape(-1)
    assert torch.equal(torch.isnan(edge), torch.isnan(want)), name
    finite = ~torch.isnan(want)
    if bool(finite.any()):
        assert rel(edge[finite], want[finite]) <= 1e-6, name


def test_fixture_holds_the_cases_it_is_for(golden):
    """The properties make_losses_golden.py asserts as it writes, read back: exact ties under the mask, log(0) off the sparse mask, the
    masked sparse depth below 0.5, the empty sample and the zero translation of the edge record."""
    g = golden(FIXTURE)
    mask, depth, warped = (np.array(g["main::" + k]) for k in ("mask", "depth", "warped"))
    assert mask.shape == (4, 1, 16, 24) and set(np.unique(mask)) == {0.0, 1.0} and all(mask[i].sum() > 0 for i in range(4))
    assert int(((depth == warped) & (mask > 0)).sum()) >= 5
    sparse, smask = np.array(g["main::sparse"]), np.array(g["main::sparse_mask"])
    assert np.all(sparse[smask == 0] == 0) and int(((smask > 0) & (sparse < 0.5)).sum()) == 1
    assert np.array(g["main::images"]).shape == (4, 3, 16, 24)
    assert len(set(np.array(g["main::display_upstream"]).tolist())) == 4
    assert np.array(g["edge::mask"])[1].sum() == 0 and np.array(g["edge::sparse_mask"])[1].sum() == 0
    assert not np.array(g["edge::translations"])[0].any()
    for name in ("NormalizedL2Loss", "NormalizedL1Loss", "MaskedScaleInvariantLoss"):
        assert np.isnan(np.array(g["edge::%s::loss" % name]))
    for name in ("NormalizedWeightedMaskedL2Loss", "MaskedL1Loss"):
        assert np.isfinite(np.array(g["edge::%s::loss" % name]))
    assert np.array(g["edge::SparseMaskedL1LossDisplay::loss"])[1] == 0


def test_fp64_evaluation_of_the_restatement(golden):
    """The restatement is dtype-generic: on .double() inputs it returns fp64 and stays within fp32 rounding of the fp32 value."""
    g = golden(FIXTURE)
    for name, (fn, names, _, _) in lr.CASES.items():
        x = record(g, "main", names)
        v32, v64 = fn(*x), fn(*[t.double() for t in x])
        assert v64.dtype == torch.float64 and rel(v32, v64) <= 1e-5, name


def test_names_and_constructor_defaults():
    for name, (_, _, _, kw) in lr.CASES.items():
        cls = getattr(ea, name)
        assert cls is getattr(ea.losses, name) and issubclass(cls, torch.nn.Module)
        params = inspect.signature(cls.__init__).parameters
        assert list(params) == ["self"] + list(kw), name
        assert {k: params[k].default for k in kw} == kw, name
        module = cls()
        assert all(getattr(module, k) == v for k, v in kw.items()), name


def test_cpu_tensors_raise(golden):
    g = golden(FIXTURE)
    for name, (_, names, _, _) in lr.CASES.items():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(ea, name)()(record(g, "main", names))


def test_inputs_the_reference_never_differentiates_are_refused(golden):
    """A mask, a sparse depth map or a translation that asks for a gradient is an error, not a silent None -- decided before anything
    touches a device."""
    g = golden(FIXTURE)
    for name, (_, names, ndiff, _) in lr.CASES.items():
        for i in range(ndiff, len(names)):
            x = record(g, "main", names)
            x[i].requires_grad_(True)
            with pytest.raises(RuntimeError, match="no gradient"):
                getattr(ea, name)()(x)


def test_new_entry_points_validate_before_any_device_work():
    """ENDO_E_BADARG on null pointers, without a device (as endo_depth_scale_fwd in test_abi_and_host.py)."""
    lib = ea._lib.load()
    assert lib.endo_abi_version() == 7          # additive: the version stays
    for stem in ("norm_l2", "norm_l1", "weighted_l2", "masked_scale_inv", "sparse_l1_display"):
        for which in ("fwd", "bwd"):
            name = "endo_%s_%s" % (stem, which)
            _, argtypes = ea._lib.SIGNATURES[name]
            args = [None if t is ea._lib._P else (1.0 if t is ea._lib._F else 1) for t in argtypes]
            assert getattr(lib, name)(*args) == -1, name
    for name in ("endo_norm_l2_fwd", "endo_norm_l1_fwd", "endo_masked_scale_inv_fwd"):          # sizes are validated too
        assert getattr(lib, name)(None, None, None, None, None, 0, 16, 1e-3, None) == -1
