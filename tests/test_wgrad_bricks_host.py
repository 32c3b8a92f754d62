"""CPU side of the fp32 WEIGHT-GRADIENT BRICKS (include/endo_hip.h; the GPU side is tests/test_gpu_wgrad_bricks.py): the restated operation
agrees with an independent formulation, every case of tests/wgrad_restate.py has the edge its comment claims, endo_wgrad_brick_ok of the
loaded library decides as the restated predicates do, the bounds are what the fp32 yardsticks give, and every case can tell the mistake
it exists for from the truth.  No device is needed.

Yardsticks measured here (max |fp32 - fp64| / max |fp64|, worst case of each family) and the bounds they give (4 x, one digit, up):
    f34 2.8e-6 (first_16x32 F34Prep; f34_segq2_cin2052 2.8e-6, the cases of up to 84 channels 1.0e-6 .. 2.3e-6) -> 2e-5
    nsplit 3.6e-7 -> 2e-6   taps, direct, subpix 4.8e-7 -> 2e-6   td_plain, td_dma 2.7e-7 -> 2e-6
(torch's own fp32 convolution on one thread: oneDNN's result moves between 1.2e-6 and 4.7e-6 with the thread count on
nsplit_three_chunks_per_block, no yardstick for a bound that has to hold on every machine.)
The F(3x3, 4x4) yardstick follows the kernel's own order of operations (wgrad_restate.f34_dw): column pass, row pass, the 36 sums over
the tiles of ONE wave's walk, that wave's output transform, then the sum of the partial dW.  A single output transform behind the sum
over all tiles is another algorithm -- the 36 sums grow with the tile count and cancel in the transform -- and lies 5.1e-6 .. 6.0e-6
from float64 on the three cases that put every wave of the chip to work."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import wgrad_restate as wr

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
ALL = wr.CASES + wr.BATCH_CASE
PAIRS = [(c, f) for c in ALL for f in c["forms"]]
POINTERS = ("in", "dy", "saved", "gamma", "beta", "dy_idx", "prep_x", "prep_p", "prep_q", "prep_bias", "dw")


def ids(c):
    return c["name"]


def fake_ptrs(c, misalign=None):
    """addresses nobody dereferences, aligned as the caching allocator aligns them"""
    ptrs = {"in": 0x10000000, "dy": 0x20000000, "dw": 0x30000000}
    if c["kind"] in (wr.DENSE, wr.TD):
        ptrs.update({"saved": 0x40000000, "gamma": 0x41000000, "beta": 0x42000000})
    if c["kind"] == wr.TD:
        ptrs["dy_idx"] = 0x50000000
    if c["prep"]:
        ptrs.update({"prep_x": 0x60000000, "prep_p": 0x61000000, "prep_q": 0x62000000, "prep_bias": 0x63000000})
    if misalign:
        ptrs[misalign] += 4
    return ptrs


def c_operands(o):
    a = ea._lib.WgradOperands()
    for name, _ in a._fields_:
        key = "in" if name == "in_" else name
        setattr(a, name, (o[key] or None) if key in POINTERS else o[key])
    return a


def lib_ok(kind, form, o):
    return int(ea._lib.load().endo_wgrad_brick_ok(kind, form, ctypes.byref(c_operands(o))))


# ---- reference ----
@pytest.mark.parametrize("c", ALL, ids=ids)
def test_reference_agrees_with_the_nine_tap_sum(c):
    """autograd of F.conv2d in float64 against one einsum per tap over the shifted window, to 1e-12 of the tensor's maximum"""
    ops = wr.make_case(c)
    lg = wr.logical(c, ops)
    a = wr.activation(c, ops, lg["x"])
    for form in sorted({"F34Prep" if f == "F34Prep" else None for f in c["forms"]}, key=str):
        ref = wr.reference(c, form)["dw"]
        other = wr.taps_dw(a, wr.gradient(c, ops, lg, form), wr.ksize(c))
        assert ref.shape == (c["cout"], c["cin"], wr.ksize(c), wr.ksize(c))
        assert wr.rel_err(other, ref) <= 1e-12


@pytest.mark.parametrize("c", [k for k in ALL if "F34" in k["forms"] or "F34Prep" in k["forms"]][:6], ids=ids)
def test_winograd_restatement_is_the_operation(c):
    """A^T [ sum (S g S^T) .* (B^T d B) ] A in float64 is dW (the fp32 evaluation of the same lines is the F34 yardstick)"""
    ops = wr.make_case(c)
    lg = wr.logical(c, ops)
    got = wr.f34_dw(wr.activation(c, ops, lg["x"]), wr.gradient(c, ops, lg), np.float64)
    assert wr.rel_err(got, wr.reference(c)["dw"]) <= 1e-12


@pytest.mark.parametrize("c", ALL, ids=ids)
def test_inputs(c):
    """about half the activations positive; no more dW elements below 1e-3 of the maximum than chance gives (every input channel's
    elements taken as normal with that channel's own rms: the expected fraction is the mean of erf(t / (rms sqrt 2)))"""
    ops = wr.make_case(c)
    lg = wr.logical(c, ops)
    if c["kind"] in (wr.DENSE, wr.TD):
        assert 0.4 < float((wr.activation(c, ops, lg["x"]) > 0).mean()) < 0.6
    if c["kind"] == wr.TD:
        assert sorted(np.unique(lg["codes"]).tolist()) == [0, 1, 2, 3]          # all four window positions occur
    dw = wr.reference(c)["dw"]
    t = 1e-3 * float(dw.abs().max())
    rms = dw.pow(2).mean(dim=(0, 2, 3)).sqrt()
    chance = float(torch.erf(t / (rms * 2 ** 0.5)).mean())
    small = float((dw.abs() < t).double().mean())
    assert small <= 1.5 * chance + 3.0 * (chance / dw.numel()) ** 0.5, (small, chance)


# ---- edges ----
@pytest.mark.parametrize("c", ALL, ids=ids)
def test_case_has_the_edge_it_exists_for(c):
    e, n, h, w, cin, cout = c["edge"], c["n"], c["h"], c["w"], c["cin"], c["cout"]
    group_n = c["group_n"] or n
    if "F34" in c["forms"] and c["kind"] == wr.DENSE:
        plan = wr.f34_plan(n, h, w, cin)
        total, written = wr.f34_scratch_rows(plan)
        assert total * 256 <= wr.K_F34_SCRATCH and plan["groups"] * plan["wpg"] <= 256
        walks = wr.f34_walks(plan)
        assert sorted(u for v in walks.values() for u in v) == sorted(list(range(plan["units"])) * plan["groups"])          # every unit once per channel group
        if "units" in e:
            assert plan["units"] == e["units"] and sum(1 for v in walks.values() if v) == plan["groups"] and written == 9 * 8 * plan["groups"]
        if "strip_rest" in e:
            assert w % 16 == e["strip_rest"]
        if "segq" in e:
            assert plan["segq"] == e["segq"]
        if e.get("mixed"):
            assert plan["wpg"] % 4 != 0 and wr.f34_mixed_blocks(plan)
        if "spb" in e:
            assert plan["spb"] >= e["spb"] and written < total          # rows past a group's last block: never written, never to be read
        if "walk" in e:
            crossing = [v for v in walks.values() if len(v) >= e["walk"] and len({wr.f34_unit_sample(plan, u) // group_n for u in v}) > 1]
            assert crossing and (wr.geometry(c)["gs"] % (h * w) != 0) and (wr.geometry(c)["in_gs"] % (h * w) != 0)
    if "cin_rest" in e:
        assert cin % 16 == e["cin_rest"]
    if e.get("subrange"):
        g = wr.geometry(c)
        assert g["in_ns"] > cin * g["in_cs"] and g["dy_ns"] > cout * g["dy_cs"] and g["in_off"] > 0
    if "NSplit" in c["forms"]:
        ns = wr.nsplit_launch(n, h, w, cin)
        assert ns["scratch_rows"] * 256 <= wr.K_NS_SCRATCH
        for key in ("ng", "passes", "per"):
            if key in e:
                assert ns[key] == e[key], (key, ns)
        if "chunk_rest" in e:
            assert w % 32 == e["chunk_rest"]
    if e.get("taps_partial"):
        assert w % 32 and h % 8 and wr.taps_launch(n, h, w, cin, cout)["tiles_x"] > 1
    if e.get("odd"):
        o = wr.make_operands(c, wr.geometry(c), fake_ptrs(c))
        assert [wr.brick_ok(wr.DENSE, f, o) for f in range(4)] == [False, False, False, True]
    if c["kind"] == wr.TD:
        assert wr.td_dma_shape(cin, cout) == e["shape"] and (w // 2) == e["pooled_w"] and e["pooled_w"] % 4 == 0 and e["pooled_w"] % 16 != 0
        assert (w + 31) // 32 * (h // 2) * n > e["dma_chunks_over"]
        assert wr.td_plain_launch(n, h, w, cin, cout)["tiles_ci"] == (1 if cin == 96 else 2)
    if c["kind"] == wr.TU:
        sp = wr.subpix_launch(n, h // 2, w // 2)
        assert (w // 2) % 32 == e["chunk_rest"] and sp["per"] == e["per"] and sp["blocks"] * 3 * 27 * 256 <= wr.K_SP_SCRATCH
        assert wr.taps_launch(n, h, w, cin, cout)["tiles"] > wr.taps_launch(n, h, w, cin, cout)["groups"]
        assert wr.direct_launch(n, h, w, cin, cout, 1)["tiles"] > wr.direct_launch(n, h, w, cin, cout, 1)["groups"]


def test_every_enumerator_has_a_case_and_the_batch_its_four_plans():
    seen = {(c["kind"], f) for c in wr.CASES for f in c["forms"]}
    assert seen == {(k, f) for k, names in wr.FORMS.items() for f in names}
    assert {wr.f34_plan(c["n"], c["h"], c["w"], c["cin"])["segq"] for c in wr.DENSE_CASES if "F34" in c["forms"]} == {1, 2, 4}
    assert {wr.nsplit_launch(c["n"], c["h"], c["w"], c["cin"])["ng"] for c in wr.DENSE_CASES if "NSplit" in c["forms"]} == {1, 2, 3}
    plans = [wr.f34_plan(c["n"], c["h"], c["w"], c["cin"]) for c in wr.BATCH_CASE]
    assert [p["groups"] for p in plans] == [3, 4, 5, 6]          # gmax = 6: the blocks past a layer's own groups return early


# ---- predicates ----
@pytest.mark.parametrize("c", ALL, ids=ids)
def test_library_predicate_agrees_on_every_case(c):
    lib = ea._lib.load()
    o = wr.make_operands(c, wr.geometry(c), fake_ptrs(c))
    for form, name in enumerate(wr.FORMS[c["kind"]]):
        assert lib_ok(c["kind"], form, o) == int(wr.brick_ok(c["kind"], form, o)), name
        if name in c["forms"]:
            assert wr.brick_ok(c["kind"], form, o), name
        assert int(lib.endo_wgrad_brick_scratch_floats(c["kind"], form)) == wr.scratch_floats(c["kind"], form)


def test_library_predicate_agrees_on_near_misses():
    lib = ea._lib.load()
    base = next(c for c in wr.CASES if c["name"] == "dense_shared_16x32_cin40")
    td = next(c for c in wr.CASES if c["name"] == "td_96_64x40")
    tu = wr.TU_CASES[0]
    first = wr.FIRST_CASES[0]
    misses = []
    for change in ({"w": 30}, {"h": 24}, {"cin": 12}, {"cout": 24}, {"n": 0}):
        c = dict(base, **change)
        misses.append((c, wr.make_operands(c, wr.geometry(c), fake_ptrs(c))))
    for field in ("in", "dy"):
        misses.append((base, wr.make_operands(base, wr.geometry(base), fake_ptrs(base, misalign=field))))
    for c in (base, td):
        o = wr.make_operands(c, wr.geometry(c), fake_ptrs(c))
        misses += [(c, dict(o, saved=0)), (c, dict(o, dw=0)), (c, dict(o, in_ns=o["in_ns"] - 4)), (c, dict(o, group_n=3)), (c, dict(o, dy_cs=o["dy_cs"] - 4))]
    o = wr.make_operands(td, wr.geometry(td), fake_ptrs(td))
    misses += [(td, dict(o, dy_idx=0)), (td, dict(o, dy_idx=o["dy_idx"] + 2)), (td, dict(o, gs=o["gs"] + 2)), (td, dict(o, h=63))]
    o = wr.make_operands(tu, wr.geometry(tu), fake_ptrs(tu))
    misses += [(tu, dict(o, cin=32)), (tu, dict(o, w=70))]
    o = wr.make_operands(first, wr.geometry(first), fake_ptrs(first))
    misses += [(first, dict(o, prep_x=0)), (first, dict(o, cin=17)), (first, dict(o, cout=40))]
    refused = 0
    for c, o in misses:
        for form in range(len(wr.FORMS[c["kind"]])):
            want = int(wr.brick_ok(c["kind"], form, o))
            assert lib_ok(c["kind"], form, o) == want, (c["name"], form, o)
            refused += 1 - want
    assert refused > 40
    assert lib.endo_wgrad_brick_ok(wr.DENSE, 4, ctypes.byref(c_operands(wr.make_operands(base, wr.geometry(base), fake_ptrs(base))))) == 0
    assert lib.endo_wgrad_brick_ok(7, 0, None) == 0 and lib.endo_wgrad_brick_scratch_floats(wr.TD, 2) < 0


# ---- bounds ----
@pytest.fixture(scope="module")
def yardsticks():
    torch.manual_seed(0)
    worst = {k: (0.0, None) for k in wr.YARDSTICKS}
    for c, form in PAIRS:
        family = wr.FAMILY[(c["kind"], form)]
        y = wr.yardstick(c, form)
        print("yardstick %-8s %-32s %-8s %.3e" % (family, c["name"], form, y))
        if y > worst[family][0]:
            worst[family] = (y, c["name"])
    return worst


def test_recorded_yardsticks_are_what_the_fp32_evaluations_give(yardsticks):
    """YARDSTICKS of wgrad_restate.py against the measurement (a maximum over many elements: a BLAS that sums in another order moves it, so the
    record has to lie within a factor 1.5 of it), and BOUNDS = 4 x the record, rounded up to one digit"""
    for family, (y, name) in yardsticks.items():
        rec = wr.YARDSTICKS[family]
        print("%-8s measured %.3e (%s)  recorded %.3e  bound %.0e" % (family, y, name, rec, wr.BOUNDS[family]))
        assert rec / 1.5 <= y <= rec * 1.5, family
        assert wr.BOUNDS[family] == wr.round_up_one_digit(4.0 * rec)
        assert 4.0 * rec <= wr.BOUNDS[family] < 4.0 * rec * 2.0 + 1e-30


@pytest.mark.parametrize("family", sorted(wr.YARDSTICKS))
def test_every_bound_lies_below_the_network_bound(family):
    """a brick bound at or above GRAD_TOL would say nothing the whole-network tests do not"""
    assert wr.BOUNDS[family] < wr.GRAD_TOL, (family, wr.BOUNDS[family])


# ---- sensitivity ----
SENSITIVITY = [
    # (mutation, case, form)
    ("drop_tile", "f34_minimum_1x16x16", "F34"), ("drop_tile", "f34_walk_group_change", "F34"), ("drop_tile", "f34_segq4_cin2052", "F34"),
    ("drop_tile", "first_16x32", "F34"), ("drop_tile", "first_16x32", "F34Prep"),
    ("drop_chunk", "nsplit_w40_h5_ng1", "NSplit"), ("drop_chunk", "nsplit_three_chunks_per_block", "NSplit"), ("drop_chunk", "taps_11x44_cin20", "Taps"),
    ("drop_chunk", "direct_9x37_cin17", "Direct"), ("drop_chunk", "td_96_64x40", "Dma"), ("drop_chunk", "td_144_16x24", "Plain"), ("drop_chunk", "tu_48_6x72", "Subpix"),
    ("right_columns", "f34_partial_strip_cin60", "F34"), ("right_columns", "nsplit_w40_h5_ng1", "NSplit"), ("right_columns", "taps_11x44_cin20", "Taps"),
    ("halo_side", "dense_shared_16x32_cin40", "F34"), ("halo_side", "f34_mixed_blocks_spb", "F34"),
    ("group_table", "f34_walk_group_change", "F34"), ("group_table", "dense_shared_16x32_cin40", "NSplit"), ("group_table", "nsplit_w40_h5_ng1", "Taps"),
    ("group_table", "td_96_64x40", "Dma"), ("group_table", "td_96_64x40", "Plain"),
    ("last_group_shift", "f34_partial_strip_cin60", "F34"), ("last_group_shift", "f34_cin84", "F34"), ("last_group_shift", "f34_cin72_subrange", "F34"),
    ("last_group_shift", "nsplit_ng2_cin84", "NSplit"), ("last_group_shift", "taps_11x44_cin20", "Taps"),
    ("unpool_swap", "td_96_64x40", "Dma"), ("unpool_swap", "td_144_16x24", "Dma"), ("unpool_swap", "td_144_16x24", "Plain"),
]


@pytest.mark.parametrize("which,name,form", SENSITIVITY, ids=lambda v: str(v))
def test_case_sees_the_mistake_it_exists_for(which, name, form):
    """the float64 operation with one mistake a kernel can make differs from the true one by at least 10 x the form's bound"""
    c = next(k for k in ALL if k["name"] == name)
    ref = wr.reference(c, form)["dw"]
    moved = wr.rel_err(wr.mutated(c, which, form), ref)
    print("%s on %s (%s): moves dW by %.2e of its maximum, bound %.0e" % (which, name, form, moved, wr.bound(c["kind"], form)))
    assert moved >= 10.0 * wr.bound(c["kind"], form)


def test_batched_reduction_sees_another_layers_channel_count():
    """one of four batched layers reduced with its neighbour's cin: dW lands on other elements"""
    for k, c in enumerate(wr.BATCH_CASE):
        ref = wr.reference(c)["dw"]
        other = wr.BATCH_CASE[(k + 1) % 4]["cin"]
        assert wr.rel_err(wr.batch_reduce_with(ref, other), ref) >= 10.0 * wr.bound(wr.DENSE, "F34")
