"""CPU-only checks around the backward bricks of the 16-bit-storage family (include/endo_hip.h endo_bf16_* / endo_f16_* wgrad, dgrad_bn,
dgrad_sumpool, dgrad_block, dgrad_weights): the symbols exist for both storage types in the header and the ctypes table, arguments
are refused before any device work, the workspace query agrees with the formulas of csrc/bf16_bwd_kernels.h, the fp64 restatements
(tests/bf16_backward_restate.py) agree with torch autograd on tiny inputs, and every case of the GPU module is SENSITIVE: a dropped
tile border row, a one-pixel shift of G, a neighbouring pool code or a dropped tap moves its reference by at least ten times the bound
the case is held to.  No GPU compute is launched here."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_backward_restate as bbr

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRICKS = ("dgrad_weight_elems", "dgrad_weights", "wgrad_partial_floats", "wgrad", "dgrad_bn", "dgrad_sumpool", "dgrad_block")
FORWARD = ("conv_weight_elems", "conv_weights", "conv")
PREFIX = {"bf16": "endo_bf16_", "fp16": "endo_f16_"}


def fn(lib, storage, name):
    return getattr(lib, PREFIX[storage] + name)


@pytest.mark.parametrize("storage", ["bf16", "fp16"])
def test_symbols_exist_in_both_storage_types(storage):
    text = open(os.path.join(ROOT, "include", "endo_hip.h")).read()
    declared = set(re.findall(r"\b(endo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = ea._lib.load()
    for name in BRICKS + FORWARD:
        full = PREFIX[storage] + name
        assert full in declared and full in ea._lib.SIGNATURES and hasattr(lib, full), full
    for name in BRICKS:
        assert ea._lib.SIGNATURES["endo_bf16_" + name] == ea._lib.SIGNATURES["endo_f16_" + name]
    assert lib.endo_abi_version() == 7          # additive entries


def _host_pointer():
    buf = ctypes.create_string_buffer(256)          # a host address no kernel may see: every call below must return before a launch
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def _wgrad_args(ptr, **kw):
    a = ptr
    d = dict(a=a, a_t=64, a_blk=32, ac0=0, cin=32, cin_w=0, ups=0, saved=a, gamma=a, beta=a, rot=0, rot_n=0, group_n=0, gs_saved=0, g=a, g_t=32, g_blk=32,
             gc0=0, cout=16, g_idx=None, gscale=None, partial=a, cap=1 << 40, dw=a, n=2, h=8, w=8, ks=3)
    d.update(kw)
    return [d[k] for k in ("a", "a_t", "a_blk", "ac0", "cin", "cin_w", "ups", "saved", "gamma", "beta", "rot", "rot_n", "group_n", "gs_saved", "g", "g_t",
                           "g_blk", "gc0", "cout", "g_idx", "gscale", "partial", "cap", "dw", "n", "h", "w", "ks")] + [None]


@pytest.mark.parametrize("storage", ["bf16", "fp16"])
def test_bad_arguments_are_refused_before_any_device_work(storage):
    lib = ea._lib.load()
    keep, a = _host_pointer()
    wgrad = fn(lib, storage, "wgrad")
    bad = [dict(a=None), dict(g=None), dict(partial=None), dict(dw=None), dict(cin=30), dict(cin=34), dict(ac0=4), dict(ac0=12), dict(cout=10), dict(gc0=2),
           dict(ks=1, cout=12), dict(ks=1, gc0=4), dict(ks=2), dict(n=3, group_n=1), dict(n=0), dict(h=0), dict(w=-1), dict(ac0=40), dict(gc0=24),
           dict(saved=a, gamma=None), dict(ups=1, h=7), dict(ks=1, g_idx=a, w=7), dict(ks=3, g_idx=a), dict(cin_w=33), dict(rot=8, rot_n=8),
           dict(rot=4, rot_n=40), dict(cap=0), dict(cap=int(fn(lib, storage, "wgrad_partial_floats")(2, 8, 8, 32, 16, 3)) - 1), dict(a_t=48)]
    for kw in bad:
        assert wgrad(*_wgrad_args(a, **kw)) == -1, kw
    assert fn(lib, storage, "wgrad_partial_floats")(0, 8, 8, 32, 16, 3) == -1 and fn(lib, storage, "wgrad_partial_floats")(1, 8, 8, 32, 16, 2) == -1
    assert fn(lib, storage, "dgrad_weight_elems")(12, 0, 3) == -1 and fn(lib, storage, "dgrad_weight_elems")(12, 60, 3) == 2 * 9 * 3 * 16 * 32
    dw = fn(lib, storage, "dgrad_weights")
    for args in ((None, 12, 60, 3, 0, 0, 0, 0, a), (a, 12, 60, 3, 0, 0, 0, 0, None), (a, 12, 60, 2, 0, 0, 0, 0, a), (a, 12, 60, 3, 48, 48, 0, 0, a),
                 (a, 12, 60, 3, 0, 0, 40, 0, a), (a, 12, 60, 3, 0, 0, 48, 24, a), (a, 12, 60, 1, 0, 0, 48, 0, a), (a, 12, 60, 3, 0, 0, 96, 0, a)):
        assert dw(*args, None) == -1, args
    # dgrad_bn: g, g_t, g_blk, gc0, gcount, wgt, layer_cin, out, x, out_t, out_blk, co_off, cout, saved, gamma, beta, rot, rot_n, group_n, gs_saved,
    # out_sums, gs_out_sums, slot stride, salt, in_idx, n, h, w, ks
    def bn_args(**kw):
        d = dict(g=a, g_t=96, g_blk=32, gc0=60, gcount=12, wgt=a, layer_cin=60, out=a, x=a, out_t=96, out_blk=32, co_off=48, cout=12, saved=a, gamma=a, beta=a,
                 rot=0, rot_n=0, group_n=0, gs_saved=0, sums=a, gs_sums=0, stride=0, salt=1, idx=None, n=1, h=8, w=8, ks=3)
        d.update(kw)
        return list(d.values()) + [None]
    dgrad_bn = fn(lib, storage, "dgrad_bn")
    for kw in (dict(g=None), dict(wgt=None), dict(out=None), dict(x=None), dict(saved=None), dict(sums=None), dict(co_off=84, cout=0), dict(co_off=84, cout=12, layer_cin=96),
               dict(gcount=10), dict(cout=10), dict(gc0=62), dict(gc0=88), dict(cout=16), dict(ks=1), dict(idx=a), dict(ks=1, idx=a, h=7), dict(ks=1, idx=a, co_off=0, cout=48),
               dict(n=3, group_n=2), dict(stride=8), dict(g_blk=12), dict(out_t=40)):
        assert dgrad_bn(*bn_args(**kw)) == -1, kw
    sumpool = fn(lib, storage, "dgrad_sumpool")
    ok = dict(g=a, g_t=96, g_blk=32, gc0=48, gcount=48, wgt=a, out=a, out_t=96, out_blk=32, oc0=48, cout=48, sums=a, salt=1, n=1, h=8, w=8)
    for kw in (dict(g=None), dict(out=None), dict(sums=None), dict(h=7), dict(w=9), dict(gc0=52), dict(oc0=50), dict(oc0=64), dict(gcount=50), dict(n=0)):
        d = dict(ok); d.update(kw)
        assert sumpool(*(list(d.values()) + [None])) == -1, kw
    block = fn(lib, storage, "dgrad_block")
    four = (ctypes.c_void_p * 4)(a.value, a.value, a.value, a.value)
    null4 = (ctypes.c_void_p * 4)(a.value, None, a.value, a.value)
    okb = dict(d=a, x=a, t=96, blk=32, gc0=48, c0=48, wgt=four, saved=four, gamma=four, beta=four, sums=four, rot=0, rot_n=0, group_n=0, gs_saved=0, gs_sums=0,
               stride=0, salt=1, n=1, h=8, w=8)
    for kw in (dict(d=None), dict(x=None), dict(wgt=None), dict(sums=null4), dict(c0=84, gc0=88), dict(c0=0), dict(gc0=52), dict(gc0=40), dict(gc0=64), dict(blk=12),
               dict(rot=48, rot_n=96), dict(n=3, group_n=2), dict(stride=8), dict(h=0)):
        d = dict(okb); d.update(kw)
        assert block(*(list(d.values()) + [None])) == -1, kw
    del keep


@pytest.mark.parametrize("storage", ["bf16", "fp16"])
def test_workspace_query_agrees_with_the_launcher_formulas(storage):
    lib = ea._lib.load()
    query = fn(lib, storage, "wgrad_partial_floats")
    for c in bbr.WGRAD_CASES:
        assert query(c["n"], c["h"], c["w"], c["cin"], c["cout"], c["ks"]) == bbr.wgrad_partial_floats(c["n"], c["h"], c["w"], c["cin"], c["cout"], c["ks"]), c["name"]
    for cout, cin, ks in ((12, 60, 3), (12, 324, 3), (96, 96, 1), (48, 48, 3), (160, 160, 1)):
        assert fn(lib, storage, "dgrad_weight_elems")(cout, cin, ks) == ((cout + 31) // 32) * ((cin + 47) // 48) * ks * ks * 3 * 16 * 32


def test_the_walk_cases_walk():
    """what the comments of WGRAD_CASES promise, from bf16_wgrad_blocks restated"""
    by = {c["name"]: c for c in bbr.WGRAD_CASES}
    for name, blocks, tiles in (("dense_cin384_cout48_walk", 28, 96), ("td_cin768_cout160_walk", 32, 102), ("dense_cin60_odd", 20, 20), ("dense_cin84_odd", 20, 20)):
        c = by[name]
        assert bbr.wgrad_blocks(c["n"], c["h"], c["w"], c["cin"], c["cout"], c["ks"]) == (blocks, tiles), name
    for name in ("dense_cin384_cout48_walk", "td_cin768_cout160_walk"):
        c = by[name]
        blocks, tiles = bbr.wgrad_blocks(c["n"], c["h"], c["w"], c["cin"], c["cout"], c["ks"])
        assert tiles // blocks >= 3 and tiles % blocks != 0          # every block walks at least three tiles, some one more
    sides = set()
    for c in bbr.WGRAD_CASES:
        if c["name"].startswith("grid_"):
            sides.update((c["h"], c["w"]))
    assert {1, 3, 4, 5, 31, 32, 33} <= sides
    c = by["td_96_codes_all4"]
    codes = bbr.make_wgrad_case(c, "bf16")["codes"]
    assert all(len(set(codes[0, y, x].tolist())) == 4 for y in range(codes.shape[1]) for x in range(codes.shape[2]))


def test_restatements_against_autograd():
    """the written-out pieces (upsampling, unpooling, sum-pooling, the transposed convolution, the BatchNorm / ReLU backward, the channel
    rotation) against torch autograd of the forward operation in float64, on tiny inputs"""
    g = torch.Generator().manual_seed(5)
    a = torch.randn(2, 3, 4, 5, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.equal(bbr.upsample2(a.detach()), F.interpolate(a.detach(), scale_factor=2, mode="nearest"))
    cot = torch.randn(2, 3, 8, 10, dtype=torch.float64, generator=g)
    (F.interpolate(a, scale_factor=2, mode="nearest") * cot).sum().backward()
    assert torch.allclose(bbr.sumpool2(cot), a.grad, rtol=0, atol=1e-14)
    # max-unpooling from codes = the gradient of max_pool2d where the codes are the argmax positions
    z = torch.randn(2, 3, 8, 10, dtype=torch.float64, generator=g, requires_grad=True)
    pooled, idx = F.max_pool2d(z, 2, return_indices=True)
    yy, xx = idx // 10, idx % 10
    codes = ((yy % 2) * 2 + (xx % 2)).permute(0, 2, 3, 1).to(torch.uint8)
    gp = torch.randn_like(pooled)
    (pooled * gp).sum().backward()
    assert torch.equal(bbr.unpool2(gp, codes), z.grad)
    # data gradient of BN -> ReLU -> conv with a rotated parameter order, and its sums
    for ks in (1, 3):
        cin, cout, rot, rot_n = 6, 4, 2, 5
        x = torch.randn(2, cin, 5, 7, dtype=torch.float64, generator=g, requires_grad=True)
        wt = torch.randn(cout, cin, ks, ks, dtype=torch.float64, generator=g, requires_grad=True)
        sc, sh = torch.randn(cin, dtype=torch.float64, generator=g), torch.randn(cin, dtype=torch.float64, generator=g)
        pc = torch.from_numpy(bbr.rot_index(np.arange(cin), rot, rot_n).astype(np.int64))          # buffer channel -> parameter
        act = torch.relu(x * sc[pc].view(1, -1, 1, 1) + sh[pc].view(1, -1, 1, 1))
        inv = torch.empty_like(pc); inv[pc] = torch.arange(cin)
        y = F.conv2d(act[:, inv], wt, padding=ks // 2)          # the reference convolves the channels in parameter order
        gy = torch.randn_like(y)
        (y * gy).sum().backward()
        dz = bbr.conv_data_grad(gy, wt.detach())[:, pc]
        mask = bbr.relu_mask(x.detach(), sc[pc].view(1, -1, 1, 1), sh[pc].view(1, -1, 1, 1))
        da = torch.where(mask, dz, torch.zeros_like(dz))
        assert torch.allclose(sc[pc].view(1, -1, 1, 1) * da, x.grad, rtol=0, atol=1e-12)
        dw_buf = bbr.conv_weight_grad(act.detach(), gy, ks)
        dw = torch.zeros_like(dw_buf); dw[:, pc] = dw_buf
        assert torch.allclose(dw, wt.grad, rtol=0, atol=1e-12)
    assert bbr.rot_index(np.arange(8), 2, 5).tolist() == [2, 3, 4, 0, 1, 5, 6, 7]
    # spacing of the storage types
    t = torch.tensor([1.0, 1.5, 2.0, 0.75, 3e-5, 1e-8, 1000.0], dtype=torch.float64)
    assert bbr.ulp(t, "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -23, 2.0 ** -34, 4.0]
    assert bbr.ulp(t, "fp16").tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 0.5]


def test_weight_layout_restatement_places_every_weight_once():
    """the data-gradient layout's restatement: every weight of the layer appears exactly once, rows below `base` inside their K window"""
    rng = np.random.default_rng(3)
    wt = torch.from_numpy(rng.integers(1, 1 << 20, (12, 60, 3, 3)).astype(np.float32))
    flat = bbr.dgrad_weight_layout(wt, 0, 0, 48, 12)
    assert sorted(flat[flat != 0].tolist()) == sorted(wt.reshape(-1).tolist())
    lay = flat.reshape(1, 2, 9, 3, 16, 32)
    assert (lay[0, 1, :, 0, :12, 12:] == 0).all() and (lay[0, 1, :, 0, :12, :12] != 0).all()          # rows 48..59: plain k = co
    # row 5 of group 0 (base): co at k = 12 + co, slot k / 8 at position (k / 8) ^ ((5 >> 1) & 3)
    row = lay[0, 0, 4, 0, 5]
    want = np.zeros(32, np.float32)
    for co in range(12):
        k = 12 + co
        want[(((k >> 3) ^ 2) << 3) | (k & 7)] = wt[co, 5, 1, 1]          # centre tap
    assert np.array_equal(row, want)


@pytest.mark.parametrize("case", bbr.WGRAD_CASES, ids=lambda c: c["name"])
def test_weight_gradient_cases_are_sensitive(case):
    """a border row of one tile zeroed, G shifted by one pixel, a neighbouring pool code: each moves the fp64 reference by >= 10 x the bound"""
    for storage in ("bf16", "fp16"):
        ops = bbr.make_wgrad_case(case, storage)
        ref = bbr.wgrad_reference(case, ops, storage)
        scale = float(ref.abs().max())
        assert scale > 0
        for perturb in ("zero_row", "shift_x") + (("code",) if case["codes"] else ()):
            moved = float((bbr.wgrad_reference(case, ops, storage, perturb) - ref).abs().max()) / scale
            assert moved >= 10.0 * bbr.WGRAD_BOUND[storage], (storage, perturb, moved)
        if case["cin"] >= 384:
            break          # (the large cases: one storage type; the operands differ only in their rounding)


@pytest.mark.parametrize("name", ["c48_j3", "c96", "oc288", "c96_rot"])
def test_data_gradient_cases_are_sensitive(name):
    """one case per kernel form with one tap dropped: the reference moves by >= 10 x the element bound (one storage ulp plus the allowance)"""
    case = [c for c in bbr.DGRAD_CASES if c["name"] == name][0]
    for storage in ("bf16", "fp16"):
        ops = bbr.make_dgrad_case(case, storage)
        chans, add, sums, mag = bbr.dgrad_reference(case, ops, storage)
        old = ops["d"][:, chans].double()
        tol = bbr.dgrad_tolerance(old + add, old.abs() + mag, storage)
        _, add2, sums2, _ = bbr.dgrad_reference(case, ops, storage, drop_tap=0 if case["kind"] == "td" else 5)
        assert float((add2 - add).abs().max()) >= 10.0 * float(tol.max())
        for j in sums:
            assert float((sums2[j] - sums[j]).abs().max()) / float(sums[j].abs().max()) >= 10.0 * bbr.DGRAD_SUMS_BOUND[storage]
