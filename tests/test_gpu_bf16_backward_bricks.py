"""The backward kernels of the 16-bit-storage family ONE BY ONE against fp64 (include/endo_hip.h, "BACKWARD BRICKS"): each test is a
single launch of endo_net16_bwd / endo_net16h_bwd -- the weight gradient (bf16_wgrad_kernel<3, 1> / <1, 3> + bf16_wgrad_reduce_kernel),
bf16_conv_kernel with the kEpiDgradBn epilogue (a dense layer's new-map sub-range; the transition down with max-unpooling) and with the
kEpiSumPool epilogue (transition up), bf16_dgrad_block_kernel, and the data-gradient branch of bf16_all_weights_kernel -- against the
plain operation in float64 on operands rounded exactly as the kernel rounds them (tests/bf16_backward_restate.py; never another kernel
of this library), for bf16 and for half storage.  The whole-network comparisons of test_gpu_bf16.py carry the tolerances 57 layers of
16-bit gradient storage force on them (1e-1 of a tensor's maximum); here a weight gradient is held to 6e-7 and a stored gradient to one
storage ulp.

Out of scope (no brick): bf16_prep_dy_kernel, bf16_bn_finalize_kernel / bf16_bn_finalize4_kernel and bf16_final_bwd_kernel.

Every call runs inside tests/guarded_alloc.py's guarded(): buffers are exactly as large as the contract says, with guard bands, and
scratch starts as NaN.  The bounds live in bf16_backward_restate.py (the host module's sensitivity checks are stated in them); the
measurements they come from are in the docstrings below: 3 x the worst value measured on an MI355X, rounded up to one digit."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import bf16_backward_restate as bbr
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
PREFIX = {"bf16": "endo_bf16_", "fp16": "endo_f16_"}
STORAGES = ["bf16", "fp16"]
SALT = 0x9E3779B1


def dev():
    return torch.device("cuda:0")


def fn(storage, name):
    return getattr(ea._lib.load(), PREFIX[storage] + name)


def gput(t, dtype=None):
    """a device copy of `t` in a buffer of exactly its size (guarded inside guarded())"""
    out = torch.empty(tuple(t.shape), dtype=dtype or t.dtype, device=dev())
    out.copy_(t)
    return out


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t


def pattern(count, scale=1.0):
    """a known, nonzero, non-NaN prefill"""
    return ((torch.arange(count, dtype=torch.float64) * 0.618033988749895) % 1.0 * 0.75 + 0.125) * scale


# ---------------------------------------------------------------------------------------------
# (a) weight gradient
# ---------------------------------------------------------------------------------------------
def run_wgrad(case, ops, storage, gscale=None, g_mult=1.0, short=0, zero_dw=False):
    """-> (rc, dw [cout][cin_w][ks][ks] fp64 = what the call added, untouched: everything around dw kept its bits)"""
    c = case
    dt = bbr.DTYPES[storage]
    n, h, w, ks, cin, cout = c["n"], c["h"], c["w"], c["ks"], c["cin"], c["cout"]
    cin_w = c["cin_w"] or cin
    with guarded():
        a = gput(bbr.to_blocked(ops["x"], c["a_blk"]), dt)
        g = gput(bbr.to_blocked(ops["g"] * g_mult, 32), dt)
        codes = gput(ops["codes"]) if c["codes"] else None
        saved = gput(ops["saved"]) if c["bn"] else None
        gamma = gput(ops["gamma"]) if c["bn"] else None
        beta = gput(ops["beta"]) if c["bn"] else None
        gs = gput(torch.tensor(gscale, dtype=torch.float32)) if gscale else None
        need = int(fn(storage, "wgrad_partial_floats")(n, h, w, cin, cout, ks))
        assert need == bbr.wgrad_partial_floats(n, h, w, cin, cout, ks)
        partial = torch.empty(need - short, dtype=torch.float32, device=dev())
        count, pad = cout * cin_w * ks * ks, 64
        fill = (pattern(count + 2 * pad) * (0.0 if zero_dw else 1.0)).float()
        if zero_dw:
            fill[:pad] = 1.0; fill[pad + count:] = 1.0
        dw = gput(fill)
        rc = fn(storage, "wgrad")(ptr(a), c["a_t"], c["a_blk"], c["ac0"], cin, c["cin_w"], c["ups"], ptr(saved), ptr(gamma), ptr(beta), c["rot"], c["rot_n"],
                                  n // c["groups"] if c["groups"] > 1 else 0, 2 * cin, ptr(g), c["g_t"], 32, c["gc0"], cout, ptr(codes), ptr(gs), ptr(partial),
                                  need - short, ctypes.c_void_p(dw.data_ptr() + 4 * pad), n, h, w, ks, None)
        torch.cuda.synchronize()
        got = dw.cpu()
    outside = torch.cat([got[:pad], got[pad + count:]])
    untouched = torch.equal(outside.view(torch.int32), torch.cat([fill[:pad], fill[pad + count:]]).view(torch.int32))
    return rc, got[pad:pad + count], (got[pad:pad + count].double() - fill[pad:pad + count].double()).reshape(cout, cin_w, ks, ks), untouched


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", bbr.WGRAD_CASES, ids=lambda c: c["name"])
def test_weight_gradient_against_fp64(case, storage):
    """endo_*_wgrad on the cases of bf16_backward_restate.WGRAD_CASES (their comments say what each is for and how many tiles its blocks
    walk) against torch autograd of F.conv2d in float64.  dw starts from a known pattern: the call accumulates and leaves everything
    around [cout][cin_w] bit-identical.
    Measured max err / max |ref| (MI355X), worst case of the list: bf16 1.32e-7 (dense_cin384_cout48_walk) -> bound 4e-7; half 1.78e-7
    (the same case) -> bound 6e-7.  The smallest: 5.1e-8 (grid_1x31).  (The whole-network tests hold the same tensors to 1e-1.)"""
    ops = bbr.make_wgrad_case(case, storage)
    ref = bbr.wgrad_reference(case, ops, storage)
    rc, _, got, untouched = run_wgrad(case, ops, storage)
    assert rc == 0, rc
    err = float((got - ref).abs().max() / ref.abs().max())
    blocks, tiles = bbr.wgrad_blocks(case["n"], case["h"], case["w"], case["cin"], case["cout"], case["ks"])
    print("wgrad %s %s (%d tiles / %d blocks): max err / max |ref| = %.2e" % (storage, case["name"], tiles, blocks, err))
    assert torch.isfinite(got).all()
    assert untouched, "the call wrote outside dw[cout][cin_w][ks][ks]"
    assert err <= bbr.WGRAD_BOUND[storage]


@pytest.mark.parametrize("name", ["dense_cin60_odd", "dense_cin384_cout48_walk", "td_96_codes"])
def test_half_gradient_scale_is_exact(name):
    """(d) half storage: G stored pre-multiplied by S = 2^6 with gscale = {S, 1 / S} gives the bits of the unscaled run (powers of two
    commute with every rounding of the sums).  Cases of at most 64 blocks and a zeroed dw: one fp32 atomic per element, no run-to-run order."""
    case = [c for c in bbr.WGRAD_CASES if c["name"] == name][0]
    ops = bbr.make_wgrad_case(case, "fp16")
    S = 64.0
    g = ops["g"]
    assert float(g.abs().max()) * S < 65504.0 and torch.equal(bbr.rnd(g * S, "fp16"), g * S)          # nothing overflows or loses bits when scaled
    assert float(g[g != 0].abs().min()) >= 2.0 ** -24 and bbr.wgrad_blocks(case["n"], case["h"], case["w"], case["cin"], case["cout"], case["ks"])[0] <= 64
    rc0, raw0, _, _ = run_wgrad(case, ops, "fp16", zero_dw=True)
    rc1, raw1, _, _ = run_wgrad(case, ops, "fp16", gscale=[S, 1.0 / S, 0.0, 0.0], g_mult=S, zero_dw=True)
    assert rc0 == 0 and rc1 == 0
    assert float(raw0.abs().max()) > 0
    assert torch.equal(raw0.view(torch.int32), raw1.view(torch.int32))


@pytest.mark.parametrize("storage", STORAGES)
def test_short_partial_workspace_is_refused(storage):
    """(e) a capacity one float short of the query: ENDO_E_BADARG, dw untouched"""
    case = bbr.WGRAD_CASES[0]
    ops = bbr.make_wgrad_case(case, storage)
    rc, _, added, untouched = run_wgrad(case, ops, storage, short=1)
    assert rc == -1
    assert untouched and float(added.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# the data-gradient weight layout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", [(12, 60, 3, 0, 0, 48, 12), (12, 228, 3, 48, 192, 192, 20), (12, 120, 3, 0, 0, 96, 8), (96, 96, 1, 0, 0, 0, 0), (48, 48, 3, 0, 0, 0, 0),
                                   (160, 160, 1, 0, 0, 0, 0)], ids=lambda s: "cout%d_cin%d_ks%d_rot%d_base%d_koff%d" % (s[0], s[1], s[2], s[3], s[5], s[6]))
def test_data_gradient_weight_layout(shape, storage):
    """endo_*_dgrad_weights (bf16_all_weights_kernel, dgrad = 1, one layer) against the layout restated from its contract, bit for bit:
    flipped taps, rot, and for rows below `base` the K offset and the LDS slot swizzle"""
    cout, cin, ks, rot, rot_n, base, koff = shape
    rng = np.random.default_rng(17)
    wt = torch.from_numpy(rng.standard_normal((cout, cin, ks, ks)).astype(np.float32))
    with guarded():
        out = torch.empty(int(fn(storage, "dgrad_weight_elems")(cout, cin, ks)), dtype=bbr.DTYPES[storage], device=dev())
        assert fn(storage, "dgrad_weights")(ptr(gput(wt)), cout, cin, ks, rot, rot_n, base, koff, ptr(out), None) == 0
        torch.cuda.synchronize()
        got = out.float().cpu().numpy()
    want = bbr.dgrad_weight_layout(bbr.rnd(wt, storage), rot, rot_n, base, koff)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# (b), (c) data gradients
# ---------------------------------------------------------------------------------------------
def run_dgrad(case, ops, storage):
    """-> (d after [n][t][..] fp32 planar, its bits, sums {layer: [groups][cin][2] = what was added}, sums_clean, g_clean)"""
    c = case
    dt = bbr.DTYPES[storage]
    n, h, w, groups = c["n"], c["h"], c["w"], c["groups"]
    layers = ops["layers"]
    tu = c["kind"] == "tu"
    with guarded():
        # one table region per group: the layers' (mean, rstd) / sums tables back to back, R floats / doubles per group
        offs, R = {}, 0
        for j, layer in layers.items():
            offs[j] = R
            R += 2 * (48 if tu else layer["cin"])
        stride = groups * R if c["slots"] else 0
        sums_fill = pattern((8 if c["slots"] else 1) * groups * R)
        sums = gput(sums_fill)
        wl, saved, gamma, beta = {}, None, {}, {}
        if not tu:
            saved = gput(torch.cat([torch.cat([layers[j]["saved"][g].reshape(-1) for j in layers]) for g in range(groups)]))
        for j, layer in layers.items():
            if c["kind"] in ("dense", "block"):
                args = (12, layer["cin"], 3, c["rot"], ops["rot_n"], c["c0"], bbr.KOFFS[j])
            elif c["kind"] == "td":
                args = (c["c"], c["c"], 1, 0, 0, 0, 0)
            else:
                args = (48, 48, 3, 0, 0, 0, 0)
            wl[j] = torch.empty(int(fn(storage, "dgrad_weight_elems")(*args[:3])), dtype=dt, device=dev())
            assert fn(storage, "dgrad_weights")(ptr(gput(layer["w"])), *args, ptr(wl[j]), None) == 0
            if not tu:
                gamma[j], beta[j] = gput(layer["gamma"]), gput(layer["beta"])
        group_n = n // groups if groups > 1 else 0
        d_shape = ops["d"].shape
        d = gput(bbr.to_blocked(ops["d"], 32), dt)
        d_fill = bits(d).clone()
        x = gput(bbr.to_blocked(ops["x"], 32), dt) if not tu else None
        g = gput(bbr.to_blocked(ops["g"], 32), dt) if "g" in ops else None
        g_fill = bits(g).clone() if g is not None else None
        codes = gput(ops["codes"]) if "codes" in ops else None

        def at(t, elems, size):
            return ctypes.c_void_p(t.data_ptr() + elems * size)

        if c["kind"] == "dense":
            j = c["j"]
            rc = fn(storage, "dgrad_bn")(ptr(d), ops["t"], 32, c["c0"] + 12 * j, 12, ptr(wl[j]), layers[j]["cin"], ptr(d), ptr(x), ops["t"], 32, c["c0"], 12 * j,
                                         ptr(saved), ptr(gamma[j]), ptr(beta[j]), c["rot"], ops["rot_n"], group_n, R, ptr(sums), R, stride, SALT, None, n, h, w, 3, None)
        elif c["kind"] == "td":
            rc = fn(storage, "dgrad_bn")(ptr(g), ops["g_t"], 32, 0, c["c"], ptr(wl[0]), c["c"], ptr(d), ptr(x), ops["t"], 32, 0, c["c"], ptr(saved), ptr(gamma[0]),
                                         ptr(beta[0]), 0, 0, group_n, R, ptr(sums), R, stride, SALT, ptr(codes), n, h, w, 1, None)
        elif tu:
            rc = fn(storage, "dgrad_sumpool")(ptr(g), ops["g_t"], 32, c["gc0"], 48, ptr(wl[0]), ptr(d), c["out_t"], 32, c["oc0"], 48, ptr(sums), SALT, n, h, w, None)
        else:
            four = lambda f: (ctypes.c_void_p * 4)(*[f(j).value for j in range(4)])
            rc = fn(storage, "dgrad_block")(ptr(d), ptr(x), ops["t"], 32, c["c0"], c["c0"], four(lambda j: ptr(wl[j])), four(lambda j: at(saved, offs[j], 4)),
                                            four(lambda j: ptr(gamma[j])), four(lambda j: ptr(beta[j])), four(lambda j: at(sums, offs[j], 8)), c["rot"], ops["rot_n"],
                                            group_n, R, R, stride, SALT, n, h, w, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        d_bits = bits(d).cpu()
        after = bbr.from_blocked(d.float().cpu(), d_shape[0], d_shape[1], d_shape[2], d_shape[3], 32)
        fill_planar = bbr.from_blocked(d_fill.cpu(), d_shape[0], d_shape[1], d_shape[2], d_shape[3], 32)
        bits_planar = bbr.from_blocked(d_bits, d_shape[0], d_shape[1], d_shape[2], d_shape[3], 32)
        g_clean = g is None or torch.equal(bits(g).cpu(), g_fill.cpu())
        got_sums = sums.cpu()
    slots = 8 if c["slots"] else 1
    added = (got_sums.reshape(slots, groups, R) - sums_fill.reshape(slots, groups, R)).sum(dim=0)          # the reader adds the copies up
    same = (got_sums.view(torch.int64) == sums_fill.view(torch.int64)).reshape(slots, groups, R).all(dim=0)
    out = {}
    for j, layer in layers.items():
        cin = 48 if tu else layer["cin"]
        out[j] = (added[:, offs[j]:offs[j] + 2 * cin].reshape(groups, cin, 2), same[:, offs[j]:offs[j] + 2 * cin].reshape(groups, cin, 2))
    return after, bits_planar, fill_planar, out, g_clean


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", bbr.DGRAD_CASES, ids=lambda c: "%s_%s" % (c["kind"], c["name"]))
def test_data_gradient_against_fp64(case, storage):
    """endo_*_dgrad_bn (dense new-map sub-range; transition down), endo_*_dgrad_sumpool and endo_*_dgrad_block against the header's own
    statement in float64: da = [x * sc + sh > 0] * dz, out += sc * da, sums += (sum da, sum da * x).  Per case:
      * every stored element within ONE storage ulp of the reference (exact for the stochastic rounding of pack_s16x2_sr) plus the fp32
        accumulation allowance DGRAD_ALLOW ulps at the magnitude of the accumulated terms;
      * the mean signed error over all stored elements at most 0.05 ulp, and so the mean error TOWARDS LARGER MAGNITUDES (a store that
        truncated the value shows -0.5 in the first, one that truncated the bits -0.5 in the second and 0 in the first);
      * the fp64 sums (the four layers' tables separately for the block kernel) within DGRAD_SUMS_BOUND of their maximum;
      * everything outside the written channels, the gradient read and the sums of other channels bit-identical to their prefill;
      * the same inputs give the same stored bits twice.
    Measured (MI355X), worst case of the list.  Largest |err|: bf16 0.998 ulp; half 1.000 ulp where the terms do not cancel and 9.8 of
    the element's own ulps where they cancel into the subnormal range (block_c96_rot).  Excess over one ulp in ulps of the magnitude:
    half 1.85e-5 (block_c288_groups) -> DGRAD_ALLOW 6e-5; bf16 0 in every case -> 8e-6 (the half figure in bf16 ulps, see
    bf16_backward_restate.py).  Mean signed error: at most 0.0053 ulp (bf16, tu_oc192_odd) and 0.0071 ulp (half, the same case).  Towards larger
    magnitudes: at most 0.0069 ulp (bf16, tu_oc288); with the dither removed from the bf16 store every bf16 case fails here (-0.5).
    Sums max err / max |ref|: bf16 1.54e-7 (tu_oc192_odd) -> 5e-7; half 2.01e-7 (dense_c96_j2_rot) -> 7e-7."""
    ops = bbr.make_dgrad_case(case, storage)
    chans, add, ref_sums, mag = bbr.dgrad_reference(case, ops, storage)
    after, after_bits, fill_bits, sums, g_clean = run_dgrad(case, ops, storage)
    old = ops["d"][:, chans].double()
    ref = old + add
    got = after[:, chans].double()
    assert got.numel() >= 10000
    assert torch.isfinite(got).all()
    u = bbr.ulp(ref, storage)
    err = got - ref
    excess = float(torch.clamp_min((err.abs() - u) / bbr.ulp(old.abs() + mag, storage), 0.0).max())
    mean_ulps = float((err / u).mean())
    mean_away = float((torch.sign(ref) * err / u).mean())          # towards larger magnitudes: a store that truncates the BITS moves towards zero
    worst_sums = 0.0
    for j, (added, same) in sums.items():
        lo = chans[0] if case["kind"] == "dense" else 0
        sl = slice(lo, lo + len(chans))
        worst_sums = max(worst_sums, float((added[:, sl] - ref_sums[j]).abs().max() / ref_sums[j].abs().max()))
        keep = torch.ones(added.shape[1], dtype=torch.bool); keep[sl] = False
        assert same[:, keep].all(), "sums of channels the launch does not own changed"
    print("dgrad %s %s_%s: max |err| %.3f ulp, excess over one ulp %.2e ulp(mag), mean signed err %+.4f ulp (away from zero %+.4f) over %d elements, sums max err / max |ref| = %.2e" % (
        storage, case["kind"], case["name"], float((err.abs() / u).max()), excess, mean_ulps, mean_away, got.numel(), worst_sums))
    other = torch.ones(after.shape[1], dtype=torch.bool); other[chans] = False
    assert torch.equal(after_bits[:, other], fill_bits[:, other]), "channels outside the written range changed"
    assert g_clean, "the gradient the launch reads changed"
    assert (err.abs() <= bbr.dgrad_tolerance(ref, old.abs() + mag, storage)).all(), float((err.abs() / u).max())
    assert abs(mean_ulps) <= 0.05 and abs(mean_away) <= 0.05
    assert worst_sums <= bbr.DGRAD_SUMS_BOUND[storage]
    _, again_bits, _, _, _ = run_dgrad(case, ops, storage)
    assert torch.equal(after_bits, again_bits), "the same inputs gave other bits"
