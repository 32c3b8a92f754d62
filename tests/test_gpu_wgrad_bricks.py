"""The fp32 weight-gradient kernels ONE BY ONE against fp64 (include/endo_hip.h, "WEIGHT-GRADIENT BRICKS"): each call is a single
weight-gradient launch of endo_net_bwd, made by the function the network itself switches over the forms in, on operands of the test's
own (tests/wgrad_restate.py: seeded normal x and G, BatchNorm tables per sample group, argmax codes), against autograd of F.conv2d in
float64 -- never another kernel of this library.  The whole-network tests hold the same tensors to GRAD_TOL = 3e-5 on operands other
kernels of the pass wrote.

Template instantiations covered (case lists and their edges: wgrad_restate.py; what each case is for is asserted on the CPU by
tests/test_wgrad_bricks_host.py):
    wgrad_f34_kernel<0, false, false> + wgrad_f34_reduce_kernel            dense F34 (segq 1 / 2 / 4, one unit .. three-unit walks)
    wgrad_f34_kernel<0, false, false> x 4 + wgrad_f34_reduce_batch_kernel   endo_wgrad_brick_f34_batch
    wgrad_f34_kernel<0, true, false> / <0, true, true>                      first convolution F34 / F34Prep (+ bias gradient)
    wgrad_nsplit_kernel<1> / <2> / <3> + wgrad_nsplit_reduce_kernel         dense NSplit (one and two channel passes)
    wgrad_taps_kernel<12, IN_BNRELU> / <12, IN_PLAIN> / <12, IN_UPSAMPLE>   dense / first / transition-up Taps
    wgrad_mfma_kernel<3, 1, IN_BNRELU, DY_PLAIN> / <3, 3, IN_PLAIN, DY_PLAIN> / <3, 1, IN_UPSAMPLE, DY_PLAIN>      Direct
    wgrad1x1_mfma_kernel                                                    transition-down Plain
    wgrad1x1_dma_kernel<0, 2, 2> / <0, 3, 1>                                transition-down Dma
    tu_wgrad_subpix_kernel + tu_wgrad_subpix_reduce_kernel                  transition-up Subpix
Deliberately without a brick: the bf16-operand forms (ENDO_OPT_MFMA_BF16: <.., BF = 1>), prep_dy_kernel, the bn_bwd_finalize kernels,
final_bwd_weight_kernel, and every forward and data-gradient kernel.

Every call runs inside tests/guarded_alloc.py's guarded(): buffers are exactly as large as the contract says, with guard bands; scratch
is NaN on entry (a partial-sum row no block wrote must never be read: f34_row_written); dw starts from a known pattern inside a padded
allocation and everything around it must keep its bits.  The bounds are wgrad_restate.BOUNDS: 4 x the distance of a plain fp32
evaluation of the same algorithm from float64 (measured on the CPU by the host test), not what the kernels give.

Measured max |err| / max |ref| on an MI355X, worst case per family (bound):
    f34       2.82e-6 first_16x32 F34Prep; dense 2.20e-6 f34_segq4_cin2052, batch 1.47e-6; the smallest 9.0e-7 f34_cin72_subrange  (2e-5)
    nsplit    2.26e-7 nsplit_three_chunks_per_block (2e-6)      taps    2.36e-7 tu_48_6x72 (2e-6)      direct  3.86e-7 tu_48_6x72 (2e-6)
    subpix    3.31e-7 tu_48_6x72 (2e-6)      td_plain  6.00e-7 td_96_64x40 (2e-6)      td_dma  5.64e-7 td_96_64x40 (2e-6)
    F34Prep's bias gradient 4.8e-8 of sum |G| (1.1e-5).  Between forms on shared operands: F34 against the others 1.8e-6 .. 1.9e-6, the
    others among themselves 1.4e-7 .. 5.3e-7 (atomics: the figures move by a few 1e-8 from run to run).
No case found a bug: every form passed on its first run."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import wgrad_restate as wr
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
PAD = 64          # floats of the prefill pattern on either side of dw
POINTERS = ("in", "dy", "saved", "gamma", "beta", "dy_idx", "prep_x", "prep_p", "prep_q", "prep_bias", "dw")


def dev():
    return torch.device("cuda:0")


def gput(array):
    """a device copy of a numpy array in a buffer of exactly its size (guarded inside guarded())"""
    t = torch.from_numpy(np.array(array))          # (a copy: the cases' arrays are read-only)
    out = torch.empty(tuple(t.shape), dtype=t.dtype, device=dev())
    out.copy_(t)
    return out


def pattern(count):
    """a known, nonzero, non-NaN prefill"""
    return (((torch.arange(count, dtype=torch.float64) * 0.618033988749895) % 1.0) * 0.75 + 0.125).float()


def c_operands(o):
    a = ea._lib.WgradOperands()
    for name, _ in a._fields_:
        key = "in" if name == "in_" else name
        setattr(a, name, (o[key] or None) if key in POINTERS else o[key])
    return a


class Staged(object):
    """a case's operands on the device: the buffers (kept alive), the operand record, dw and the bias prefill"""

    def __init__(self, c, form):
        ops = wr.make_case(c)
        g = ops["geometry"]
        self.c, self.count = c, c["cout"] * c["cin"] * wr.ksize(c) ** 2
        self.buffers = {key: gput(ops[key]) for key in ("in", "dy", "saved", "gamma", "beta", "prep_x", "prep_p", "prep_q") if key in ops}
        if "idx" in ops:
            self.buffers["dy_idx"] = gput(ops["idx"])
        self.fill = pattern(self.count + 2 * PAD)
        self.dw = gput(self.fill.numpy())
        ptrs = {key: t.data_ptr() for key, t in self.buffers.items()}
        ptrs["dw"] = self.dw.data_ptr() + 4 * PAD
        if form == "F34Prep":
            self.bias_fill = pattern(c["cout"] + 2 * PAD)
            self.bias = gput(self.bias_fill.numpy())
            ptrs["prep_bias"] = self.bias.data_ptr() + 4 * PAD
        self.o = wr.make_operands(c, g, ptrs)
        self.operands = c_operands(self.o)

    def result(self):
        """-> (dw as it is now, what the call added as float64 [cout][cin][ks][ks], everything around dw kept its bits)"""
        got = self.dw.cpu()
        ks = wr.ksize(self.c)
        around = torch.cat([got[:PAD], got[PAD + self.count:]]).view(torch.int32)
        kept = torch.equal(around, torch.cat([self.fill[:PAD], self.fill[PAD + self.count:]]).view(torch.int32))
        inner = got[PAD:PAD + self.count]
        return inner, (inner.double() - self.fill[PAD:PAD + self.count].double()).reshape(self.c["cout"], self.c["cin"], ks, ks), kept

    def bias_result(self):
        got = self.bias.cpu()
        n = self.c["cout"]
        around = torch.cat([got[:PAD], got[PAD + n:]]).view(torch.int32)
        kept = torch.equal(around, torch.cat([self.bias_fill[:PAD], self.bias_fill[PAD + n:]]).view(torch.int32))
        return got[PAD:PAD + n].double() - self.bias_fill[PAD:PAD + n].double(), kept


def run_brick(c, form, short=0, o_change=None):
    """one endo_wgrad_brick call -> (rc, Staged)"""
    lib = ea._lib.load()
    kind, index = c["kind"], wr.FORMS[c["kind"]].index(form)
    st = Staged(c, form)
    if o_change:
        st.o = dict(st.o, **o_change)
        st.operands = c_operands(st.o)
    need = int(lib.endo_wgrad_brick_scratch_floats(kind, index))
    assert need == wr.scratch_floats(kind, index)
    scratch = torch.empty(max(need - short, 1), dtype=torch.float32, device=dev()) if need else None          # NaN inside guarded()
    rc = lib.endo_wgrad_brick(kind, index, ctypes.byref(st.operands), ctypes.c_void_p(scratch.data_ptr()) if need else None, need - short, None)
    torch.cuda.synchronize()
    return rc, st


def check(c, form, st, what):
    ref = wr.reference(c, form)
    inner, got, kept = st.result()
    assert torch.isfinite(inner).all(), "%s: non-finite dW (a scratch row nobody wrote was read?)" % what
    err = wr.rel_err(got, ref["dw"])
    print("wgrad brick %-8s %-32s %-8s max err / max |ref| = %.2e (bound %.0e)" % (wr.FAMILY[(c["kind"], form)], c["name"], form, err, wr.bound(c["kind"], form)))
    assert kept, "%s: something around dw[cout][cin][ks][ks] changed" % what
    assert err <= wr.bound(c["kind"], form), what
    return got


@pytest.mark.parametrize("c,form", [(c, f) for c in wr.CASES for f in c["forms"]], ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_weight_gradient_against_fp64(c, form):
    """endo_wgrad_brick on every (case, form) of wgrad_restate.CASES.  dw starts from a known pattern: the call accumulates, leaves
    everything around it bit-identical, and (got - prefill) is within the form's bound of the float64 reference as max |err| / max |ref|;
    scratch starts as NaN and the result is finite.  F34Prep also gives the bias gradient, sum G."""
    with guarded():
        rc, st = run_brick(c, form)
        assert rc == 0, rc
        check(c, form, st, "%s %s" % (c["name"], form))
        if form == "F34Prep":
            ops = wr.make_case(c)
            lg = wr.logical(c, ops)
            gg = wr.gradient(c, ops, lg, form)
            got, kept = st.bias_result()
            err = float((got - wr.reference(c, form)["bias"]).abs().max() / np.abs(gg).sum(axis=(0, 2, 3)).max())
            bound = wr.bias_bound(c["n"] * c["h"] * c["w"])
            print("wgrad brick F34Prep bias gradient: max |err| / max sum |G| = %.2e (bound %.1e)" % (err, bound))
            assert kept and torch.isfinite(got).all()
            assert err <= bound


def test_f34_batch_of_four_layers():
    """four dense layers (cin 48, 60, 72, 84: 3, 4, 5, 6 channel groups) on one grid, each into its own NaN scratch slice, then ONE
    wgrad_f34_reduce_batch_kernel: gmax = 6, the blocks past a layer's own groups return early, every layer's dW within the F34 bound"""
    lib = ea._lib.load()
    with guarded():
        staged = [Staged(c, "F34") for c in wr.BATCH_CASE]
        layers = (ea._lib.WgradOperands * 4)(*[st.operands for st in staged])
        need = 4 * wr.K_F34_SCRATCH
        scratch = torch.empty(need, dtype=torch.float32, device=dev())
        assert lib.endo_wgrad_brick_f34_batch(layers, 4, ctypes.c_void_p(scratch.data_ptr()), need - 1, None) != 0          # one float short
        assert lib.endo_wgrad_brick_f34_batch(layers, 5, ctypes.c_void_p(scratch.data_ptr()), need, None) != 0
        rc = lib.endo_wgrad_brick_f34_batch(layers, 4, ctypes.c_void_p(scratch.data_ptr()), need, None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        for c, st in zip(wr.BATCH_CASE, staged):
            check(c, "F34", st, "batch layer %s" % c["name"])


@pytest.mark.parametrize("name", ["dense_shared_16x32_cin40", "first_16x32", "tu_48_6x72"])
def test_forms_agree_on_shared_operands(name):
    """the forms that accept the same operands compute the same function up to summation order: pairwise within the sum of their bounds
    (F34Prep forms its own gradient and stays out)"""
    c = next(k for k in wr.CASES if k["name"] == name)
    forms = [f for f in c["forms"] if f != "F34Prep"]
    assert len(forms) >= 3
    got = {}
    with guarded():
        for form in forms:
            rc, st = run_brick(c, form)
            assert rc == 0, (form, rc)
            got[form] = st.result()[1]
    scale = float(wr.reference(c)["dw"].abs().max())
    for i, a in enumerate(forms):
        for b in forms[i + 1:]:
            diff = float((got[a] - got[b]).abs().max()) / scale
            print("wgrad brick %s: %s against %s: %.2e" % (name, a, b, diff))
            assert diff <= wr.bound(c["kind"], a) + wr.bound(c["kind"], b)


def test_refusals_leave_dw_untouched():
    """a scratch capacity one float short, and a (form, shape) pair whose predicate is false: ENDO_E_BADARG with nothing launched"""
    shared = next(k for k in wr.CASES if k["name"] == "dense_shared_16x32_cin40")
    odd = next(k for k in wr.CASES if k["name"] == "direct_9x37_cin17")
    tu = wr.TU_CASES[0]
    with guarded():
        for c, form, kw in ((shared, "F34", {"short": 1}), (shared, "NSplit", {"short": 1}), (tu, "Subpix", {"short": 1}),
                            (odd, "F34", {}), (odd, "NSplit", {}), (odd, "Taps", {}),
                            (shared, "F34", {"o_change": {"h": 24}}), (shared, "Taps", {"o_change": {"saved": 0}}),
                            (shared, "Direct", {"o_change": {"group_n": 3}}), (shared, "Direct", {"o_change": {"n": 0}})):
            rc, st = run_brick(c, form, **kw)
            assert rc != 0, (c["name"], form, kw)
            inner, _, kept = st.result()
            assert kept and torch.equal(inner.view(torch.int32), st.fill[PAD:PAD + st.count].view(torch.int32)), (c["name"], form, kw)
