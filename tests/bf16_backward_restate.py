"""The backward kernels of the 16-bit-storage family restated as plain fp64 operations (test infrastructure, no library code):
operands rounded exactly where the kernels round them -- stored values, matrix-core weights and the staged relu(bn(x)) to the storage
type, (scale, shift) in fp32 -- and everything else (convolutions, sums, the BatchNorm / ReLU backward) in float64 through torch.
Shared by tests/test_bf16_backward_bricks_host.py (the helpers against autograd, the sensitivity of every case) and
tests/test_gpu_bf16_backward_bricks.py (the bricks against them).

Layouts: tensors here are PLANAR [n][channels][h][w]; to_blocked / from_blocked convert to the library's [n][t / blk][h][w][blk].
"""
import numpy as np
import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANTISSA = {"bf16": 7, "fp16": 10}          # explicit mantissa bits
MIN_EXP = {"bf16": -126, "fp16": -14}
KOFFS = (0, 12, 8, 20)                      # K window of layer j's base rows (bf16_dgrad_block_kernels.h)

# THE BOUNDS the GPU module holds the bricks to (tests/test_gpu_bf16_backward_bricks.py states the measurements next to them) -- here
# because the sensitivity checks of the host module are stated in terms of them
WGRAD_BOUND = {"bf16": 4e-7, "fp16": 6e-7}             # max |dw - ref| / max |ref|; measured 1.32e-7 / 1.78e-7
# fp32 accumulation noise per stored element, in storage ulps at the magnitude of the accumulated terms.  Half: measured 1.85e-5 (where the
# terms cancel into half's subnormal range an element is up to 9.8 of ITS ulps off).  bf16: no element was measured beyond one ulp
# (excess 0), so three times the measurement says nothing; the fp32 accumulation is the same arithmetic, a bf16 ulp is 8 half ulps:
# the half allowance / 8, rounded up.  Both are far below a quarter of an ulp.
DGRAD_ALLOW = {"bf16": 8e-6, "fp16": 6e-5}
DGRAD_SUMS_BOUND = {"bf16": 5e-7, "fp16": 7e-7}        # max |sums - ref| / max |ref| per table; measured 1.54e-7 / 2.01e-7


def dgrad_tolerance(ref, mag, storage):
    """per stored element: one storage ulp at the reference (exact for the stochastic rounding) + the allowance at the magnitude of the terms"""
    return ulp(ref, storage) + DGRAD_ALLOW[storage] * ulp(mag, storage)


# mirrors of bf16_bwd_kernels.h: the weight gradient's tile, channels per block, couts per 1 x 1 block
WG_ROWS, WG_COLS, WG_CO1 = 4, 32, 144


def rnd(t, storage):
    """fp32 -> storage type (round to nearest even) -> fp32"""
    return t.float().to(DTYPES[storage]).float()


def ulp(t, storage):
    """spacing of the storage type at |t| (float64 tensor)"""
    a = t.abs().double()
    e = torch.floor(torch.log2(torch.clamp_min(a, 2.0 ** MIN_EXP[storage])))
    e = torch.where(2.0 ** (e + 1) <= a, e + 1, torch.where(2.0 ** e > a, e - 1, e))          # log2 is not exact at powers of two
    return 2.0 ** (torch.clamp_min(e, MIN_EXP[storage]) - MANTISSA[storage])


def to_blocked(planar, blk):
    n, c, h, w = planar.shape
    blk = blk or c
    return planar.reshape(n, c // blk, blk, h, w).permute(0, 1, 3, 4, 2).contiguous()


def from_blocked(buf, n, c, h, w, blk):
    blk = blk or c
    return buf.reshape(n, c // blk, h, w, blk).permute(0, 1, 4, 2, 3).reshape(n, c, h, w)


def rot_index(c, rot, rot_n):
    """parameter index of buffer channel c (the up path keeps [skip | transition-up output] where the reference concatenates the other way)"""
    c = np.asarray(c)
    return np.where(c < rot_n, np.where(c + rot < rot_n, c + rot, c + rot - rot_n), c)


def scale_shift(saved, gamma, beta):
    """fp32 as the kernels compute them: sc = gamma * rstd, sh = fma(-mean, sc, beta); saved [c][2] = (mean, rstd)"""
    sc = gamma.float() * saved[:, 1].float()
    sh = (-saved[:, 0].double() * sc.double() + beta.double()).float()          # the product of two fp32 is exact in fp64: one rounding
    return sc, sh


def channel_tables(saved, gamma, beta, chans, rot, rot_n):
    """(sc, sh) of buffer channels `chans` of a layer, [groups][len(chans)] each; saved [groups][c][2]"""
    pc = torch.from_numpy(rot_index(np.asarray(chans), rot, rot_n).astype(np.int64))
    out = [scale_shift(saved[g], gamma, beta) for g in range(saved.shape[0])]
    return torch.stack([o[0][pc] for o in out]), torch.stack([o[1][pc] for o in out])


def per_sample(table, n, group_n):
    """[groups][c] -> [n][c][1][1]: sample i belongs to group i // group_n (group_n 0 = one group)"""
    idx = torch.tensor([(i // group_n if group_n > 0 else 0) for i in range(n)])
    return table[idx][:, :, None, None]


def staged_activation(x, sc, sh, storage):
    """relu(fma(x, sc, sh)) in fp32, rounded to the storage type; x planar, storage-rounded; sc, sh [n][c][1][1]"""
    z = (x.double() * sc.double() + sh.double()).float()
    return rnd(torch.clamp_min(z, 0.0), storage).double()


def relu_mask(x, sc, sh):
    return (x.double() * sc.double() + sh.double()) > 0


def upsample2(a):
    """nearest x2, written out: out[y][x] = a[y >> 1][x >> 1]"""
    h, w = a.shape[-2] * 2, a.shape[-1] * 2
    return a[..., torch.arange(h) // 2, :][..., torch.arange(w) // 2]


def unpool2(g, codes):
    """max-unpooling: out[2 y + dy][2 x + dx] = g[y][x] where codes[y][x] == 2 dy + dx, else 0; g [n][c][h][w], codes [n][h][w][c]"""
    n, c, h, w = g.shape
    out = torch.zeros(n, c, 2 * h, 2 * w, dtype=g.dtype)
    cp = codes.permute(0, 3, 1, 2)
    for dy in range(2):
        for dx in range(2):
            out[:, :, dy::2, dx::2] = torch.where(cp == 2 * dy + dx, g, torch.zeros_like(g))
    return out


def sumpool2(z):
    return z[..., 0::2, 0::2] + z[..., 0::2, 1::2] + z[..., 1::2, 0::2] + z[..., 1::2, 1::2]


def conv_weight_grad(a, g, ks):
    """dW of y = conv2d(a, W, padding = ks // 2) for dL/dy = g, by autograd in float64"""
    wt = torch.zeros(g.shape[1], a.shape[1], ks, ks, dtype=torch.float64, device=a.device, requires_grad=True)
    (F.conv2d(a, wt, padding=ks // 2) * g).sum().backward()
    return wt.grad.detach()


def conv_data_grad(g, wt):
    """dL/da of y = conv2d(a, W, padding = ks // 2) for dL/dy = g: the transposed convolution, float64"""
    return F.conv_transpose2d(g, wt, padding=wt.shape[-1] // 2)


# ---------------------------------------------------------------------------------------------
# weight-gradient cases
# ---------------------------------------------------------------------------------------------
def wgrad_blocks(n, h, w, cin, cout, ks):
    """bf16_wgrad_blocks restated: (blocks of the walk, tiles)"""
    tiles = ((w + WG_COLS - 1) // WG_COLS) * ((h + WG_ROWS - 1) // WG_ROWS) * n
    ci_blk = 64 if ks == 3 else 192
    ci_groups = (cin + ci_blk - 1) // ci_blk
    co_groups = (cout + 15) // 16 if ks == 3 else (cout + WG_CO1 - 1) // WG_CO1
    blocks = max(1, (512 if ks == 3 else 256) // (ci_groups * co_groups))
    return min(blocks, tiles), tiles


def wgrad_partial_floats(n, h, w, cin, cout, ks):
    blocks, _ = wgrad_blocks(n, h, w, cin, cout, ks)
    co_groups = (cout + 15) // 16 if ks == 3 else (cout + WG_CO1 - 1) // WG_CO1
    return blocks * co_groups * 9 * 16 * ((cin + 15) // 16 * 16)


def wg(name, n, h, w, ks, a_t, ac0, cin, g_t, gc0, cout, bn=True, rot=0, rot_n=0, groups=1, ups=0, cin_w=0, codes=None, a_blk=32):
    return dict(name=name, n=n, h=h, w=w, ks=ks, a_t=a_t, ac0=ac0, cin=cin, g_t=g_t, gc0=gc0, cout=cout, bn=bn, rot=rot, rot_n=rot_n, groups=groups,
                ups=ups, cin_w=cin_w, codes=codes, a_blk=a_blk)


# tiles each block walks = tiles / blocks of wgrad_blocks (test_bf16_backward_bricks_host.py asserts the counts stated here)
WGRAD_CASES = [
    # a dense layer with BatchNorm, cin = 60 (7.5 units, 3.75 ci tiles), slices at nonzero offsets, partial tiles in both directions: 20 tiles, 20 blocks
    wg("dense_cin60_odd", 1, 37, 53, 3, 96, 8, 60, 96, 72, 12),
    # cin = 84 = 64 + 20: the second ci group is partial: 20 tiles, 20 blocks
    wg("dense_cin84_odd", 1, 37, 53, 3, 128, 16, 84, 128, 104, 12),
    # THE PIPELINED WALK: 6 ci groups x 3 co groups -> 28 blocks over 96 tiles: 3 or 4 tiles per block (96 = 3 * 28 + 12)
    wg("dense_cin384_cout48_walk", 2, 64, 96, 3, 384, 0, 384, 64, 8, 48),
    # its 1 x 1 analogue (pooled gradient with codes, two co groups): 4 ci groups x 2 co groups -> 32 blocks over 102 tiles: 3 or 4 tiles per block
    wg("td_cin768_cout160_walk", 2, 68, 96, 1, 768, 0, 768, 160, 0, 160, codes="random"),
    # 1 x 1 over a full-resolution gradient (the kernel's path without codes; the network never launches it): 20 tiles, 20 blocks
    wg("conv1x1_no_codes", 2, 20, 64, 1, 224, 8, 208, 96, 8, 48),
    # the up path: rot = 48, rot_n = skip + 48 = 192, cin = 216 > rot_n: channels below and above rot_n: 8 tiles, 8 blocks
    wg("up_rot48_cin216", 1, 16, 40, 3, 224, 0, 216, 256, 240, 12, rot=48, rot_n=192),
    # two sample groups with their own statistics, n = 2 and n = 4: 12 tiles / 12 blocks and 24 / 24
    wg("groups_n2", 2, 12, 36, 3, 64, 0, 60, 96, 60, 12, groups=2),
    wg("groups_n4", 4, 9, 33, 3, 64, 0, 60, 96, 60, 12, groups=2),
    # transition up: nearest x2 of the raw input, 48 -> 48, no table: 16 tiles, 16 blocks
    wg("tu_48_48", 2, 16, 40, 3, 96, 48, 48, 192, 96, 48, bn=False, ups=1),
    # transition down: 1 x 1 over the pooled gradient with random codes, 96 -> 96: 24 tiles, 24 blocks
    wg("td_96_codes", 2, 24, 40, 1, 96, 0, 96, 96, 0, 96, codes="random"),
    # ... and with codes drawn so that all four positions occur among the channels of every window: 6 tiles, 6 blocks
    wg("td_96_codes_all4", 1, 10, 34, 1, 96, 0, 96, 128, 8, 96, codes="all4"),
    # the first convolution: 3 input channels travelling as 4 of an 8-channel record: 10 tiles, 10 blocks
    wg("first_cin3", 1, 20, 40, 3, 8, 0, 4, 64, 0, 48, bn=False, cin_w=3, a_blk=8),
] + [
    # grid sides around the tile (4 rows x 32 columns), the smallest grids on which the tile geometry can go wrong: 2 to 18 tiles,
    # one per block
    wg("grid_%dx%d" % (h, w), 2, h, w, 3, 32, 0, 20, 32, 4, 12) for h, w in ((1, 31), (3, 32), (4, 33), (5, 31), (31, 1), (32, 3), (33, 5), (4, 32))
]


def make_wgrad_case(case, storage, seed=11):
    """operands of a case (CPU tensors, planar): x storage-rounded [n][a_t][a_h][a_w], the tables, G [n][g_t][g_h][g_w], codes"""
    rng = np.random.default_rng(seed)
    c = case
    n, h, w = c["n"], c["h"], c["w"]
    a_h, a_w = (h // 2, w // 2) if c["ups"] else (h, w)
    g_h, g_w = (h // 2, w // 2) if c["codes"] else (h, w)
    ops = {"x": rnd(torch.from_numpy(rng.uniform(-1, 1, (n, c["a_t"], a_h, a_w)).astype(np.float32)), storage),
           "g": rnd(torch.from_numpy(rng.standard_normal((n, c["g_t"], g_h, g_w)).astype(np.float32)), storage)}
    if c["bn"]:
        cin = c["cin"]
        # different statistics per group; about half of relu's arguments positive
        ops["saved"] = torch.from_numpy(np.stack([rng.uniform(-0.3, 0.3, (c["groups"], cin)), rng.uniform(0.5, 1.5, (c["groups"], cin))], axis=2).astype(np.float32))
        ops["gamma"] = torch.from_numpy((rng.uniform(0.5, 1.5, cin) * rng.choice([-1, 1], cin)).astype(np.float32))
        ops["beta"] = torch.from_numpy(rng.uniform(-0.3, 0.3, cin).astype(np.float32))
    if c["codes"] == "random":
        ops["codes"] = torch.from_numpy(rng.integers(0, 4, (n, g_h, g_w, c["cout"])).astype(np.uint8))
    elif c["codes"] == "all4":          # channel k of a window takes position (k + a per-window offset) % 4
        off = rng.integers(0, 4, (n, g_h, g_w, 1))
        ops["codes"] = torch.from_numpy(((np.arange(c["cout"])[None, None, None, :] + off) % 4).astype(np.uint8))
    return ops


def wgrad_operands(case, ops, storage, perturb=None):
    """(a, G) of the convolution as float64 planar tensors on the h x w grid: a [n][cin], G [n][cout]"""
    c = case
    n, h, w = c["n"], c["h"], c["w"]
    x = ops["x"][:, c["ac0"]:c["ac0"] + c["cin"]]
    if c["bn"]:
        sc, sh = channel_tables(ops["saved"], ops["gamma"], ops["beta"], np.arange(c["cin"]), c["rot"], c["rot_n"])
        group_n = n // c["groups"] if c["groups"] > 1 else 0
        a = staged_activation(x, per_sample(sc, n, group_n), per_sample(sh, n, group_n), storage)
    else:
        a = x.double()
    if c["ups"]:
        a = upsample2(a)
    g = ops["g"][:, c["gc0"]:c["gc0"] + c["cout"]].double()
    if c["codes"]:
        codes = ops["codes"]
        if perturb == "code":
            codes = codes ^ 1          # the neighbouring position of the same row
        g = unpool2(g, codes)
    if perturb == "zero_row":          # the first row of the last tile
        y0, x0 = WG_ROWS * ((h - 1) // WG_ROWS), WG_COLS * ((w - 1) // WG_COLS)
        g = g.clone()
        g[n - 1, :, y0, x0:x0 + WG_COLS] = 0
    elif perturb == "shift_x":
        g = torch.cat([torch.zeros_like(g[..., :1]), g[..., :-1]], dim=-1)
    return a, g


def wgrad_reference(case, ops, storage, perturb=None, device="cpu"):
    """dw [cout][cin_w][ks][ks] float64 in PARAMETER order (buffer channel ci -> (ci + rot) % rot_n)"""
    a, g = wgrad_operands(case, ops, storage, perturb)
    dw_buf = conv_weight_grad(a.to(device), g.to(device), case["ks"]).cpu()
    dw = torch.zeros_like(dw_buf)
    dw[:, torch.from_numpy(rot_index(np.arange(case["cin"]), case["rot"], case["rot_n"]).astype(np.int64))] = dw_buf
    return dw[:, :(case["cin_w"] or case["cin"])]


# ---------------------------------------------------------------------------------------------
# data-gradient cases
# ---------------------------------------------------------------------------------------------
def up32(v):
    return (v + 31) // 32 * 32


def dg(kind, name, n, h, w, c0=0, j=0, rot=0, groups=1, slots=0, **kw):
    d = dict(kind=kind, name=name, n=n, h=h, w=w, c0=c0, j=j, rot=rot, groups=groups, slots=slots)
    d.update(kw)
    return d


# kind "dense": layer j of a block with c0 base channels with respect to its new maps [c0, c0 + 12 j) (rot on: rot = 48, rot_n = c0);
# "td": 1 x 1 with max-unpooling, c channels; "tu": 3 x 3 + 2 x 2 sum-pool into `oc0` of a coarser buffer; "block": four layers, base channels
DGRAD_CASES = [
    dg("dense", "c48_j1_odd", 1, 37, 53, c0=48, j=1),                     # one 16-row quad group live, partial tiles in both directions
    dg("dense", "c48_j3", 2, 16, 40, c0=48, j=3, slots=1),                # 36 new maps; the sums in eight copies
    dg("dense", "c96_j2_rot", 2, 17, 33, c0=96, j=2, rot=48),             # grp0 = 2 of 3 weight groups, an up-path block (rot_n = c0)
    dg("dense", "c288_j1", 1, 16, 56, c0=288, j=1),                       # grp0 = 6
    dg("dense", "c288_j3_groups", 2, 9, 35, c0=288, j=3, groups=2),       # two sample groups with their own statistics
    dg("td", "c96", 2, 24, 40, c=96),                                     # two groups of 48 rows, 3 K-chunks
    dg("td", "c144_groups", 2, 18, 34, c=144, groups=2, slots=1),         # partial tiles (the pooled grid is 9 x 17)
    dg("tu", "oc288", 2, 16, 40, gc0=240, oc0=288, out_t=352),            # the bottleneck's new maps receive the first transition up
    dg("tu", "oc192_odd", 1, 22, 54, gc0=96, oc0=192, out_t=288),         # partial tiles; pooled grid 11 x 27
    dg("block", "c48_odd", 1, 37, 53, c0=48),                             # grid.y = 1
    dg("block", "c96_rot", 2, 16, 20, c0=96, rot=48),                     # grid.y = 2, an up-path block
    dg("block", "c288_groups", 2, 8, 33, c0=288, groups=2, slots=1),      # grid.y = 6, two sample groups, the sums in eight copies
]
LAYER_SCALE = (1.0, 2.0, 0.5, 4.0)          # a different weight scale per layer: a K-window slip between layers does not cancel


def _tables(rng, groups, c):
    saved = torch.from_numpy(np.stack([rng.uniform(-0.3, 0.3, (groups, c)), rng.uniform(0.5, 1.5, (groups, c))], axis=2).astype(np.float32))
    gamma = torch.from_numpy((rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c)).astype(np.float32))
    beta = torch.from_numpy(rng.uniform(-0.3, 0.3, c).astype(np.float32))
    return saved, gamma, beta


def _weight(rng, cout, cin, ks, scale=1.0):
    return torch.from_numpy((rng.standard_normal((cout, cin, ks, ks)) * scale * (2.0 / (cout * ks * ks)) ** 0.5).astype(np.float32))


def make_dgrad_case(case, storage, seed=13):
    """operands (CPU, planar, storage-rounded): d = the gradient buffer(s) with every element prefilled, x the forward buffer, layers"""
    rng = np.random.default_rng(seed)
    c = case
    n, h, w = c["n"], c["h"], c["w"]

    def stored(*shape):
        return rnd(torch.from_numpy(rng.standard_normal(shape).astype(np.float32)), storage)

    ops = {}
    if c["kind"] in ("dense", "block"):
        c0 = c["c0"]
        t = up32(c0 + 48)
        ops["t"] = t
        ops["d"] = stored(n, t, h, w)
        ops["x"] = rnd(torch.from_numpy(rng.uniform(-1, 1, (n, t, h, w)).astype(np.float32)), storage)
        ops["rot_n"] = c0 if c["rot"] else 0
        layers = range(4) if c["kind"] == "block" else [c["j"]]
        ops["layers"] = {}
        for j in layers:
            cin = c0 + 12 * j
            saved, gamma, beta = _tables(rng, c["groups"], cin)
            ops["layers"][j] = dict(cin=cin, w=_weight(rng, 12, cin, 3, LAYER_SCALE[j]), saved=saved, gamma=gamma, beta=beta)
    elif c["kind"] == "td":
        ch = c["c"]
        ops["t"] = up32(ch)
        ops["g_t"] = up32(ch) + 32
        ops["d"] = stored(n, ops["t"], h, w)
        ops["x"] = rnd(torch.from_numpy(rng.uniform(-1, 1, (n, ops["t"], h, w)).astype(np.float32)), storage)
        ops["g"] = stored(n, ops["g_t"], h // 2, w // 2)
        ops["codes"] = torch.from_numpy(rng.integers(0, 4, (n, h // 2, w // 2, ch)).astype(np.uint8))
        saved, gamma, beta = _tables(rng, c["groups"], ch)
        ops["layers"] = {0: dict(cin=ch, w=_weight(rng, ch, ch, 1), saved=saved, gamma=gamma, beta=beta)}
    else:
        ops["g_t"] = up32(c["gc0"] + 48)
        ops["g"] = stored(n, ops["g_t"], h, w)
        ops["d"] = stored(n, c["out_t"], h // 2, w // 2)
        ops["layers"] = {0: dict(cin=48, w=_weight(rng, 48, 48, 3))}
    return ops


def dgrad_reference(case, ops, storage, drop_tap=None):
    """What the launch adds, in float64.  Returns (chans, add [n][len(chans)][..] = what is added to those channels of d,
    sums {layer: [groups][len(chans)][2]}, mag = the magnitude the fp32 accumulation works at, same shape as add)"""
    c = case
    n = c["n"]
    group_n = n // c["groups"] if c["groups"] > 1 else 0
    gidx = [(i // group_n if group_n > 0 else 0) for i in range(n)]

    def weights(layer):
        wt = rnd(layer["w"], storage).double()
        if drop_tap is not None:
            wt = wt.clone()
            wt[:, :, drop_tap // wt.shape[-1], drop_tap % wt.shape[-1]] = 0
        return wt

    def bn_backward(layer, dz, chans, rot, rot_n):
        """dz [n][len(chans)] at buffer channels chans -> (sc * da, sums [groups][len][2], sc * |dz| bound)"""
        x = ops["x"][:, chans].double()
        sc, sh = channel_tables(layer["saved"], layer["gamma"], layer["beta"], chans, rot, rot_n)
        scn, shn = per_sample(sc, n, group_n), per_sample(sh, n, group_n)
        da = torch.where(relu_mask(x, scn, shn), dz, torch.zeros_like(dz))
        sums = torch.zeros(c["groups"], len(chans), 2, dtype=torch.float64)
        for i in range(n):
            sums[gidx[i], :, 0] += da[i].sum(dim=(1, 2))
            sums[gidx[i], :, 1] += (da[i] * x[i]).sum(dim=(1, 2))
        return scn.double() * da, sums, scn.double().abs()

    if c["kind"] in ("dense", "block"):
        c0, rot, rot_n = c["c0"], c["rot"], ops["rot_n"]
        chans = np.arange(c0, c0 + 12 * c["j"]) if c["kind"] == "dense" else np.arange(c0)
        pc = torch.from_numpy(rot_index(chans, rot, rot_n).astype(np.int64))
        add = 0.0
        mag = 0.0
        sums = {}
        for j, layer in ops["layers"].items():
            g = ops["d"][:, c0 + 12 * j:c0 + 12 * j + 12].double()
            wt = weights(layer)
            dz = conv_data_grad(g, wt)[:, pc]
            term, sums[j], asc = bn_backward(layer, dz, chans, rot, rot_n)
            add = add + term
            mag = mag + asc * conv_data_grad(g.abs(), wt.abs())[:, pc]
        return chans, add, sums, mag
    if c["kind"] == "td":
        layer = ops["layers"][0]
        chans = np.arange(c["c"])
        g = unpool2(ops["g"][:, :c["c"]].double(), ops["codes"])
        wt = weights(layer)
        term, sums, asc = bn_backward(layer, conv_data_grad(g, wt), chans, 0, 0)
        return chans, term, {0: sums}, asc * conv_data_grad(g.abs(), wt.abs())
    layer = ops["layers"][0]
    chans = np.arange(c["oc0"], c["oc0"] + 48)
    g = ops["g"][:, c["gc0"]:c["gc0"] + 48].double()
    wt = weights(layer)
    add = sumpool2(conv_data_grad(g, wt))
    sums = torch.zeros(1, 48, 2, dtype=torch.float64)
    sums[0, :, 0] = add.sum(dim=(0, 2, 3))
    return chans, add, {0: sums}, sumpool2(conv_data_grad(g.abs(), wt.abs()))


# ---------------------------------------------------------------------------------------------
# the data-gradient weight layout (bf16_all_weights_kernel, dgrad = 1), restated from its contract
# ---------------------------------------------------------------------------------------------
def dgrad_weight_layout(wt, rot, rot_n, base, koff):
    """W [cout][cin][ks][ks] (already rounded) -> [chunk][group][tap][3][16 rows][32 k] as a flat fp32 array: row r = input channel
    (buffer order; parameter (r + rot) % rot_n), taps flipped; rows below `base`: output channel co at k = koff + co, and position p of
    the 32 holds k = ((p / 8) XOR (row16 >> 1) & 3) * 8 + p % 8; rows from `base` on: co at k = co, plain order"""
    cout, cin, ks, _ = wt.shape
    taps = ks * ks
    groups, chunks = (cin + 47) // 48, (cout + 31) // 32
    out = np.zeros((chunks, groups, taps, 3, 16, 32), dtype=np.float32)
    wn = wt.numpy().reshape(cout, cin, taps)
    for grp in range(groups):
        for t in range(3):
            for r16 in range(16):
                row = (grp * 3 + t) * 16 + r16
                if row >= cin:
                    continue
                pci = int(rot_index(row, rot, rot_n))
                for chunk in range(chunks):
                    for p in range(32):
                        k = chunk * 32 + p
                        if row < base:
                            k = (((p >> 3) ^ ((r16 >> 1) & 3)) << 3) | (p & 7)
                            k -= koff
                        if 0 <= k < cout:
                            out[chunk, grp, :, t, r16, p] = wn[k, pci, ::-1]
    return out.reshape(-1)
