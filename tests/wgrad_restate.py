"""The fp32 weight-gradient kernels restated in plain torch / numpy, for the WEIGHT-GRADIENT BRICKS of include/endo_hip.h.

Nothing of the library is imported here and no kernel serves as a reference.  The module holds

  * the operation itself in float64 (``reference``: autograd of F.conv2d; ``reference_taps``: an explicit nine-tap sum over shifted
    windows, which also carries the MUTATIONS the host test uses to show that a case can see the mistake it exists for),
  * the host-side arithmetic of the launches (``f34_plan`` = wgrad_f34_plan, ``f34_block_count``, ``f34_row_written``, the grids of the
    other forms, the ``*_ok`` predicates), so that the case list can assert on the CPU what each case is for,
  * the case lists (every case names the edge it exists for),
  * the fp32 YARDSTICKS the bounds come from, and the bounds.

Layout of the operands (include/endo_hip.h, endo_wgrad_operands): planar fp32; sample s = group * group_n + nl; channel c of it at
base + group * gs + nl * ns + c * cs.  ``make_case`` builds every buffer exactly as large as that contract says and fills whatever lies
between the operands' planes (neighbouring channels of a wider buffer, the gap between two sample groups) with FILLER, a large finite
value: a kernel that reads one plane too many shows it in dW.
"""
import functools
import warnings

import numpy as np
import torch
import torch.nn.functional as F

GRAD_TOL = 3.0e-5          # the whole-network bound (tests/test_gpu_network.py): every brick bound must lie below it
FILLER = 3.0e4

DENSE, FIRST, TD, TU = 0, 1, 2, 3                                     # ENDO_WGRAD_*
FORMS = {DENSE: ["F34", "NSplit", "Taps", "Direct"], FIRST: ["F34Prep", "F34", "Taps", "Direct"], TD: ["Plain", "Dma"],
         TU: ["Subpix", "Taps", "Direct"]}                            # the enumerators of ENDO_PLAN_*_WGRAD, in order
K_F34_WAVES_PER_XCD = 256
K_F34_SCRATCH = 9 * 8 * K_F34_WAVES_PER_XCD * 256
K_NS_SCRATCH = 1024 * 12 * 7 * 256
K_SP_MAX_BLOCKS = 170
K_SP_SCRATCH = K_SP_MAX_BLOCKS * 3 * 27 * 256
MAX_GROUPS = 4


def scratch_floats(kind, form):
    name = FORMS[kind][form]
    if name in ("F34", "F34Prep"):
        return K_F34_SCRATCH
    if name == "NSplit":
        return K_NS_SCRATCH
    if name == "Subpix":
        return K_SP_SCRATCH
    return 0


# ---------------------------------------------------------------------------------------------
# host arithmetic of the launches
# ---------------------------------------------------------------------------------------------
def f34_block_count(plan, g):
    return (((g + 1) * plan["wpg"] - 1) >> 2) - ((g * plan["wpg"]) >> 2) + 1


def f34_first_block(plan, g):
    return (g * plan["wpg"]) >> 2


def f34_row_written(plan, g, slot):
    return slot % plan["spb"] < f34_block_count(plan, g)


def f34_plan(n, h, w, cin, cout=12, raw=False, waves_per_xcd=K_F34_WAVES_PER_XCD):
    """wgrad_f34_plan (csrc/wgrad_f34_kernels.h), its float arithmetic in fp32 as there"""
    f = np.float32
    plan = {"groups": cout // 12 if raw else (cin + 15) // 16}
    cy, s = h // 16, (w + 15) // 16
    best = f(1e30)
    for segq in (4, 2, 1):
        if cy % segq:
            continue
        per_xcd = (n * (cy // segq) * s + 7) // 8
        wpg = min(waves_per_xcd // plan["groups"], per_xcd)
        iters = (per_xcd + wpg - 1) // wpg
        cost = f(iters) * (f(4.0) * f(segq) + f(1.5))
        if cost < best * f(0.97):
            best, plan["segq"], plan["wpg"] = cost, segq, wpg
    plan["spb"] = max([1] + [f34_block_count(plan, g) for g in range(plan["groups"])])
    plan["slots"] = 8 * plan["spb"]
    plan["S"], plan["YS"] = s, cy // plan["segq"]
    plan["units"] = n * plan["YS"] * s
    plan["per_xcd"] = (plan["units"] + 7) // 8
    return plan


def f34_walks(plan):
    """the units every active wave walks: {(xcd, group, wq): [unit, ...]} as wgrad_f34_kernel numbers them (strip fastest)"""
    walks = {}
    for xcd in range(8):
        u_end = min(plan["units"], (xcd + 1) * plan["per_xcd"])
        for g in range(plan["groups"]):
            for wq in range(plan["wpg"]):
                walks[(xcd, g, wq)] = list(range(xcd * plan["per_xcd"] + wq, u_end, plan["wpg"]))
    return walks


def f34_unit_sample(plan, u):
    return u // plan["S"] // plan["YS"]


def f34_scratch_rows(plan):
    """(rows of 256 floats the launch may address, rows some block writes)"""
    total = plan["groups"] * 9 * plan["slots"]
    written = sum(9 for g in range(plan["groups"]) for slot in range(plan["slots"]) if f34_row_written(plan, g, slot))
    return total, written


def f34_mixed_blocks(plan):
    """blocks (of four waves) of an XCD whose waves belong to two channel groups"""
    total = plan["groups"] * plan["wpg"]
    return [b for b in range((total + 3) // 4) if len({(4 * b + k) // plan["wpg"] for k in range(4) if 4 * b + k < total}) > 1]


def nsplit_launch(n, h, w, cin):
    """launch_wgrad_nsplit: the NG instantiation, the channel passes and the block grid"""
    groups = (cin + 15) // 16
    passes = (groups + 11) // 12
    per_pass = (groups + passes - 1) // passes
    ng = min(3, max(1, (per_pass + 3) // 4))
    segs = (w + 31) // 32
    chunks = segs * h * n
    blocks = (512 if ng == 3 else 768 if ng == 2 else 1024) // passes
    per = (chunks + blocks - 1) // blocks
    blocks = (chunks + per - 1) // per
    return {"groups": groups, "passes": passes, "ng": ng, "segs": segs, "chunks": chunks, "blocks": blocks, "per": per,
            "scratch_rows": groups * 7 * blocks}


def taps_launch(n, h, w, cin, cout):
    tx, ty = (w + 31) // 32, (h + 7) // 8
    ci_chunks, co_sets, tiles = (cin + 15) // 16, (cout + 11) // 12, tx * ty * n
    groups = max(1, min(512 // (ci_chunks * co_sets), tiles))
    if groups >= 16:
        groups &= ~7
    return {"tiles_x": tx, "tiles_y": ty, "tiles": tiles, "ci_chunks": ci_chunks, "co_sets": co_sets, "groups": groups}


def direct_launch(n, h, w, cin, cout, q):
    tx, ty = (w + 31) // 32, (h + 7) // 8
    ci_chunks, co_sets, tiles = (cin + 15) // 16, (cout + 16 * q - 1) // (16 * q), tx * ty * n
    groups = max(1, min(1024 // (ci_chunks * co_sets), 384, tiles))
    return {"tiles_x": tx, "tiles_y": ty, "tiles": tiles, "ci_chunks": ci_chunks, "co_sets": co_sets, "groups": groups}


def td_dma_shape(cin, cout):
    """the (QO, QI) wave shape launch_wgrad1x1_dma chooses: the tiles that cover cout x cin with the fewer MFMAs"""
    def padded(to, ti):
        return (cout + to - 1) // to * to * ((cin + ti - 1) // ti) * ti
    return (2, 2) if padded(96, 96) <= padded(144, 48) else (3, 1)


def td_plain_launch(n, h, w, cin, cout):
    tiles_co, tiles_ci = (cout + 95) // 96, (cin + 95) // 96
    chunks = (h * w + 63) // 64 * n
    return {"tiles_co": tiles_co, "tiles_ci": tiles_ci, "chunks": chunks, "splits": max(1, min(768 // (tiles_co * tiles_ci), chunks))}


def subpix_launch(n, h, w):
    """launch_tu_wgrad_subpix on the LOW-resolution grid h x w"""
    segs = (w + 31) // 32
    chunks = segs * h * n
    blocks = min(K_SP_MAX_BLOCKS, chunks)
    per = (chunks + blocks - 1) // blocks
    return {"segs": segs, "chunks": chunks, "per": per, "blocks": (chunks + per - 1) // per}


# ---- the predicates (the kernels' *_ok without their tile / chunk minimum) on an operand record (make_operands) ----
def _al16(p):
    return p % 16 == 0


def f34_ok(o, cin=None, cout=None):
    cin, cout = cin or o["cin"], cout or o["cout"]
    aligned = o["w"] % 4 == 0 and o["h"] % 16 == 0 and o["dy_w"] % 4 == 0 and o["dy_cs"] % 4 == 0 and o["dy_ns"] % 4 == 0 and o["in_w"] % 4 == 0 \
        and o["in_cs"] % 4 == 0 and o["in_ns"] % 4 == 0 and _al16(o["dy"]) and _al16(o["in"])
    small = o["in_cs"] * (cin + 16) * 4 < 2 ** 31 and o["dy_cs"] * 12 * 4 < 2 ** 31
    return aligned and small and cout == 12 and cin >= 16 and (cin + 15) // 16 <= K_F34_WAVES_PER_XCD


def f34_raw_ok(o):
    return o["cin"] <= 16 and o["cout"] % 12 == 0 and o["cout"] // 12 <= 16 and o["in_cs"] * 32 * 4 < 2 ** 31 and f34_ok(o, 16, 12)


def nsplit_ok(o):
    return o["w"] % 4 == 0 and o["dy_w"] % 4 == 0 and o["dy_cs"] % 4 == 0 and o["dy_ns"] % 4 == 0 and o["in_w"] % 4 == 0 and o["in_cs"] % 4 == 0 \
        and o["in_ns"] % 4 == 0 and _al16(o["dy"]) and _al16(o["in"]) and o["cout"] == 12


def taps_ok(o, upsampled=False):
    dy_ok = o["w"] % 4 == 0 and o["dy_w"] % 4 == 0 and o["dy_cs"] % 4 == 0 and o["dy_ns"] % 4 == 0 and _al16(o["dy"])
    in_ok = upsampled or (o["in_w"] % 4 == 0 and o["in_cs"] % 4 == 0 and o["in_ns"] % 4 == 0 and _al16(o["in"]))
    return dy_ok and in_ok


def td_dma_ok(o):
    fits = (o["cin"] + 96) * o["in_cs"] * 4 < 2 ** 31 and (o["cout"] + 240) * o["dy_cs"] * 4 < 2 ** 31
    return fits and o["dy_w"] % 4 == 0 and o["dy_cs"] % 4 == 0 and o["dy_ns"] % 4 == 0 and o["idx_ns"] % 4 == 0 and o["h"] % 2 == 0 \
        and o["w"] == 2 * o["dy_w"] and o["in_w"] % 4 == 0 and o["in_cs"] % 4 == 0 and o["in_ns"] % 4 == 0 and o["gs"] % 4 == 0 and o["in_gs"] % 4 == 0 \
        and _al16(o["in"]) and _al16(o["dy"]) and o["dy_idx"] % 4 == 0


def subpix_ok(o):
    """on the LOW-resolution grid (w / 2)"""
    return o["cin"] == 48 and o["cout"] == 48 and (o["w"] // 2) % 4 == 0 and o["in_w"] % 4 == 0 and o["in_cs"] % 4 == 0 and o["in_ns"] % 4 == 0 \
        and o["dy_w"] % 8 == 0 and o["dy_cs"] % 4 == 0 and o["dy_ns"] % 4 == 0 and _al16(o["in"]) and _al16(o["dy"])


def operands_ok(kind, form, o):
    """sizes, strides and required pointers (brick_operands_ok of csrc/net.hip)"""
    if not (o["in"] and o["dy"] and o["dw"]) or min(o["n"], o["h"], o["w"], o["cin"], o["cout"]) <= 0 or o["group_n"] < 0:
        return False
    half_in, half_dy = kind == TU, kind == TD
    if (half_in or half_dy) and (o["h"] % 2 or o["w"] % 2):
        return False
    in_h, in_w = (o["h"] // 2, o["w"] // 2) if half_in else (o["h"], o["w"])
    dy_h, dy_w = (o["h"] // 2, o["w"] // 2) if half_dy else (o["h"], o["w"])
    if o["in_w"] < in_w or o["in_cs"] < in_h * o["in_w"] or o["in_ns"] < o["cin"] * o["in_cs"]:
        return False
    if o["dy_w"] < dy_w or o["dy_cs"] < dy_h * o["dy_w"] or o["dy_ns"] < o["cout"] * o["dy_cs"]:
        return False
    group_n = o["group_n"] or o["n"]
    if o["n"] % group_n or o["n"] // group_n > MAX_GROUPS:
        return False
    if o["n"] // group_n > 1 and (o["gs"] < group_n * o["dy_ns"] or o["in_gs"] < group_n * o["in_ns"]):
        return False
    if kind == DENSE and o["cout"] != 12:
        return False
    if kind == FIRST and (o["cin"] > 16 or o["cout"] % 12 or o["cout"] // 12 > 16):
        return False
    if kind in (DENSE, TD) and not (o["saved"] and o["gamma"] and o["beta"]):
        return False
    if kind == TD and (not o["dy_idx"] or o["idx_ns"] < o["cout"] * o["dy_cs"]):
        return False
    if kind == FIRST and FORMS[kind][form] == "F34Prep" and not (o["prep_x"] and o["prep_p"] and o["prep_q"]):
        return False
    return True


def brick_ok(kind, form, o):
    """endo_wgrad_brick_ok restated"""
    if not operands_ok(kind, form, o):
        return False
    name = FORMS[kind][form]
    if name == "Direct" or (kind == TD and name == "Plain"):
        return True
    if kind == DENSE:
        return {"F34": f34_ok, "NSplit": nsplit_ok, "Taps": taps_ok}[name](o)
    if kind == FIRST:
        return f34_raw_ok(o) if name in ("F34Prep", "F34") else taps_ok(o)
    if kind == TD:
        return td_dma_ok(o)
    return subpix_ok(o) if name == "Subpix" else taps_ok(o, True)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def case(name, kind, forms, n, h, w, cin, cout, why, group_n=0, pre=0, post=0, gs_extra=0, prep=False, edge=None, seed=None):
    """pre / post: channels of FILLER in front of / behind the operands' channels in both buffers (a sub-range of a wider buffer);
    gs_extra: floats of FILLER between two sample groups (with group_n); edge: the properties the host test asserts from the plan"""
    return {"name": name, "kind": kind, "forms": forms, "n": n, "h": h, "w": w, "cin": cin, "cout": cout, "why": why, "group_n": group_n,
            "pre": pre, "post": post, "gs_extra": gs_extra, "prep": prep, "edge": edge or {}, "seed": seed}


DENSE_CASES = [
    # the smallest launch the form accepts: ONE unit -- seven of eight XCDs and all but cin / 16 of the 2048 waves have no work, their scratch rows stay unwritten
    case("f34_minimum_1x16x16", DENSE, ["F34"], 1, 16, 16, 16, 12, "one unit", edge={"units": 1}),
    # w % 16 = 4: the last strip holds one tile column inside the image and three outside; cin % 16 = 12: the last channel group is 12 of 16
    case("f34_partial_strip_cin60", DENSE, ["F34"], 2, 32, 20, 60, 12, "last strip partly outside, last group 12 of 16", edge={"strip_rest": 4, "cin_rest": 12}),
    # cin % 16 = 4 and = 8 (with 12 above: every remainder a growth-12 block produces)
    case("f34_cin84", DENSE, ["F34"], 1, 32, 32, 84, 12, "cin % 16 == 4", edge={"cin_rest": 4}),
    case("f34_cin72_subrange", DENSE, ["F34"], 2, 16, 32, 72, 12, "cin % 16 == 8; operands inside wider buffers", pre=2, post=3, edge={"cin_rest": 8, "subrange": True}),
    # wpg % 4 != 0: blocks whose four waves belong to two channel groups (their sums meet in LDS and leave as two rows); and spb > 1
    case("f34_mixed_blocks_spb", DENSE, ["F34"], 3, 32, 48, 48, 12, "wpg not a multiple of 4, spb > 1", edge={"mixed": True, "spb": 2}),
    # a wave walks >= 3 units and crosses from sample group 0 into group 1 inside its walk: 24 channel groups (10 waves each per XCD), 2 x 2 samples
    # (170 units, 22 per XCD: XCD 3 owns units 66 .. 87 and sample 1 begins at unit 85; 80 x 260 is the smallest such grid of two samples)
    case("f34_walk_group_change", DENSE, ["F34"], 2, 80, 260, 384, 12, "walk of >= 3 units across a sample-group change", group_n=1, gs_extra=20,
         edge={"walk": 3, "group_change": True}),
    # segq = 2 and 4 (1: every other case).  The plan takes longer segments only where shorter ones would make a wave iterate more often, i.e. where
    # every wave of the chip has work: 129 channel groups leave ONE wave per group and XCD, and 8 (16) units of 2 (4) quads give each of them one
    case("f34_segq2_cin2052", DENSE, ["F34"], 2, 32, 64, 2052, 12, "segq == 2", edge={"segq": 2, "cin_rest": 4}),
    case("f34_segq4_cin2052", DENSE, ["F34"], 2, 64, 64, 2052, 12, "segq == 4", edge={"segq": 4, "cin_rest": 4}),
    # the four forms on the same operands (16 x 32: every predicate holds)
    case("dense_shared_16x32_cin40", DENSE, ["F34", "NSplit", "Taps", "Direct"], 2, 16, 32, 40, 12, "agreement between the forms; <12, IN_BNRELU>, <3, 1, IN_BNRELU>",
         group_n=1, gs_extra=12, edge={"segq": 1, "ng": 1}),
    # n-split: w = 40: the second 32-pixel chunk of a row is 8 pixels; h = 5; NG = 1 (cin <= 64); a grouped batch
    case("nsplit_w40_h5_ng1", DENSE, ["NSplit", "Taps", "Direct"], 2, 5, 40, 24, 12, "partial last chunk, odd height, NG = 1, grouped", group_n=1, gs_extra=8,
         edge={"ng": 1, "chunk_rest": 8, "taps_partial": True}),
    # 2112 chunks for 1024 blocks: every block owns three consecutive chunks (the two-chunks-ahead loads, the walk across rows and samples)
    case("nsplit_three_chunks_per_block", DENSE, ["NSplit"], 11, 64, 96, 24, 12, "blocks walk several chunks", edge={"ng": 1, "per": 3}),
    case("nsplit_ng2_cin84", DENSE, ["NSplit"], 1, 6, 36, 84, 12, "NG = 2 (cin 65 .. 128)", edge={"ng": 2}),
    case("nsplit_ng3_cin132", DENSE, ["NSplit"], 1, 4, 32, 132, 12, "NG = 3 (cin 129 .. 192)", edge={"ng": 3}),
    # 13 channel groups: two passes over the channels (gridDim.y = 2), 7 and 6 groups
    case("nsplit_two_passes_cin196", DENSE, ["NSplit"], 1, 4, 32, 196, 12, "several channel passes", edge={"passes": 2}),
    # a grid no other form accepts (w % 4 != 0), cin one past a multiple of the 16-channel chunk
    case("direct_9x37_cin17", DENSE, ["Direct"], 2, 9, 37, 17, 12, "odd grid, cin = 16 + 1; <3, 1, IN_BNRELU>", edge={"odd": True, "cin_rest": 1}),
    # taps: partial tiles in x and y (44 = 32 + 12, 11 = 8 + 3), cin % 16 = 4, more than one tile per block
    case("taps_11x44_cin20", DENSE, ["Taps"], 1, 11, 44, 20, 12, "partial tiles in x and y, cin % 16 == 4", edge={"taps_partial": True, "cin_rest": 4}),
]

# four layers of a dense block on one grid into four scratch slices + ONE batched reduction: 3, 4, 5, 6 channel groups
BATCH_CASE = [case("f34_batch_cin%d" % c, DENSE, ["F34"], 2, 16, 32, c, 12, "layer of the batched reduction", seed=100 + c) for c in (48, 60, 72, 84)]

FIRST_CASES = [
    # the network's first convolution, 3 -> 48 channels; two sample groups with their own P, Q for the fused preparation
    case("first_16x32", FIRST, ["F34Prep", "F34", "Taps", "Direct"], 2, 16, 32, 3, 48, "<0, RAW(, PREP)>, <12, IN_PLAIN>, <3, 3, IN_PLAIN>; bias gradient; two groups' P, Q",
         group_n=1, gs_extra=16, prep=True),
]

TD_CASES = [
    # 96 = one 96-tile of either kernel, (QO, QI) = (2, 2); pooled width 20: a multiple of 4 but not of 16 (the 16 code bytes of a piece run past the row's end)
    # 640 chunks for the 512 blocks of the Dma launch: a quarter of them walk two chunks (the second buffer, the strided walk); two groups of 5
    case("td_96_64x40", TD, ["Plain", "Dma"], 10, 64, 40, 96, 96, "QO x QI = 2 x 2; pooled width 20; grouped", group_n=5, gs_extra=24,
         edge={"shape": (2, 2), "pooled_w": 20, "dma_chunks_over": 512}),
    # 144 = one and a half 96-tiles of the plain kernel, (QO, QI) = (3, 1): 264 chunks for its 256 blocks; inside wider buffers
    case("td_144_16x24", TD, ["Plain", "Dma"], 33, 16, 24, 144, 144, "QO x QI = 3 x 1; 1.5 tiles of the plain kernel", pre=1, post=2,
         edge={"shape": (3, 1), "pooled_w": 12, "dma_chunks_over": 256}),
]

TU_CASES = [
    # low-resolution grid 3 x 36: a 4-pixel second chunk per row; 40 samples: 240 chunks for at most 170 blocks, so every block walks two
    # (and 120 tiles for the 42 blocks per channel slice of the taps kernel, the 113 of the direct one)
    case("tu_48_6x72", TU, ["Subpix", "Taps", "Direct"], 40, 6, 72, 48, 48, "partial last chunk, more chunks than blocks; <12, IN_UPSAMPLE>, <3, 1, IN_UPSAMPLE>",
         edge={"chunk_rest": 4, "per": 2}),
]

CASES = DENSE_CASES + FIRST_CASES + TD_CASES + TU_CASES


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
def geometry(c):
    """strides and buffer extents (floats) of a case: dict of in_* / dy_* / gs / in_gs / sizes / offsets"""
    kind, n, h, w = c["kind"], c["n"], c["h"], c["w"]
    in_h, in_w = (h // 2, w // 2) if kind == TU else (h, w)
    dy_h, dy_w = (h // 2, w // 2) if kind == TD else (h, w)
    group_n = c["group_n"] or n
    groups = n // group_n
    in_cs, dy_cs = in_h * in_w, dy_h * dy_w
    in_ns, dy_ns = (c["pre"] + c["cin"] + c["post"]) * in_cs, (c["pre"] + c["cout"] + c["post"]) * dy_cs
    gs = group_n * dy_ns + c["gs_extra"]
    in_gs = group_n * in_ns + c["gs_extra"]
    g = {"in_h": in_h, "in_w": in_w, "dy_h": dy_h, "dy_w": dy_w, "group_n": group_n, "groups": groups, "in_cs": in_cs, "dy_cs": dy_cs, "in_ns": in_ns,
         "dy_ns": dy_ns, "gs": gs, "in_gs": in_gs, "idx_ns": c["cout"] * dy_cs, "in_off": c["pre"] * in_cs, "dy_off": c["pre"] * dy_cs}
    g["in_len"] = g["in_off"] + (groups - 1) * in_gs + (group_n - 1) * in_ns + c["cin"] * in_cs
    g["dy_len"] = g["dy_off"] + (groups - 1) * gs + (group_n - 1) * dy_ns + c["cout"] * dy_cs
    g["saved_len"] = (groups - 1) * gs + 2 * c["cin"]
    g["pq_len"] = (groups - 1) * gs + c["cout"]
    g["idx_len"] = (groups - 1) * 4 * gs + (group_n - 1) * g["idx_ns"] + c["cout"] * dy_cs
    return g


def _positions(c, g, which):
    """flat index of element [s][ch][y][x] of operand `which` ('in' / 'dy') inside its buffer (from the operand pointer)"""
    chans, hh, ww = (c["cin"], g["in_h"], g["in_w"]) if which == "in" else (c["cout"], g["dy_h"], g["dy_w"])
    ns, cs, gstride = (g["in_ns"], g["in_cs"], g["in_gs"]) if which == "in" else (g["dy_ns"], g["dy_cs"], g["gs"])
    s = np.arange(c["n"])
    base = (s // g["group_n"]) * gstride + (s % g["group_n"]) * ns
    return (base[:, None, None, None] + np.arange(chans)[None, :, None, None] * cs + np.arange(hh)[None, None, :, None] * ww
            + np.arange(ww)[None, None, None, :])


@functools.lru_cache(maxsize=None)
def _make_case(name):
    c = next(k for k in CASES + BATCH_CASE if k["name"] == name)
    g = geometry(c)
    rng = np.random.default_rng(c["seed"] if c["seed"] is not None else sum(name.encode()))
    ops = {"geometry": g}

    def planar(which, length, off):
        sign = np.where(rng.random(length) < 0.5, -1.0, 1.0)
        buf = (FILLER * sign).astype(np.float32)
        pos = _positions(c, g, which) + off
        buf[pos] = rng.standard_normal(pos.shape).astype(np.float32)
        return buf
    ops["in"] = planar("in", g["in_len"], g["in_off"])
    ops["dy"] = planar("dy", g["dy_len"], g["dy_off"])
    if c["kind"] in (DENSE, TD):
        # tables with which about half the activations are positive, both signs of gamma, each group its own
        saved = np.full(g["saved_len"], FILLER, np.float32)
        for grp in range(g["groups"]):
            t = np.stack([0.3 * rng.standard_normal(c["cin"]), rng.uniform(0.5, 1.5, c["cin"])], 1).astype(np.float32)
            saved[grp * g["gs"]: grp * g["gs"] + 2 * c["cin"]] = t.reshape(-1)
        ops["saved"] = saved
        ops["gamma"] = (rng.uniform(0.5, 1.5, c["cin"]) * np.where(rng.random(c["cin"]) < 0.25, -1.0, 1.0)).astype(np.float32)
        ops["beta"] = (0.3 * rng.standard_normal(c["cin"])).astype(np.float32)
    if c["kind"] == TD:
        idx = np.full(g["idx_len"], 7, np.uint8)          # 7: no window position
        s = np.arange(c["n"])
        base = (s // g["group_n"]) * 4 * g["gs"] + (s % g["group_n"]) * g["idx_ns"]
        pos = base[:, None, None] + np.arange(c["cout"])[None, :, None] * g["dy_cs"] + np.arange(g["dy_cs"])[None, None, :]
        idx[pos] = rng.integers(0, 4, pos.shape).astype(np.uint8)
        ops["idx"], ops["idx_pos"] = idx, pos
    if c["prep"]:
        sign = np.where(rng.random(g["dy_len"]) < 0.5, -1.0, 1.0)
        px = (FILLER * sign).astype(np.float32)
        pos = _positions(c, g, "dy") + g["dy_off"]
        px[pos] = rng.standard_normal(pos.shape).astype(np.float32)
        ops["prep_x"] = px
        for key in ("prep_p", "prep_q"):
            t = np.full(g["pq_len"], FILLER, np.float32)
            for grp in range(g["groups"]):
                t[grp * g["gs"]: grp * g["gs"] + c["cout"]] = (0.5 * rng.standard_normal(c["cout"])).astype(np.float32)
            ops[key] = t
    for v in ops.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c, ops


def make_case(c):
    """-> the case's buffers (numpy, read-only, made once): in, dy, saved, gamma, beta, idx, prep_x, prep_p, prep_q, geometry"""
    return _make_case(c["name"])[1]


def make_operands(c, g, ptrs):
    """the endo_wgrad_operands record of a case as a dict; ptrs: {field: address} of the buffers' FIRST elements (0 = null)"""
    o = {"in": ptrs.get("in", 0) + 4 * g["in_off"] if ptrs.get("in") else 0, "dy": ptrs.get("dy", 0) + 4 * g["dy_off"] if ptrs.get("dy") else 0}
    for key in ("saved", "gamma", "beta", "dy_idx", "prep_x", "prep_p", "prep_q", "prep_bias", "dw"):
        o[key] = ptrs.get(key, 0)
    if o["prep_x"]:
        o["prep_x"] += 4 * g["dy_off"]
    o.update({"in_ns": g["in_ns"], "in_cs": g["in_cs"], "in_w": g["in_w"], "dy_ns": g["dy_ns"], "dy_cs": g["dy_cs"], "dy_w": g["dy_w"], "idx_ns": g["idx_ns"],
              "gs": g["gs"], "in_gs": g["in_gs"], "group_n": c["group_n"], "n": c["n"], "h": c["h"], "w": c["w"], "cin": c["cin"], "cout": c["cout"]})
    return o


# ---------------------------------------------------------------------------------------------
# the operation in float64
# ---------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 is exact in fp64; one rounding of the sum to fp64, one to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def logical(c, ops):
    """the operands as [n][channels][rows][cols] arrays read out of the buffers by the contract's strides"""
    g = ops["geometry"]
    out = {"x": ops["in"][_positions(c, g, "in") + g["in_off"]], "g": ops["dy"][_positions(c, g, "dy") + g["dy_off"]]}
    if c["kind"] == TD:
        out["codes"] = ops["idx"][ops["idx_pos"]].reshape(out["g"].shape)
    if c["prep"]:
        out["prep_x"] = ops["prep_x"][_positions(c, g, "dy") + g["dy_off"]]
    return out


def activation(c, ops, x, table_of_group=None):
    """a[n][cin][h][w] fp32 as the kernels state it; table_of_group: which group's BN table sample group g uses (a mutation)"""
    g = ops["geometry"]
    if c["kind"] in (DENSE, TD):
        a = np.empty_like(x)
        for grp in range(g["groups"]):
            t = grp if table_of_group is None else table_of_group[grp]
            saved = ops["saved"][t * g["gs"]: t * g["gs"] + 2 * c["cin"]].reshape(-1, 2)
            sc = (ops["gamma"] * saved[:, 1]).astype(np.float32)
            sh = _fma32(-saved[:, 0], sc, ops["beta"])
            sl = slice(grp * g["group_n"], (grp + 1) * g["group_n"])
            a[sl] = np.maximum(_fma32(x[sl], sc[None, :, None, None], sh[None, :, None, None]), np.float32(0))
        return a
    if c["kind"] == TU:
        return x.repeat(2, axis=2).repeat(2, axis=3)
    return x


def gradient(c, ops, lg, form=None, swap=None):
    """G[n][cout][h][w] float64 on the full grid: un-routed for the transition down (swap: (a, b) = codes a and b exchanged, a
    mutation), d + P x + Q for the first convolution's fused preparation"""
    g = ops["geometry"]
    gg = lg["g"].astype(np.float64)
    if c["kind"] == TD:
        codes = lg["codes"]
        if swap:
            codes = np.where(codes == swap[0], swap[1], np.where(codes == swap[1], swap[0], codes))
        full = np.zeros(gg.shape[:2] + (c["h"], c["w"]))
        for pos in range(4):
            full[:, :, pos >> 1::2, pos & 1::2] = np.where(codes == pos, gg, 0.0)
        return full
    if form == "F34Prep":
        for grp in range(g["groups"]):
            p = ops["prep_p"][grp * g["gs"]: grp * g["gs"] + c["cout"]].astype(np.float64)
            q = ops["prep_q"][grp * g["gs"]: grp * g["gs"] + c["cout"]].astype(np.float64)
            sl = slice(grp * g["group_n"], (grp + 1) * g["group_n"])
            gg[sl] += p[None, :, None, None] * lg["prep_x"][sl].astype(np.float64) + q[None, :, None, None]
    return gg


def conv_dw(a, gg, ks, dtype=torch.float64):
    """dW by autograd of F.conv2d.  On torch's own convolution path (unfold + GEMM): oneDNN splits the sum over pixels by the thread count, and
    its fp32 result moves by a factor 4 between 1, 8 and 16 threads -- no yardstick for a bound that must hold on every machine"""
    a = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    gg = torch.from_numpy(np.ascontiguousarray(gg)).to(dtype)
    wgt = torch.zeros(gg.shape[1], a.shape[1], ks, ks, dtype=dtype, requires_grad=True)
    threads = torch.get_num_threads()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the flags context announces what it knows about other devices)
        try:
            torch.set_num_threads(1)             # (the 1x1 case is one GEMM whose K the BLAS splits over its threads: 2.4e-7 .. 4.5e-7 with 8 .. 32)
            with torch.backends.mkldnn.flags(enabled=False):
                F.conv2d(a, wgt, padding=ks // 2).backward(gg)
        finally:
            torch.set_num_threads(threads)
    return wgt.grad.detach()


def taps_dw(a, gg, ks, halo_fix=None):
    """the same sum written out: one einsum per tap over the shifted window, float64.  halo_fix(ky, kx, window) may alter a window (mutations)"""
    a, gg = np.asarray(a, np.float64), np.asarray(gg, np.float64)
    n, cin, h, w = a.shape
    r = ks // 2
    pad = np.zeros((n, cin, h + 2 * r, w + 2 * r))
    pad[:, :, r:r + h, r:r + w] = a
    out = np.zeros((gg.shape[1], cin, ks, ks))
    for ky in range(ks):
        for kx in range(ks):
            win = pad[:, :, ky:ky + h, kx:kx + w]
            if halo_fix:
                win = halo_fix(ky, kx, win)
            out[:, :, ky, kx] = np.einsum("nchw,nohw->oc", win, gg, optimize=True)
    return torch.from_numpy(out)


def ksize(c):
    return 1 if c["kind"] == TD else 3


@functools.lru_cache(maxsize=None)
def _reference(name, form):
    c, ops = _make_case(name)
    lg = logical(c, ops)
    gg = gradient(c, ops, lg, form)
    out = {"dw": conv_dw(activation(c, ops, lg["x"]), gg, ksize(c))}
    if form == "F34Prep":
        out["bias"] = torch.from_numpy(gg.sum(axis=(0, 2, 3)))
    return out


def reference(c, form=None):
    """{'dw': [cout][cin][ks][ks] float64 (, 'bias': [cout])}; computed once per case (F34Prep has a gradient of its own)"""
    return _reference(c["name"], "F34Prep" if form == "F34Prep" else None)


# ---------------------------------------------------------------------------------------------
# fp32 yardsticks: a plain fp32 evaluation of the same algorithm on the same operands
# ---------------------------------------------------------------------------------------------
BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64)
# as the kernel has them: S without its row scales (1/4, -1/6, -1/6, 1/24, 1/24, 1: small integers, so S g S^T rounds as little as B^T d B does), the
# scales folded into the output transform C = A^T diag(scales)
S = np.array([[1, 0, 0, 0], [1, 1, 1, 1], [1, -1, 1, -1], [1, 2, 4, 8], [1, -2, 4, -8], [0, 0, 0, 1]], np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 1]], np.float64) * np.array([1 / 4, -1 / 6, -1 / 6, 1 / 24, 1 / 24, 1])[None, :]


def f34_tile_waves(plan, n, h, w):
    """[n][h / 4][w / 4]: which wave of its channel group (xcd * wpg + wq) works on every 4 x 4 tile (wgrad_f34_kernel's unit walk)"""
    ty, tx = np.arange(h // 4), np.arange(w // 4)
    unit = ((np.arange(n)[:, None, None] * plan["YS"] + (ty // (4 * plan["segq"]))[None, :, None]) * plan["S"] + (tx // 4)[None, None, :])
    xcd = unit // plan["per_xcd"]
    return xcd * plan["wpg"] + (unit - xcd * plan["per_xcd"]) % plan["wpg"]


def f34_dw(a, gg, dtype=np.float32, plan=None):
    """sum over waves of A^T [ sum over the wave's tiles (S g S^T) .* (B^T d B) ] A (csrc/wgrad_f34_kernels.h) in `dtype`: within a wave the
    36 products are accumulated over tiles BEFORE the output transform, every wave transforms its own sums, and the partial dW are added up
    (plan: f34_plan's; None: all tiles as one wave's)"""
    a, gg = np.asarray(a, dtype), np.asarray(gg, dtype)
    n, cin, h, w = a.shape
    cout = gg.shape[1]
    bt, s, at = BT.astype(dtype), S.astype(dtype), AT.astype(dtype)
    pad = np.zeros((n, cin, h + 2, w + 2), dtype)
    pad[:, :, 1:h + 1, 1:w + 1] = a
    ty, tx = h // 4, w // 4
    sn, sc, sy, sx = pad.strides
    d = np.lib.stride_tricks.as_strided(pad, (n, cin, ty, tx, 6, 6), (sn, sc, 4 * sy, 4 * sx, sy, sx))
    # both transforms as the kernel runs them: a column pass, its result rounded to `dtype`, then a row pass
    v = np.einsum("ij,nctujk->nctuik", bt, d).astype(dtype)
    v = np.einsum("nctuik,lk->ilcntu", v, bt).astype(dtype).reshape(6, 6, cin, -1)          # B^T d B            [6][6][cin][tiles]
    gt = gg.reshape(n, cout, ty, 4, tx, 4).transpose(0, 1, 2, 4, 3, 5)
    u = np.einsum("ij,notujk->notuik", s, gt).astype(dtype)
    u = np.einsum("notuik,lk->ilontu", u, s).astype(dtype).reshape(6, 6, cout, -1)          # S g S^T            [6][6][cout][tiles]
    waves = np.zeros(n * ty * tx, np.int64) if plan is None else f34_tile_waves(plan, n, h, w).reshape(-1)
    total = np.zeros((cout, cin, 3, 3), dtype)
    for wave in np.unique(waves):
        sel = np.nonzero(waves == wave)[0]
        m = np.matmul(u[:, :, :, sel], v[:, :, :, sel].transpose(0, 1, 3, 2))               # the GEMMs over the wave's tiles, accumulated in `dtype`
        out = np.einsum("ai,ijoc->ajoc", at, m).astype(dtype)
        total += np.einsum("ajoc,bj->ocab", out, at).astype(dtype)
    return torch.from_numpy(total.astype(np.float64))


def rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def yardstick(c, form):
    """distance from float64 of the fp32 evaluation that stands for `form` on case c"""
    ops = make_case(c)
    lg = logical(c, ops)
    a = activation(c, ops, lg["x"])
    gg = gradient(c, ops, lg, form).astype(np.float32)
    ref = reference(c, form)["dw"]
    if form in ("F34", "F34Prep"):
        return rel_err(f34_dw(a, gg, np.float32, f34_plan(c["n"], c["h"], c["w"], c["cin"], c["cout"], raw=c["kind"] == FIRST)), ref)
    return rel_err(conv_dw(a, gg, ksize(c), torch.float32), ref)


# YARDSTICKS: the worst distance over the cases of each form, measured by tests/test_wgrad_bricks_host.py (which checks these records
# against what it measures); BOUNDS = 4 x that (the margin for another fp32 summation order and for atomics -- what GRAD_TOL carries over
# its own measurement), rounded up to one digit.  Keys: the form families that share a kernel and therefore a bound.
FAMILY = {(DENSE, "F34"): "f34", (FIRST, "F34"): "f34", (FIRST, "F34Prep"): "f34", (DENSE, "NSplit"): "nsplit", (DENSE, "Taps"): "taps", (FIRST, "Taps"): "taps",
          (TU, "Taps"): "taps", (DENSE, "Direct"): "direct", (FIRST, "Direct"): "direct", (TU, "Direct"): "direct", (TD, "Plain"): "td_plain", (TD, "Dma"): "td_dma",
          (TU, "Subpix"): "subpix"}
#   f34       2.82e-6  first_16x32 F34Prep (f34_segq2_cin2052 2.76e-6, f34_segq4_cin2052 2.21e-6, f34_walk_group_change 1.52e-6, the others 1.0e-6 .. 2.3e-6) -> 2e-5
#             (with ONE output transform behind the sum over all tiles the three large cases are 5.1e-6 .. 6.0e-6 from float64: the 36 sums grow with
#             the tile count and cancel in A^T . A.  The kernel transforms every wave's own sums, and so does f34_dw)
#   nsplit    3.62e-7  nsplit_three_chunks_per_block                                                                                       -> 2e-6
#   taps / direct / subpix  4.81e-7  tu_48_6x72                                                                                          -> 2e-6
#   td_plain / td_dma       2.74e-7  td_96_64x40                                                                                         -> 2e-6
# (torch's own fp32 convolution path on one thread, conv_dw: the same figures on 1, 8 and 32 threads for the 3x3 cases)
YARDSTICKS = {"f34": 2.82e-6, "nsplit": 3.62e-7, "taps": 4.81e-7, "direct": 4.81e-7, "td_plain": 2.74e-7, "td_dma": 2.74e-7, "subpix": 4.81e-7}


def round_up_one_digit(v):
    e = int(np.floor(np.log10(v)))
    return float("%de%d" % (int(np.ceil(v / 10.0 ** e - 1e-9)), e))


BOUNDS = {k: round_up_one_digit(4.0 * v) if v > 0 else 0.0 for k, v in YARDSTICKS.items()}


def bias_bound(terms):
    """F34Prep's bias gradient, sum G over `terms` elements per channel, as |error| / sum |G|: every one of the ~ 2 * terms roundings (forming G,
    adding it) is at most 2^-24 of the running magnitude, which sum |G| bounds; independent roundings add up like a random walk -- sqrt(2 *
    terms) * 2^-24 -- and the same factor 4 as above covers the order of the additions"""
    return 4.0 * float(np.sqrt(2.0 * terms)) * 2.0 ** -24


def bound(kind, form):
    return BOUNDS[FAMILY[(kind, form)]]


# ---------------------------------------------------------------------------------------------
# mutations: the float64 operation with one mistake a kernel can make (tests/test_wgrad_bricks_host.py: every mutation moves the result
# by at least 10 x the form's bound on the case that exists for that edge)
# ---------------------------------------------------------------------------------------------
MUTATIONS = ["drop_tile", "drop_chunk", "right_columns", "halo_side", "group_table", "last_group_shift", "unpool_swap"]


def mutated(c, which, form=None):
    """dW float64 of case c with mutation `which`"""
    _, ops = _make_case(c["name"])
    lg = logical(c, ops)
    g = ops["geometry"]
    x = lg["x"]
    swap = (1, 2) if which == "unpool_swap" else None              # window position (0, 1) takes what belongs to (1, 0)
    gg = gradient(c, ops, lg, form, swap)
    table = [0] * g["groups"] if which == "group_table" else None  # every group evaluated with group 0's BatchNorm table
    a = activation(c, ops, x, table).astype(np.float64)
    fix = None
    w = c["w"]
    if which == "drop_tile":                                       # the last 4 x 4 tile of the last sample never added
        gg = gg.copy()
        gg[-1, :, -4:, (w - 1) // 4 * 4:] = 0.0
    elif which == "drop_chunk":                                    # the last 32-pixel chunk (row segment) of the last sample never added
        gg = gg.copy()
        gg[-1, :, -1, (w - 1) // 32 * 32:] = 0.0
    elif which == "right_columns":                                 # the column right of the image is what follows in memory: the next row's first pixel
        nxt = np.zeros(a.shape[:3])
        nxt[:, :, :-1] = a[:, :, 1:, 0]
        padded = np.zeros(a.shape[:2] + (a.shape[2] + 2,))
        padded[:, :, 1:-1] = nxt

        def fix(ky, kx, win):
            if kx != 2:
                return win
            win = win.copy()
            win[:, :, :, w - 1] = padded[:, :, ky:ky + a.shape[2]]
            return win
    elif which == "halo_side":                                     # the left halo column of the strip that begins at column 16 taken from its right side
        padded = np.zeros(a.shape[:2] + (a.shape[2] + 2,))
        padded[:, :, 1:-1] = a[:, :, :, 20]

        def fix(ky, kx, win):
            if kx != 0:
                return win
            win = win.copy()
            win[:, :, :, 16] = padded[:, :, ky:ky + a.shape[2]]
            return win
    elif which == "last_group_shift":                              # the last 16-channel group reads its planes one channel off
        c0 = (c["cin"] - 1) // 16 * 16
        a = a.copy()
        a[:, c0:] = np.roll(a[:, c0:], 1, axis=1)
    return taps_dw(a, gg, ksize(c), fix)


def batch_reduce_with(dw, cin_used):
    """a layer's dW [12][cin][3][3] as the batched reduction would scatter it with another layer's channel count `cin_used`"""
    cin = dw.shape[1]
    out = torch.zeros(dw.numel(), dtype=dw.dtype)
    for ci in range(min(cin, cin_used)):
        for co in range(12):
            base = (co * cin_used + ci) * 9
            if base + 9 <= out.numel():
                out[base:base + 9] += dw[co, ci].reshape(-1)
    return out.reshape(dw.shape)
