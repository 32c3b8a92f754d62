"""Which kernel forms the fp64-compared tests run, against which forms the benchmark runs.  No GPU: the plan of a pass
(csrc/net.hip plan_fwd / plan_bwd) is asked through endo_net_plan_query on made-up aligned addresses.

plan_fwd / plan_bwd choose the kernel of every launch from the grid, the sample count, pointer alignment and the handle's
options.  A predicate or threshold that moves sends a layer to another kernel, and a parity test that forces options and says in
its docstring which kernel "takes" a shape stays green on whatever runs instead.  So:

  * FP64_CASES lists every (test, shape, groups, options, training) that a GPU test compares with the fp64 oracle; those tests take their
    parameters from it (cases / shapes below), so the table is what runs;
  * every (operand mode, kind, form, level) and every split-K slice count per level in the plans of bench.py's fp32-tensor
    configurations must be in the union of the table's plans (test_every_form_the_benchmark_takes_is_compared_with_fp64);
  * every value of every plan enum must be in that union or in NOT_COVERED with its reason, and nothing a benchmark plan
    contains may be listed there;
  * the default configuration's plan is pinned below as text: a change of form at the benchmark grid is a one-line diff.

The grids the fp64 oracle can afford are far smaller than the benchmark's, and several forms are chosen by how many tiles a launch has
(Subpix32x8 from 1024 tiles, Direct16x8 from 768).  ENDO_OPT_CHIP_DIVISOR = d (include/endo_hip.h) makes the plan count every tile d
times and gives the persistent launches 1 / d of the compute units: the added cases (tests/test_gpu_plan_forms.py) use it."""

import ast
import collections
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")

# ENDO_OPT_* (include/endo_hip.h)
WINO_FWD, WINO_DGRAD, DGRAD_VEC, WINO_MIN_TILES, MFMA_BF16, WGRAD_OVERLAP, WGRAD_F34, FINAL_VIRTUAL, TD_PERSIST, CHIP_DIVISOR = 0, 1, 2, 3, 4, 5, 7, 8, 9, 10

WINOGRAD = {WINO_MIN_TILES: 1, WINO_FWD: 1}
WINOGRAD4 = {WINO_MIN_TILES: 1, WINO_FWD: 5}
DIRECT = {WINO_FWD: 0, WINO_DGRAD: 0, DGRAD_VEC: 0, WGRAD_F34: 0}
NSPLIT = {WGRAD_F34: 0}
PLAIN = dict(list(DIRECT.items()) + [(FINAL_VIRTUAL, 0), (TD_PERSIST, 0)])          # every kernel form that has a switch, off

# shape = (samples per group, height, width); tag: the test's own name of the variant; takes: the (kind, form, level) entries -- or
# ("dense_fwd_ksplit", slices, level) -- the case exists for (asserted on the CPU here, and on the GPU from the pass's own plan before any
# comparison); x_offset: bytes the image tensor is moved off its 256-byte alignment
# backward: the test also differentiates the pass and compares gradients (else only the forward plan counts); beyond: what an added case is there
# for that (kind, form, level) cannot say (test_no_added_case_is_redundant)
Case = collections.namedtuple("Case", "test tag shape groups options training takes x_offset backward beyond")


def _case(test, tag, shape, groups=1, options=None, training=True, takes=(), x_offset=0, backward=True, beyond=""):
    return Case(test, tag, shape, groups, dict(options or {}), training, tuple(takes), x_offset, backward, beyond)


_PARITY = "test_gpu_parity."
_CONTRACT = "test_gpu_workspace_contract."
_FORMS = "test_gpu_plan_forms."

FP64_CASES = (
    [_case(_PARITY + "test_network_forward_levels", "train", s, backward=False) for s in ((2, 32, 32), (2, 64, 96), (1, 128, 160))] +
    [_case(_PARITY + "test_network_forward_levels", "eval", s, training=False, backward=False) for s in ((2, 32, 32), (2, 64, 96), (1, 128, 160))] +
    [_case(_PARITY + "test_network_backward", "", (2, 64, 96)),
     _case(_PARITY + "test_network_backward_eval_mode", "", (2, 64, 96), training=False)] +
    [_case(_PARITY + "test_network_backward_kernel_forms", tag, s, options=o)
     for tag, o in (("winograd", WINOGRAD), ("direct", DIRECT), ("winograd4", WINOGRAD4)) for s in ((2, 64, 96), (2, 128, 160), (1, 64, 128))] +
    [_case(_PARITY + "test_network_backward_kernel_forms", "nsplit", (2, 128, 256), options=NSPLIT,
           takes=[("dense_wgrad", "NSplit", 0), ("dense_wgrad", "Taps", 1)])] +
    [_case(_PARITY + "test_bf16_operand_mode_on_pattern", "", s, options={MFMA_BF16: 1}) for s in ((2, 64, 96), (2, 128, 160))] +
    [_case(_PARITY + "test_forward_pair_is_two_calls", "", s, groups=2) for s in ((2, 64, 96), (3, 32, 64))] +
    [_case(_PARITY + "test_network_backward_last_block_exact", "", s) for s in ((2, 64, 64), (2, 128, 160))] +
    [_case(_CONTRACT + "test_portrait_network_backward_on_pattern", tag, (2, 160, 96), options=o)
     for tag, o in (("default", {}), ("winograd", WINOGRAD), ("winograd4", WINOGRAD4), ("direct", PLAIN))] +
    [_case(_CONTRACT + "test_three_and_four_sample_groups", str(g), (2, 64, 96), groups=g) for g in (3, 4)]
)

# The cases this table gained so that the benchmark's forms are compared with fp64 (tests/test_gpu_plan_forms.py runs each: forward and backward in
# train mode, depth and all 210 gradients on the pass's own activation pattern).  Found with endo_net_plan_query; every one at or below 65 536
# pixel-samples.  d = ENDO_OPT_CHIP_DIVISOR.
ADDED_CASES = [
    # 2 x 8 x 256 x 320 (bench.py's default) as two groups of 1 x 128 x 192 with d = 27: every (kind, form, level) of that plan but F34 at level 4
    _case(_FORMS + "test_forms_against_fp64", "model-256x320", (1, 128, 192), groups=2, options={CHIP_DIVISOR: 27},
          takes=[("dense_fwd", "Wino4", 0), ("dense_fwd", "Wino2_32x8", 1), ("dense_fwd", "DirectAuto", 2), ("dense_fwd_ksplit", 3, 3),
                 ("tu_dgrad", "Subpix32x8", 0), ("tu_dgrad", "Subpix16x8", 1), ("base_pass", "Wino3Persistent", 0), ("newmap", "Persistent", 0),
                 ("td_fwd", "Persistent", 0), ("td_dgrad", "Persistent", 1), ("dense_wgrad", "F34", 3), ("first_wgrad", "F34Prep", 0)]),
    # 2 x 4 x 512 x 640 (--config 3) as two groups of 1 x 128 x 128 with d = 80: all of that plan but F34 at levels 4 and 5
    _case(_FORMS + "test_forms_against_fp64", "model-512x640", (1, 128, 128), groups=2, options={CHIP_DIVISOR: 80},
          takes=[("dense_fwd", "Wino4", 1), ("dense_fwd", "Direct16x8", 2), ("tu_dgrad", "Subpix32x8", 0), ("tu_dgrad", "Subpix16x4", 4),
                 ("block_bwd", "Fused", 5), ("td_dgrad", "Dma", 4)]),
    # F(3x3, 4x4) weight gradient at the two coarsest levels: h >> level must be a multiple of 16 -- narrow portrait grids reach that cheaply
    # (d = 40 at the first: the split-K slice counts of --config 3's two coarsest levels as well)
    _case(_FORMS + "test_forms_against_fp64", "f34-level-4", (1, 256, 64), options={CHIP_DIVISOR: 40},
          takes=[("dense_wgrad", "F34", 4), ("dense_fwd_ksplit", 5, 4), ("dense_fwd_ksplit", 6, 4), ("dense_fwd_ksplit", 9, 5), ("dense_fwd_ksplit", 11, 5)]),
    _case(_FORMS + "test_forms_against_fp64", "f34-level-5", (1, 512, 128), options={CHIP_DIVISOR: 64},
          takes=[("dense_wgrad", "F34", 5), ("dense_wgrad", "F34", 4)]),
    # F(2x2, 3x3) forward on 32 x 8 tiles over a level 48 wide (one and a half tiles) and the 16 x 8 direct kernel over one 24 wide
    _case(_FORMS + "test_forms_against_fp64", "partial-tiles", (2, 64, 96), options={CHIP_DIVISOR: 96},
          takes=[("dense_fwd", "Wino2_32x8", 1), ("dense_fwd", "Direct16x8", 2)],
          beyond="both forms over a partial last tile; the model grids' levels are whole tiles"),
    # (split-K: the fewest slices a benchmark plan holds, 3 at level 3, are in model-256x320; the most, 21 in the bottleneck's last layer, in every
    # case whose level 5 is one tile -- test_network_backward's for one)
    # forms the benchmark does not take, each behind an option or an alignment
    _case(_FORMS + "test_forms_against_fp64", "newmap-vec16", (2, 64, 96), options={DGRAD_VEC: 1}, takes=[("newmap", "Vec16", 0), ("newmap", "Vec16", 3)]),
    _case(_FORMS + "test_forms_against_fp64", "first-wgrad-f34", (2, 64, 96), options={FINAL_VIRTUAL: 0, WINO_MIN_TILES: 1},
          takes=[("first_wgrad", "F34", 0)]),
    _case(_FORMS + "test_forms_against_fp64", "first-wgrad-direct", (2, 64, 96), x_offset=4, takes=[("first_wgrad", "Direct", 0)]),
    _case(_FORMS + "test_forms_against_fp64", "direct-32x8", (2, 64, 96), options={WINO_FWD: 0, CHIP_DIVISOR: 64},
          takes=[("dense_fwd", "Direct32x8", 1)]),
    # bf16 operands (--config 5) at the default grid's forms: the bounds of test_bf16_operand_mode_on_pattern
    _case(_FORMS + "test_forms_against_fp64", "model-256x320-bf16", (1, 128, 192), groups=2, options={MFMA_BF16: 1, CHIP_DIVISOR: 27},
          takes=[("dense_fwd", "Direct32x8", 1), ("dense_wgrad", "NSplit", 0), ("dense_wgrad", "NSplit", 2), ("newmap", "Bf16", 0),
                 ("base_pass", "Block8Bf16", 4), ("tu_dgrad", "Subpix32x8", 0)]),
]
FP64_CASES = FP64_CASES + ADDED_CASES

# (kind, form): reason.  A plan-enum value no fp64 case takes may stand here only while no benchmark configuration's plan contains it.
NOT_COVERED = {}


def cases(test):
    """The table's cases of one test (module.name), in table order."""
    found = [c for c in FP64_CASES if c.test == test]
    assert found, test
    return found


def shapes(test):
    """The distinct shapes of a test's cases, in table order (for tests parametrised by shape alone)."""
    out = []
    for c in cases(test):
        if c.shape not in out:
            out.append(c.shape)
    return out


def case(test, tag, shape=None):
    found = [c for c in cases(test) if c.tag == tag and (shape is None or c.shape == tuple(shape))]
    assert len(found) == 1, (test, tag, shape)
    return found[0]


# ---------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------
def _library():
    if not os.path.exists(ea._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ea._lib.load()


def followed(entries):
    """Plan entries without those a per-layer block decides but does not follow (NEWMAP, BASE_PASS, WINO3_LAYOUT of a block that is not fused)."""
    fused = {index: value == "Fused" for kind, index, _, value in entries if kind == "block_bwd"}
    per_block = {"newmap": 4, "base_pass": 1, "wino3_layout": 1}
    return [e for e in entries if not (e[0] in per_block and not fused[e[1] // per_block[e[0]]])]


def forms_of(entries):
    """{(kind, form or number, level)} of a plan; the split-K slice counts only where the layer is split (0 elsewhere)."""
    # (the slice count is the launch's grid in y and the length of the reduction behind it, whatever the operands: see fp64_union)
    return {(kind, value, level) for kind, _, level, value in followed(entries) if not (kind == "dense_fwd_ksplit" and value == 0)}


def assert_takes(entries, takes, what):
    got = forms_of(entries)
    missing = [t for t in takes if tuple(t) not in got]
    assert not missing, "%s: the plan does not take %s; at those kinds it takes %s" % (
        what, missing, sorted(g for g in got if g[0] in {t[0] for t in missing} and not isinstance(g[1], int) or g[0] == "dense_fwd_ksplit"))


def plan_of_case(c):
    _library()
    n, h, w = c.shape
    entries = ea.models.plan_query(n * c.groups, h, w, c.groups, c.options, c.training, entries=True, x_offset=c.x_offset)
    return entries if c.backward else entries[:FWD_ENTRIES]


FWD_ENTRIES, BWD_ENTRIES = 145, 140          # fields of FwdPlan / BwdPlan (the query writes the forward plan first)


def mode_of(options):
    return "bf16" if options.get(MFMA_BF16) else "fp32"


def with_mode(mode, forms):
    """(operand mode, kind, form, level): a kernel's bf16-operand form is another kernel.  Split-K slice counts are kept under "fp32" for both."""
    return {("fp32" if f[0] == "dense_fwd_ksplit" else mode,) + f for f in forms}


def fp64_union(table=None):
    union = set()
    for c in (FP64_CASES if table is None else table):
        union |= with_mode(mode_of(c.options), forms_of(plan_of_case(c)))
    return union


def bench_configs():
    """{config: (samples per group, height, width, groups, options)} of bench.py's fp32-tensor configurations, read from its text (importing it
    would run its module-level set-up): CONFIGS, whose entries are dict(...) calls of literals.  A training step runs both frames of its pairs
    as one grouped pass (train_step.TrainingStep: forward_pair), so groups = 2; bf16_operands is ENDO_OPT_MFMA_BF16 = 1 (bench.py sets it so)."""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    (node,) = [n.value for n in tree.body if isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "CONFIGS" for t in n.targets)]
    out = {}
    for key, call in zip(node.keys, node.values):
        cfg = {kw.arg: ast.literal_eval(kw.value) for kw in call.keywords}
        if cfg.get("bf16_storage") or cfg.get("fp16_storage"):
            continue          # the 16-bit storage family has its own selection code (net16.hip)
        out[ast.literal_eval(key)] = (cfg["batch"], cfg["height"], cfg["width"], 2, {MFMA_BF16: 1} if cfg.get("bf16_operands") else {})
    return out


def bench_plans():
    _library()
    plans = {}
    for key, (n, h, w, groups, options) in bench_configs().items():
        plans[key] = (mode_of(options), ea.models.plan_query(n * groups, h, w, groups, options, True, entries=True))
    return plans


def dump(entries):
    """A plan as text: one line per (kind, level) with the forms of its entries in index order, runs of one form folded."""
    lines = collections.OrderedDict()
    for kind, index, level, value in followed(entries):
        lines.setdefault((kind, level), []).append(str(value))
    out = []
    for (kind, level), values in lines.items():
        folded = []
        for v in values:
            if folded and folded[-1][0] == v:
                folded[-1][1] += 1
            else:
                folded.append([v, 1])
        out.append("%-24s %-3s %s" % (kind, "" if level < 0 else "L%d" % level, " ".join(v if k == 1 else "%s*%d" % (v, k) for v, k in folded)))
    return "\n".join(out)


# ---------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------
def test_bench_configurations_are_read_from_bench_py():
    cfgs = bench_configs()
    assert cfgs[1] == (8, 256, 320, 2, {}) and cfgs[3] == (4, 512, 640, 2, {}) and cfgs[5] == (8, 256, 320, 2, {MFMA_BF16: 1})
    assert sorted(cfgs) == [1, 3, 5, 6] and cfgs[6] == cfgs[1]          # 6: the pose regime of configs[4] on the default grid


def test_the_query_and_the_names():
    lib = _library()
    names = {lib.endo_net_plan_name(k, -1) for k in range(27)}
    assert None not in names and len(names) == 27 and lib.endo_net_plan_name(27, -1) is None and lib.endo_net_plan_name(-1, 0) is None
    assert lib.endo_net_plan_name(0, 6) == b"DirectAuto" and lib.endo_net_plan_name(0, 7) is None and lib.endo_net_plan_name(1, 0) is None
    entries = ea.models.plan_query(2, 64, 96, entries=True)
    assert len(entries) == FWD_ENTRIES + BWD_ENTRIES and len({(k, i) for k, i, _, _ in entries}) == len(entries)
    # a handle that has run nothing has no last plan; a short buffer and a null pointer are argument errors, not overruns
    import ctypes
    hnd = ctypes.c_void_p()
    assert lib.endo_net_create_grouped(ctypes.byref(hnd), 2, 64, 96, 1) == 0
    try:
        raw = (ctypes.c_int32 * 1024)()
        a = [ctypes.c_void_p((i + 1) << 40) for i in range(6)]
        assert lib.endo_net_last_plan(hnd, 0, raw, 1024) == -1 and lib.endo_net_last_plan(hnd, 1, raw, 1024) == -1
        assert lib.endo_net_plan_query(hnd, 0, 1, a[0], a[1], a[2], a[3], a[4], a[5], raw, 1024) == 580
        assert lib.endo_net_plan_query(hnd, 1, 1, a[0], a[1], a[2], a[3], a[4], a[5], raw, 1024) == 560
        assert lib.endo_net_plan_query(hnd, 1, 1, a[0], a[1], a[2], a[3], a[4], a[5], raw, 559) == -1
        assert lib.endo_net_plan_query(hnd, 2, 1, a[0], a[1], a[2], a[3], a[4], a[5], raw, 1024) == -1
        assert lib.endo_net_plan_query(hnd, 1, 1, a[0], a[1], None, a[3], a[4], a[5], raw, 1024) == -1
        assert lib.endo_net_get_option(hnd, CHIP_DIVISOR) == 1
    finally:
        lib.endo_net_destroy(hnd)
    # the divisor at its default, and a value below one, change nothing
    assert ea.models.plan_query(2, 64, 96, options={CHIP_DIVISOR: 1}, entries=True) == entries
    assert ea.models.plan_query(2, 64, 96, options={CHIP_DIVISOR: 0}, entries=True) == entries


@pytest.mark.parametrize("c", [c for c in FP64_CASES if c.takes], ids=lambda c: "%s-%s" % (c.test.split(".")[-1], c.tag))
def test_each_case_takes_the_forms_it_exists_for(c):
    assert_takes(plan_of_case(c), c.takes, "%s %s %s" % (c.tag, c.shape, c.options))
    n, h, w = c.shape
    assert n * c.groups * h * w <= 65536, "the fp64 oracle at that size takes minutes"


def test_every_form_the_benchmark_takes_is_compared_with_fp64():
    union = fp64_union()
    for key, (mode, entries) in sorted(bench_plans().items()):
        want = with_mode(mode, forms_of(entries))
        missing = sorted(want - union, key=str)
        ksplit = collections.defaultdict(set)
        for kind, value, level in forms_of(entries):
            if kind == "dense_fwd_ksplit":
                ksplit[level].add(value)
        print("bench.py --config %d: split-K slices by level %s" % (key, {l: sorted(v) for l, v in sorted(ksplit.items())}))
        assert not missing, "bench.py --config %d runs (operands, kind, form, level) that no fp64-compared case runs: %s" % (key, missing)


@pytest.mark.parametrize("dropped", [c for c in ADDED_CASES if not c.beyond], ids=lambda c: c.tag)
def test_no_added_case_is_redundant(dropped):
    """Each added case is the only one that runs something the benchmark runs or an enum holds: without it test_every_form_the_benchmark_takes_is_compared_with_fp64
    or test_every_plan_enum_value_is_covered_or_listed fails and names it.  (A case that says what it is there for `beyond` the unit of this table -- a
    partial tile -- is neither asked this nor counted for the others.)"""
    union = fp64_union([c for c in FP64_CASES if c is not dropped and not c.beyond])
    wanted = set()
    for mode, entries in bench_plans().values():
        wanted |= with_mode(mode, forms_of(entries))
    lost = ((fp64_union([dropped]) & wanted) - union) | (enums_in(fp64_union([dropped])) - enums_in(union))
    print("only %s takes: %s" % (dropped.tag, sorted(lost, key=str)))
    assert lost, "nothing the benchmark runs and no enum value is lost without %s" % (dropped.tag,)


def enums_in(union):
    """(kind, form) of the enum values a union of plans compares with fp64: in fp32-operand mode -- a form's bf16-operand instantiation does not stand
    in for it -- but for the two forms that exist for bf16 operands only."""
    return {(kind, form) for mode, kind, form, _ in union if isinstance(form, str) and (mode == "fp32" or form.endswith("Bf16"))}


def enum_values():
    lib = _library()
    out = []
    for kind in range(27):
        value = 0
        while lib.endo_net_plan_name(kind, value) is not None:
            out.append((lib.endo_net_plan_name(kind, -1).decode(), lib.endo_net_plan_name(kind, value).decode()))
            value += 1
    return out


def test_every_plan_enum_value_is_covered_or_listed():
    covered = enums_in(fp64_union())
    in_bench = {(kind, form) for _, entries in bench_plans().values() for kind, form, _ in forms_of(entries)}
    values = enum_values()
    assert len(values) == 7 + 4 + 5 + 4 + 4 + 3 + 4 + 4 + 2 + 2 + 2 + 2
    for kv in values:
        assert (kv in covered) != (kv in NOT_COVERED), "%s.%s: %s" % (kv + ("neither compared with fp64 nor listed" if kv not in covered else "listed in NOT_COVERED but covered",))
    for kv, reason in NOT_COVERED.items():
        assert kv in values and reason, kv
        assert kv not in in_bench, "%s.%s is in a benchmark plan: it must be compared with fp64, not listed" % kv


# bench.py's default configuration, 2 groups of 8 x 256 x 320, every option at its default, torch-aligned buffers.  A line that changes here
# is a kernel that changed at the benchmark grid: say so in the pull request, and check that FP64_CASES still reaches the new form.
DEFAULT_PLAN = """\
dense_fwd                L0  Wino4*8
dense_fwd_ksplit         L0  0*8
dense_fwd_chunk_weights  L0  0*8
dense_fwd                L1  Wino2_32x8*8
dense_fwd_ksplit         L1  0*8
dense_fwd_chunk_weights  L1  0*8
dense_fwd                L2  DirectAuto*8
dense_fwd_ksplit         L2  0*8
dense_fwd_chunk_weights  L2  1*8
dense_fwd                L3  SplitK*8
dense_fwd_ksplit         L3  3*8
dense_fwd_chunk_weights  L3  1*8
dense_fwd                L4  SplitK*8
dense_fwd_ksplit         L4  8*2 6*2 7 8*3
dense_fwd_chunk_weights  L4  1*8
dense_fwd                L5  SplitK*4
dense_fwd_ksplit         L5  18 19 20 21
dense_fwd_chunk_weights  L5  1*4
fwd_bf16                     0
wino4_weights                1
fuse_final                   1
td_fwd                   L0  Persistent
tu_fwd                   L0  Subpix
td_fwd                   L1  Persistent
tu_fwd                   L1  Subpix
td_fwd                   L2  PerTile
tu_fwd                   L2  Subpix
td_fwd                   L3  PerTile
tu_fwd                   L3  Subpix
td_fwd                   L4  PerTile
tu_fwd                   L4  Upsample
block_bwd                L0  Fused*2
newmap                   L0  Persistent*6
base_pass                L0  Wino3Persistent*2
wino3_layout             L0  1*2
block_bwd                L1  Fused*2
newmap                   L1  Persistent*6
base_pass                L1  Wino3Persistent Wino3
wino3_layout             L1  1*2
block_bwd                L2  Fused*2
newmap                   L2  Persistent*6
base_pass                L2  Block8*2
wino3_layout             L2  0*2
block_bwd                L3  Fused*2
newmap                   L3  Persistent*6
base_pass                L3  Block8*2
wino3_layout             L3  0*2
block_bwd                L4  Fused*2
newmap                   L4  Persistent*6
base_pass                L4  Block8*2
wino3_layout             L4  0*2
block_bwd                L5  PerLayer
dense_wgrad              L0  F34*8
dense_wgrad              L1  F34*8
dense_wgrad              L2  F34*8
dense_wgrad              L3  F34*8
dense_wgrad              L4  F34*8
dense_wgrad              L5  Direct*4
td_wgrad                 L0  Dma
td_dgrad                 L0  Persistent
tu_wgrad                 L0  Subpix
tu_dgrad                 L0  Subpix32x8
td_wgrad                 L1  Dma
td_dgrad                 L1  Persistent
tu_wgrad                 L1  Subpix
tu_dgrad                 L1  Subpix16x8
td_wgrad                 L2  Dma
td_dgrad                 L2  Dma
tu_wgrad                 L2  Subpix
tu_dgrad                 L2  Subpix16x4
td_wgrad                 L3  Dma
td_dgrad                 L3  Dma
tu_wgrad                 L3  Subpix
tu_dgrad                 L3  Subpix16x4
td_wgrad                 L4  Plain
td_dgrad                 L4  Runs128
tu_wgrad                 L4  Taps
tu_dgrad                 L4  Plain
wgrad_overlap                1
bf16_wgrad                   0
bf16_dgrad                   0
dgrad_weights                1
use_virt                     1
virt_base                    1
virt_base_w                  1
materialise                  0
c_first                      144
first_wgrad              L0  F34Prep
"""


def test_the_default_configuration_plans_as_pinned():
    mode, entries = bench_plans()[1]
    assert dump(entries) + "\n" == DEFAULT_PLAN, "the plan at 2 x 8 x 256 x 320 changed:\n" + dump(entries)
