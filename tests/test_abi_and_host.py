"""CPU-only checks: the C-ABI library loads and exports every symbol include/endo_hip.h declares,
and the host-side mirror of the reference interface (module tree, state-dict keys, parameter
order, flat buffers, LR schedule, sharding) behaves.  No GPU compute is launched here."""

import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from oracle import network as onet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")


def header_functions():
    text = open(os.path.join(ROOT, "include", "endo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(endo_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(ea._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = header_functions()
    assert len(names) >= 30
    raw = ctypes.CDLL(ea._lib.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libendo_hip.so does not export %s" % name
    assert sorted(ea._lib.SIGNATURES) == names, "ctypes table and header disagree"
    lib = ea._lib.load()
    assert lib.endo_abi_version() == 7          # ENDO_ABI_VERSION of include/endo_hip.h
    assert lib.endo_net_param_floats() == 1374865
    assert lib.endo_net_bn_floats() == 21168
    assert b"bad argument" in lib.endo_error_string(-1)
    # argument validation happens before any device work
    assert lib.endo_depth_scale_fwd(None, None, None, None, None, None, 1, 1, 1e-8, None) == -1
    hnd = ctypes.c_void_p()
    assert lib.endo_net_create(ctypes.byref(hnd), 1, 30, 32) == -2          # not a multiple of 32
    assert lib.endo_net_create(ctypes.byref(hnd), 8, 256, 320) == 0
    assert lib.endo_net_tape_floats(hnd) > 8 * 192 * 256 * 320
    assert [lib.endo_net_level_channels(i) for i in range(6)] == [192, 240, 288, 336, 384, 336]
    lib.endo_net_destroy(hnd)


def test_module_tree_matches_reference_state_dict():
    model = ea.FCDenseNet57(n_classes=1)
    spec = onet.parameter_spec()
    sd = model.state_dict()
    assert list(sd.keys()) == [n for n, _, _ in spec]                       # 357 keys, reference order
    for name, shape, _ in spec:
        assert tuple(sd[name].shape) == tuple(shape), name
    assert [n for n, _ in model.named_parameters()] == onet.trainable_names()  # 210, .parameters() order
    lib = ea._lib.load()
    assert [lib.endo_net_param_offset(i) for i in range(210)] == model._offsets
    bn_off = 0
    for i, m in enumerate(model._bns):
        assert lib.endo_net_bn_offset(i, 0) == bn_off and lib.endo_net_bn_offset(i, 1) == bn_off + m.num_features
        bn_off += 2 * m.num_features


def test_both_families_place_batchnorms_by_one_table():
    """The saved (mean, rstd) pairs of BatchNorm i lie where the same table puts them in the fp32 tape (float offsets) and in the bf16 and
    half tapes (byte offsets), each from its handle's own start; index 49 is past the table for all three."""
    lib = ea._lib.load()
    hnd = ctypes.c_void_p()
    assert lib.endo_net_create(ctypes.byref(hnd), 2, 64, 96) == 0
    try:
        saved = [lib.endo_net_tape_offset(hnd, 1, i) for i in range(50)]          # ENDO_TAPE_BN_SAVED
        assert saved[49] == -1 and min(saved[:49]) >= 0
        for family in ("endo_net16", "endo_net16h"):
            h16 = ctypes.c_void_p()
            assert getattr(lib, family + "_create")(ctypes.byref(h16), 2, 64, 96, 1) == 0
            try:
                saved16 = [getattr(lib, family + "_offset")(h16, 1, i) for i in range(50)]
                assert saved16[49] == -1 and min(saved16[:49]) >= 0
                for i in range(49):
                    assert saved16[i] - saved16[0] == 4 * (saved[i] - saved[0]), (family, i)
            finally:
                getattr(lib, family + "_destroy")(h16)
    finally:
        lib.endo_net_destroy(hnd)


def test_flat_buffers_and_checkpoint_roundtrip(tmp_path):
    state = onet.perturb_affine(onet.synthetic_state(3), 4)
    model = ea.FCDenseNet57(1)
    model.load_state_dict(state)
    flat = model.flat_parameters()
    want = torch.cat([state[n].reshape(-1) for n in onet.trainable_names()])
    assert torch.equal(flat, want)
    assert model._views_intact()
    model.firstconv.weight.data.add_(1.0)                                   # views alias the flat buffer
    assert torch.equal(flat[:1296], want[:1296] + 1.0)
    grads = model.flat_gradients()
    assert all(p.grad is not None and p.grad.data_ptr() == grads.data_ptr() + 4 * o
               for p, o in zip(model.parameters(), model._offsets))
    torch.optim.SGD(model.parameters(), lr=0.1).zero_grad()                 # set_to_none=True
    assert model.firstconv.weight.grad is None
    assert model.flat_gradients().abs().sum() == 0 and model.firstconv.weight.grad is not None
    # reference wire format, 'module.'-prefixed keys (utils.py:674-682, train.py:197)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    path = tmp_path / "checkpoint_model_epoch_1_validation_0.5.pt"
    ea.utils.save_model(model, opt, 1, 10, path, 0.5)
    blob = torch.load(str(path))
    assert set(blob) == {"model", "optimizer", "epoch", "step", "validation"}
    assert all(k.startswith("module.") for k in blob["model"])
    other = ea.FCDenseNet57(1)
    ea.utils.load_model_state(other, blob["model"])
    assert torch.equal(other.flat_parameters(), model.flat_parameters())


def test_reference_written_checkpoint_loads(golden, tmp_path):
    """the checkpoint the REFERENCE wrote (its utils.save_model on its DataParallel-wrapped model and torch.optim.SGD after
    two iterations; tensors in tests/golden/checkpoint_2x64x96.npz) loads into FCDenseNet57 + FusedClipSGD, comes back out of
    state_dict() bit for bit in torch.optim.SGD's layout (which the stock optimizer accepts), and survives this repository's
    save_model / load_checkpoint.  The opposite direction -- a file written here loaded by the reference's modules -- needs the
    reference and is asserted by make_golden.py checkpoint_case in the build container.  The resumed ITERATION is the GPU test
    tests/test_gpu_parity.py::test_checkpoint_resume_matches_reference."""
    from conftest import checkpoint_from_fixture
    blob = checkpoint_from_fixture(golden("checkpoint_2x64x96.npz"))
    assert all(k.startswith("module.") for k in blob["model"]) and len(blob["model"]) == 357
    assert len(blob["optimizer"]["state"]) == 210 and blob["epoch"] == 1 and blob["step"] == 2
    model = ea.FCDenseNet57(1)
    res = ea.utils.load_model_state(model, blob["model"])
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in model.state_dict().items():
        assert torch.equal(v, blob["model"]["module." + k]), k
    opt = ea.optim.FusedClipSGD(model, lr=0.5)
    assert opt.state_dict()["state"] == {}                                   # no step yet: nothing to carry (torch.optim.SGD does the same)
    opt.load_state_dict(blob["optimizer"])
    assert opt.param_groups[0]["lr"] == blob["optimizer"]["param_groups"][0]["lr"] and opt.param_groups[0]["momentum"] == 0.9
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(210)) and sd["param_groups"][0]["params"] == list(range(210))
    for i, p in enumerate(model.parameters()):
        buf = sd["state"][i]["momentum_buffer"]
        assert buf.shape == p.shape and torch.equal(buf, blob["optimizer"]["state"][i]["momentum_buffer"]), i
    stock = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.5)
    stock.load_state_dict(sd)                                                # the reference's optimizer takes FusedClipSGD's dictionary as is
    assert stock.param_groups[0]["momentum"] == 0.9 and stock.param_groups[0]["nesterov"] is False
    for i, p in enumerate(model.parameters()):
        assert torch.equal(stock.state[p]["momentum_buffer"], blob["optimizer"]["state"][i]["momentum_buffer"])
    # a partial optimizer state is refused, not silently zero-filled
    broken = {"state": {i: v for i, v in blob["optimizer"]["state"].items() if i != 7}, "param_groups": blob["optimizer"]["param_groups"]}
    with pytest.raises(ValueError, match="209 of 210"):
        ea.optim.FusedClipSGD(model, lr=0.5).load_state_dict(broken)
    # file round trip through this repository's writer / reader
    path = tmp_path / "checkpoint_model_epoch_1_validation_0.5.pt"
    ea.utils.save_model(model, opt, blob["epoch"], blob["step"], path, blob["validation"])
    other = ea.FCDenseNet57(1)
    other_opt = ea.optim.FusedClipSGD(other, lr=0.5)
    back = ea.utils.load_checkpoint(path, other, other_opt)
    assert list(back["model"].keys()) == list(blob["model"].keys()) and (back["epoch"], back["step"], back["validation"]) == (1, 2, 0.5)
    assert torch.equal(other.flat_parameters(), model.flat_parameters()) and torch.equal(other_opt._momentum, opt._momentum)
    for k, v in other.state_dict().items():
        assert torch.equal(v, blob["model"]["module." + k]), k


def test_clean_point_list_refuses_hsv_frames():
    """reader.get_clean_point_list filters B, G, R bytes; the reference converts HSV frames back first (utils.py:362-363), which is not
    built here -- so the flag must fail loudly instead of filtering H, S, V as colours."""
    with pytest.raises(NotImplementedError, match="BGR"):
        ea.reader.get_clean_point_list(None, [[0, 0, 0, 1]], None, None, 0.99, None, None, is_hsv=True)


def test_no_cpu_fallback():
    model = ea.FCDenseNet57(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.DepthScalingLayer()([torch.ones(1, 1, 4, 4)] * 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.SparseMaskedL1Loss()([torch.ones(1, 2, 4, 4), torch.ones(1, 2, 4, 4), torch.ones(1, 1, 4, 4)])


def test_cyclic_lr_matches_reference(golden):
    dummy = torch.nn.Parameter(torch.zeros(1))
    for base, peak, size in ((1.0e-4, 1.0e-3, 2000), (1.0e-5, 6.0e-3, 7)):
        opt = torch.optim.SGD([dummy], lr=peak, momentum=0.9)
        sched = ea.scheduler.CyclicLR(opt, base_lr=base, max_lr=peak, step_size=size)
        for b, p, s, step, lr in golden("cyclic_lr.npz")["table"]:
            if (b, p, s) == (base, peak, size):
                sched.batch_step(batch_iteration=int(step))
                np.testing.assert_allclose(opt.param_groups[0]["lr"], lr, rtol=1e-12)
    with pytest.raises(TypeError):
        ea.scheduler.CyclicLR(object())


def test_kaiming_init_and_synthetic_batch():
    model = ea.FCDenseNet57(1)
    torch.manual_seed(10085)
    ea.utils.kaiming_weight_zero_bias(model, distribution="normal")
    w = model.denseBlocksUp[4].layers[3].conv.weight
    assert abs(float(w.std()) - (2.0 / (180 * 9)) ** 0.5) < 0.1 * (2.0 / (180 * 9)) ** 0.5
    assert float(model.finalConv.bias.abs().sum()) == 0 and float(model.transDownBlocks[0].norm.weight.min()) == 1
    batch = ea.synthetic.make_batch(2, 64, 96, seed=1)
    assert set(batch) == set(ea.synthetic.BATCH_KEYS)
    assert batch["colors_1"].shape == (2, 3, 64, 96) and batch["sparse_flows_2"].shape == (2, 2, 64, 96)
    assert 0.5 < float(ea.synthetic.boundary_mask(256, 320).mean()) < 0.65
    assert int(batch["sparse_depth_masks_1"][0].sum()) == 500
    r = batch["rotations_1_wrt_2"][0]
    assert torch.allclose(r @ batch["rotations_2_wrt_1"][0], torch.eye(3), atol=1e-6)


def test_shard_range():
    assert ea.distributed.shard_range(64, 3, 8) == (24, 32)
    with pytest.raises(ValueError):
        ea.distributed.shard_range(10, 0, 4)


def test_pair_selection_matches_reference(pkg, golden):
    """utils.generating_pos_and_increment against the table the reference produced under seeded ``random``
    (tests/golden/make_golden.py: pair_selection_case) -- the same draws in the same order, so the same pairs."""
    import random
    table = golden("pair_selection.npz")["table"]
    configs = []
    for row in table:
        key = tuple(int(v) for v in row[:4])
        if key not in configs:
            configs.append(key)
    for views, low, high, seed in configs:
        rows = [r for r in table if tuple(int(v) for v in r[:4]) == (views, low, high, seed)]
        visible = list(range(100, 100 + views))
        random.seed(seed)
        for r in rows:
            pos, inc = pkg.utils.generating_pos_and_increment(idx=int(r[4]), visible_view_indexes=visible, adjacent_range=(low, high))
            assert (pos, inc) == (int(r[5]), int(r[6])), (views, low, high, seed, int(r[4]))
            assert 0 <= pos + inc < views and (abs(inc) >= min(low, views // 2))


def test_oracle_relative_poses_identities():
    """oracle/poses.py (numpy restatement of dataset.py:384-399): R_2wrt1 R_1wrt2 = I, the translation round trip, and a
    hand-computed case (pure translation between two axis-aligned cameras)."""
    import numpy as np
    from oracle import poses
    rng = np.random.default_rng(3)

    def rigid():
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        e = np.eye(4)
        e[:3, :3] = q
        e[:3, 3] = rng.standard_normal(3)
        return e
    for _ in range(5):
        e1, e2 = rigid(), rigid()
        r12, r21, t12, t21 = poses.relative_poses(e1, e2, 2.5)
        assert r12.dtype == np.float32 and t21.shape == (3, 1)
        assert np.abs(r21 @ r12 - np.eye(3)).max() < 1e-6
        assert np.abs(r12 @ t21 + t12).max() < 1e-6
    e1, e2 = np.eye(4), np.eye(4)
    e1[:3, 3] = [1.0, 2.0, 3.0]
    r12, r21, t12, t21 = poses.relative_poses(e1, e2, 2.0)
    assert np.array_equal(r12, np.eye(3, dtype=np.float32)) and np.array_equal(t12.reshape(-1), np.float32([0.5, 1.0, 1.5]))
    assert np.array_equal(t21.reshape(-1), np.float32([-0.5, -1.0, -1.5]))
    mask = np.array([[0, 255, 229], [230, 128, 255]], dtype=np.uint8)
    assert np.array_equal(poses.boundary_plane(mask), np.float32([[0, 1, 0], [1, 0, 1]]))
