"""The similarity registration on the device (csrc/registration.hip under registration.py and evaluate.registration_errors) against the
numpy fp64 restatement tests/registration_restate.py: the nearest-neighbour search against brute force, ties, exact hits, the distance
cap, the 20 sums, the ICP loop on the fixture, and the posed evaluation outputs registered to a moved copy of themselves."""
import functools
import importlib

import numpy as np
import pytest
import torch

import registration_restate as rr
from test_gpu_evaluate import random_batch
from test_gpu_evaluate_posed import random_poses

pytestmark = pytest.mark.gpu

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
registration = ea.registration
evaluate = ea.evaluate

OFFSET = np.array([150.0, -80.0, 60.0])
MOVE = (1.1, rr.rotation_about((3.0, -1.0, 2.0), 11.0), np.array([0.7, -1.1, 0.4]))          # not the identity


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def rows_on_device(points, stride):
    """float32 rows at a row stride of 3 or 6 floats; the three extra columns hold colours that no result may depend on."""
    points = np.asarray(points, np.float32)
    if stride == 3:
        return torch.from_numpy(points.copy()).to(dev())
    full = np.concatenate([points, np.full((points.shape[0], 3), 200.0, np.float32)], axis=1)
    return torch.from_numpy(full).to(dev())


def tube(k, rng):
    u = rng.uniform(0.0, 2.0 * np.pi, k)
    z = rng.uniform(0.0, 12.0, k)
    r = 4.0 + 0.8 * np.sin(3.0 * u + 0.5 * z) + 0.5 * np.cos(u) * np.sin(0.9 * z) + 0.15 * z
    return (np.stack([r * np.cos(u), 1.3 * r * np.sin(u), z + 0.6 * np.sin(2.0 * u)], axis=1) + OFFSET).astype(np.float32)


@functools.lru_cache(maxsize=None)
def match_case(m, k):
    """A target on the fixture's tube and m source rows that, moved by MOVE, lie within ~0.3 of it; the brute-force fp64 squared
    distances, computed once per shape."""
    rng = np.random.default_rng(1000 * m + k)
    target = tube(k, rng)
    near = target[rng.integers(0, k, m)].astype(np.float64) + rng.normal(0.0, 0.3, (m, 3))
    scale, rot, tr = MOVE
    source = (((near - tr) @ rot) / scale).astype(np.float32)
    moved = rr.apply(source, scale, rot, tr)
    d2 = rr.squared_distances(moved, target)
    for a in (source, target, moved, d2):
        a.setflags(write=False)
    return source, target, moved, d2


def edge_sizes():
    wave, st, tt = registration.WAVE, registration.SOURCE_TILE, registration.TARGET_TILE
    return {"one": (1, 1), "below-wave": (wave - 1, wave + 1), "wave": (wave, wave), "above-wave": (wave + 1, wave - 1),
            "below-tiles": (st - 1, tt - 1), "tiles": (st, tt), "above-tiles": (st + 1, tt + 1), "source-tile-vs-one": (st + 1, 1),
            "one-vs-target-tile": (1, tt + 1), "300x1000": (300, 1000), "1000x4099": (1000, 4099)}


SIZE_NAMES = ("one", "below-wave", "wave", "above-wave", "below-tiles", "tiles", "above-tiles", "source-tile-vs-one", "one-vs-target-tile",
              "300x1000", "1000x4099")


@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("size", SIZE_NAMES)
def test_match_against_brute_force(size, stride):
    """index: d^2(i, j) <= min_k d^2(i, k) + 16 * 2^-24 * (|x_i| + max_k |t_k|)^2 with the norms of the centred coordinates (five
    roundings per fp32 score -- four fma steps and the stored |t|^2 --, two scores compared, a margin of 1.6).  distance: the fp64
    distance to row j rounded once to float32 (2^-24 relative), plus 1e-12 for the fp64 evaluation order of the moved point."""
    m, k = edge_sizes()[size]
    source, target, moved, d2 = match_case(m, k)
    scale, rot, tr = MOVE
    model = registration.TargetModel(rows_on_device(target, stride))
    out = registration.nearest_points(rows_on_device(source, stride), model, scale, rot, tr)
    index = out["index"].cpu().numpy()
    distance = out["distance"].cpu().numpy()
    assert index.dtype == np.int32 and index.shape == (m,) and distance.dtype == np.float32
    assert index.min() >= 0 and index.max() < k
    centre = target.astype(np.float64).mean(axis=0)
    assert np.abs(model.centre - centre).max() <= 1e-9
    reach = np.linalg.norm(moved - centre, axis=1) + np.linalg.norm(target.astype(np.float64) - centre, axis=1).max()
    chosen = d2[np.arange(m), index]
    excess = chosen - d2.min(axis=1)
    bound = 16.0 * 2.0 ** -24 * reach ** 2
    print("%s stride %d: wrong-index rows %d of %d, max excess / bound %.3g" % (size, stride, int((index != d2.argmin(axis=1)).sum()), m,
                                                                                float((excess / bound).max())))
    assert (excess <= bound).all()
    exact = np.sqrt(chosen)
    assert (np.abs(distance.astype(np.float64) - exact) <= 2.0 ** -24 * exact + 1e-12).all()
    assert out["count"] == m and abs(out["rms"] - np.sqrt(chosen.mean())) <= 1e-9 * np.sqrt(chosen.mean()) + 1e-12
    assert abs(out["max"] - exact.max()) <= 1e-9 * exact.max() + 1e-12


def lattice():
    """1100 points one unit apart (every coordinate a float32 number): far enough that no rounding of a score can change a winner."""
    g = np.stack(np.meshgrid(np.arange(10.0), np.arange(10.0), np.arange(11.0), indexing="ij"), axis=-1).reshape(-1, 3)
    return (g + OFFSET).astype(np.float32)


@pytest.mark.parametrize("stride", [3, 6])
def test_ties_go_to_the_lowest_index_and_exact_hits_have_distance_zero(stride):
    """Duplicated target rows score bit-identically; the duplicates sit in the same four rows of a lane, in another lane group of the
    same 16-row step, in a later step of the same update of the running minimum, in a later update and in a later target tile."""
    target = lattice()
    tt = registration.TARGET_TILE
    assert target.shape[0] > tt + 30
    for later, first in ((5, 4), (9, 2), (20, 3), (tt + 26, 7), (tt - 1, tt - 2), (tt, 13), (33, 32), (47, 32), (100, 40), (200, 199)):
        target[later] = target[first]
    first_of = {}
    expected = np.array([first_of.setdefault(tuple(row), i) for i, row in enumerate(target)])
    assert (expected != np.arange(target.shape[0])).sum() == 10
    out = registration.nearest_points(rows_on_device(target, stride), rows_on_device(target, stride))          # the identity
    assert np.array_equal(out["index"].cpu().numpy(), expected)
    assert (out["distance"].cpu().numpy() == 0.0).all() and out["max"] == 0.0 and out["count"] == target.shape[0]


def test_the_cap_selects_the_rows_of_the_sums_and_two_calls_give_the_same_bytes():
    """The sums against numpy fp64 on the device's own indexes: only the order of addition differs, so 1e-12 of the sum of the terms'
    absolute values (a sum about a centre has no scale of its own).  n and max exactly."""
    m, k = 1000, 4099
    source, target, moved, d2 = match_case(m, k)
    scale, rot, tr = MOVE
    model = registration.TargetModel(rows_on_device(target, 6))
    src = rows_on_device(source, 6)
    everything = registration.nearest_points(src, model, scale, rot, tr)
    index = everything["index"].cpu().numpy().astype(np.int64)
    exact = np.sqrt(d2[np.arange(m), index])
    order = np.sort(exact)
    for cap in (None, 0.5 * (order[m // 2] + order[m // 2 + 1]), 0.5 * (order[10] + order[11])):
        out = registration.nearest_points(src, model, scale, rot, tr, max_distance=cap)
        again = registration.nearest_points(src, model, scale, rot, tr, max_distance=cap)
        for key in ("index", "distance"):
            assert torch.equal(out[key], again[key]) and torch.equal(out[key], everything[key])
        assert out["sums"].tobytes() == again["sums"].tobytes()
        limit = np.inf if cap is None else cap
        source_centre = source.astype(np.float64).mean(axis=0)
        want = rr.sums_of(source, target, index, exact, limit, source_centre, model.centre)
        keep = exact <= limit
        s = np.abs(source.astype(np.float64)[keep] - source_centre)
        t = np.abs(target.astype(np.float64)[index[keep]] - model.centre)
        size = np.concatenate([[1.0, exact[keep].sum(), (exact[keep] ** 2).sum(), 0.0], s.sum(axis=0), t.sum(axis=0), [(s * s).sum()],
                               (t.T @ s).reshape(9)])
        assert out["sums"][0] == keep.sum() == out["count"] and (cap is None or 0 < out["count"] < m)
        assert abs(out["sums"][3] - exact[keep].max()) <= 1e-12 * exact[keep].max()
        assert (np.abs(out["sums"] - want) <= 1e-12 * size + 1e-300)[[1, 2] + list(range(4, 20))].all()


def test_a_cap_below_every_distance_keeps_nothing_and_register_raises():
    source, target, moved, d2 = match_case(300, 1000)
    scale, rot, tr = MOVE
    cap = 0.5 * float(np.sqrt(d2.min()))
    assert cap > 0.0
    model = registration.TargetModel(rows_on_device(target, 3))
    out = registration.nearest_points(rows_on_device(source, 3), model, scale, rot, tr, max_distance=cap)
    assert out["count"] == 0 and (out["sums"] == 0.0).all() and np.isnan(out["rms"])
    with pytest.raises(ValueError, match="0 are within"):
        registration.register(rows_on_device(source, 3), model, scale, rot, tr, max_distance=cap)


def mapped_rms(source, a, b):
    """Root mean square over the source rows of |T_a(s) - T_b(s)|: the error where the points are, not on the translation vector,
    which carries the rotation's lever arm to the origin."""
    return float(np.sqrt(((rr.apply(source, *a) - rr.apply(source, *b)) ** 2).sum(axis=1).mean()))


@pytest.mark.parametrize("junk", [0, 40])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_icp_recovers_the_fixture_without_noise(seed, junk):
    """From the identity.  The limit is the float32 storage of coordinates near 170: 4 * 2^-23 * max |coordinate|, about 8e-5."""
    source, target, truth = rr.fixture(seed, 0.0, junk)
    result = registration.register(torch.from_numpy(source).to(dev()), torch.from_numpy(target).to(dev()))
    error = mapped_rms(source, (result.scale, result.rotation, result.translation), truth)
    print("seed %d junk %d: %r, mapped-point rms error %.3g" % (seed, junk, result, error))
    assert result.converged and result.iterations <= 30 and len(result.history) == result.iterations
    assert result.count == 400 - junk
    assert error <= 4.0 * 2.0 ** -23 * max(np.abs(source).max(), np.abs(target).max())
    assert abs(np.linalg.det(result.rotation) - 1.0) <= 1e-12
    assert np.abs(result.matrix[:3, :3] - result.scale * result.rotation).max() == 0.0 and (result.matrix[3] == (0, 0, 0, 1)).all()
    assert tuple(result.index.shape) == (400,) and tuple(result.distance.shape) == (400,)


@pytest.mark.parametrize("junk", [0, 40])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_icp_follows_the_restatement_with_noise(seed, junk):
    """sigma = 0.02 on the same float32 inputs: the same correspondences leave only the fp64 order of addition, so the mapped points
    agree to 1e-6 (the CPU emulation of the matrix-unit score gave exactly 0) and the kept counts are equal."""
    source, target, _ = rr.fixture(seed, 0.02, junk)
    want = rr.register(source, target)
    result = registration.register(torch.from_numpy(source).to(dev()), registration.TargetModel(target))
    error = mapped_rms(source, (result.scale, result.rotation, result.translation), (want["scale"], want["rotation"], want["translation"]))
    print("seed %d junk %d: %r against %d iterations, count %d; mapped-point rms difference %.3g" % (
        seed, junk, result, want["iterations"], want["count"], error))
    assert result.converged and want["converged"]
    assert error <= 1e-6
    assert result.count == want["count"]
    assert abs(result.rms - want["rms"]) <= 1e-6


def test_the_rigid_fit_of_a_rigidly_moved_copy():
    _, target, _ = rr.fixture(3, 0.0, 0)
    rot, tr = rr.rotation_about((1.0, 2.0, 3.0), 6.0), np.array([0.3, -0.2, 0.4])
    ctr = target.astype(np.float64).mean(axis=0)
    source = ((target[::3].astype(np.float64) - ctr - tr) @ rot + ctr).astype(np.float32)
    truth = (1.0, rot, ctr + tr - rot @ ctr)
    result = registration.register(torch.from_numpy(source).to(dev()), torch.from_numpy(target).to(dev()), with_scale=False)
    error = mapped_rms(source, (result.scale, result.rotation, result.translation), truth)
    print("rigid: %r, mapped-point rms error %.3g" % (result, error))
    assert result.scale == 1.0 and result.converged and result.count == source.shape[0]
    assert error <= 4.0 * 2.0 ** -23 * np.abs(target).max()


def test_posed_outputs_registered_to_a_moved_copy_of_themselves():
    """posed_outputs_from_predictions on synthetic.smooth_depth at 2 x 32 x 40; the target is that cloud moved on the host by a known
    similarity; registration_errors, started beside it as the tracker's pose would, recovers it per frame and merged;
    endo_similarity_apply keeps the colour columns and gives numpy's fp64 result rounded once."""
    n, h, w = 2, 32, 40
    c, b, _, kk = random_batch(n, h, w, seed=5)
    pred = ea.synthetic.smooth_depth(n, h, w, seed=2).numpy()
    rot, tr = random_poses(n, 11)
    t = [torch.from_numpy(a).to(dev()) for a in (c, b, pred, kk)]
    out = evaluate.posed_outputs_from_predictions(*t, rot, tr)
    offsets = out["offsets"]
    total = offsets[-1]
    assert total > 500 and offsets[1] > 0 and offsets[2] > offsets[1]
    cloud = out["points"][:total]
    host = cloud.cpu().numpy()
    scale, rotation = 1.07, rr.rotation_about((0.5, 1.0, -0.3), 9.0)
    translation = np.array([12.0, -7.0, 3.0])
    truth = (scale, rotation, translation)
    target = rr.apply(host, *truth).astype(np.float32)
    middle = host[:, :3].astype(np.float64).mean(axis=0)
    nudge = rr.rotation_about((0.0, 0.0, 1.0), 0.05)          # a start beside the truth: 0.05 degrees about the cloud, 0.1 % in scale
    start_scale, start_rot = scale * 1.001, rotation @ nudge
    start = (start_scale, start_rot, scale * (rotation @ middle) + translation - start_scale * (start_rot @ middle) + 0.01)
    limit = 4.0 * 2.0 ** -23 * max(np.abs(host[:, :3]).max(), np.abs(target).max())
    model = registration.TargetModel(target)
    per_frame = evaluate.registration_errors(out["points"], offsets, model, initial=start)
    assert len(per_frame) == n
    for f, result in enumerate(per_frame):
        rows = host[offsets[f]:offsets[f + 1], :3]
        error = mapped_rms(rows, (result.scale, result.rotation, result.translation), truth)
        print("frame %d: %r, mapped-point rms error %.3g (limit %.3g)" % (f, result, error, limit))
        assert result.converged and result.count == rows.shape[0] and error <= limit
    merged = evaluate.registration_errors(out["points"], offsets, model, initial=start, merged=True)
    assert merged.converged and merged.count == total
    assert mapped_rms(host[:, :3], (merged.scale, merged.rotation, merged.translation), truth) <= limit
    matrix = np.eye(4)
    matrix[:3, :3], matrix[:3, 3] = start[0] * start[1], start[2]
    from_matrix = evaluate.registration_errors(out["points"], [0, total, total], model, initial=matrix)
    assert from_matrix[1] is None and from_matrix[0].count == total
    moved = registration.similarity_apply(cloud, merged.scale, merged.rotation, merged.translation).cpu().numpy()
    want = rr.apply(host, merged.scale, merged.rotation, merged.translation)
    assert moved.shape == host.shape and np.array_equal(moved[:, 3:], host[:, 3:])
    assert (np.abs(moved[:, :3].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-12).all()
    assert np.array_equal(cloud.cpu().numpy(), host)          # the input is left alone
