"""CPU-only checks of the similarity registration: similarity_from_sums (Umeyama's closed form on the device's 20 sums), the numpy
restatement's convergence on the fixture, and the new entries of the C ABI."""
import importlib
import os
import re

import numpy as np
import pytest

import registration_restate as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
registration = importlib.import_module("endoscopydepthestimation-pytorch_amd.registration")

ENTRIES = ("endo_registration_tile", "endo_registration_prepared_bytes", "endo_registration_workspace_bytes", "endo_registration_prepare",
           "endo_registration_match", "endo_similarity_apply")


def exact_pairs(seed, n=50, mirrored=False):
    rng = np.random.default_rng(seed)
    source = rng.normal(0.0, 3.0, (n, 3)) + np.array([150.0, -80.0, 60.0])
    scale, rot, tr = 0.8, rr.rotation_about((2.0, -1.0, 0.5), 37.0), np.array([4.0, -2.0, 9.0])
    target = rr.apply(source, scale, rot, tr)
    if mirrored:
        target = target * np.array([1.0, 1.0, -1.0])
    return source, target, (scale, rot, tr)


def sums_about(source, target, source_centre, target_centre):
    index = np.arange(source.shape[0])
    return rr.sums_of(source, target, index, np.zeros(source.shape[0]), np.inf, source_centre, target_centre)


def test_recovers_a_known_similarity_from_exact_correspondences():
    source, target, (scale, rot, tr) = exact_pairs(0)
    for sc, tc in ((np.zeros(3), np.zeros(3)), (source.mean(axis=0), target.mean(axis=0))):
        s, r, t = registration.similarity_from_sums(sums_about(source, target, sc, tc), True, sc, tc)
        moved = rr.apply(source, s, r, t)
        assert abs(s - scale) <= 1e-12 and np.abs(r - rot).max() <= 1e-12
        assert np.abs(moved - target).max() <= 1e-12 * np.abs(target).max()
    s2, r2, t2 = rr.umeyama(source, target)
    assert abs(s2 - scale) <= 1e-12 and np.abs(r2 - rot).max() <= 1e-12 and np.abs(t2 - tr).max() <= 1e-10


def test_a_mirrored_set_gives_a_proper_rotation():
    source, target, _ = exact_pairs(1, mirrored=True)
    sc, tc = source.mean(axis=0), target.mean(axis=0)
    s, r, t = registration.similarity_from_sums(sums_about(source, target, sc, tc), True, sc, tc)
    assert abs(np.linalg.det(r) - 1.0) <= 1e-12 and np.abs(r @ r.T - np.eye(3)).max() <= 1e-12 and s > 0.0
    s2, r2, t2 = rr.umeyama(source, target)
    assert abs(np.linalg.det(r2) - 1.0) <= 1e-12 and abs(s - s2) <= 1e-12 and np.abs(r - r2).max() <= 1e-12


def test_with_scale_false_is_the_rigid_fit():
    source, target, (_, rot, _) = exact_pairs(2)
    sc, tc = source.mean(axis=0), target.mean(axis=0)
    s, r, t = registration.similarity_from_sums(sums_about(source, target, sc, tc), False, sc, tc)
    assert s == 1.0 and np.abs(r - rot).max() <= 1e-12          # the rotation does not depend on the scale
    assert np.abs(rr.apply(source, s, r, t).mean(axis=0) - tc).max() <= 1e-12 * np.abs(tc).max()          # the means still meet


def test_too_few_rows_and_a_source_without_extent_raise():
    source, target, _ = exact_pairs(3, n=2)
    with pytest.raises(ValueError, match="2 are within"):
        registration.similarity_from_sums(sums_about(source, target, np.zeros(3), np.zeros(3)))
    with pytest.raises(ValueError, match="0 are within"):
        registration.similarity_from_sums(np.zeros(20))
    source, target, _ = exact_pairs(4, n=5)
    flat = np.repeat(np.array([[1.0, 2.0, 3.0]]), 5, axis=0)
    with pytest.raises(ValueError, match="5 source rows"):
        registration.similarity_from_sums(sums_about(flat, target, flat[0], np.zeros(3)))


@pytest.mark.parametrize("junk", [0, 40])
@pytest.mark.parametrize("sigma", [0.0, 0.02])
def test_the_restatement_converges_on_the_fixture(sigma, junk):
    source, target, (scale, rot, tr) = rr.fixture(0, sigma, junk)
    assert source.dtype == np.float32 and source.shape == (rr.FIXTURE_M, 3) and target.shape == (rr.FIXTURE_K, 3)
    result = rr.register(source, target)
    assert result["converged"] and result["iterations"] <= 30
    assert result["count"] in ((400,) if junk == 0 else (360, 361))
    error = np.sqrt(((rr.apply(source, result["scale"], result["rotation"], result["translation"]) - rr.apply(source, scale, rot, tr)) ** 2)
                    .sum(axis=1).mean())
    if sigma == 0.0:
        assert error <= 4.0 * 2.0 ** -23 * np.abs(target).max()          # the float32 storage of coordinates near 170
        again = rr.register(source, target, fp32_score=True)          # the matrix-unit score ends on the same correspondences
        assert np.array_equal(again["index"], result["index"]) and again["count"] == result["count"]


def test_the_new_entries_are_declared_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "endo_hip.h")).read()
    assert "README" in text and "step 4" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared in include/endo_hip.h" % name
        assert name in ea._lib.SIGNATURES
    assert re.search(r"#define\s+ENDO_ABI_VERSION\s+7\b", text)
    lib = ea._lib.load()
    assert lib.endo_abi_version() == 7
    source_tile, target_tile = registration.SOURCE_TILE, registration.TARGET_TILE
    assert source_tile == int(re.search(r"#define\s+ENDO_REGISTRATION_SOURCE_TILE\s+(\d+)", text).group(1))
    assert target_tile == int(re.search(r"#define\s+ENDO_REGISTRATION_TARGET_TILE\s+(\d+)", text).group(1))
    # sizes: the prepared copy is padded to whole target tiles behind a 256-byte header; the workspace holds 20 doubles per source tile
    assert lib.endo_registration_prepared_bytes(1) == lib.endo_registration_prepared_bytes(target_tile) == 256 + 16 * target_tile
    assert lib.endo_registration_prepared_bytes(target_tile + 1) == 256 + 32 * target_tile
    assert lib.endo_registration_prepared_bytes(0) == -1 and lib.endo_registration_prepared_bytes(2 ** 31) == -1
    assert lib.endo_registration_workspace_bytes(source_tile + 1, 5) >= 2 * 20 * 8
    assert lib.endo_registration_workspace_bytes(0, 5) == -1 and lib.endo_registration_workspace_bytes(5, 0) == -1
    assert hasattr(ea, "registration") and hasattr(ea.evaluate, "registration_errors") and hasattr(ea.evaluate, "run_registration_phase")
