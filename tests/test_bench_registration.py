"""Timing prints of the similarity registration: run by hand with ``pytest -m bench -s`` on an MI355X; nothing is asserted about speed."""
import importlib
import time

import numpy as np
import pytest
import torch

import registration_restate as rr

pytestmark = [pytest.mark.bench, pytest.mark.skipif(not torch.cuda.is_available(), reason="timing prints need an MI355X")]

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
registration = ea.registration

# v_mfma_f32_16x16x4_f32 issues every 32 cycles per SIMD and scores 256 pairs; the running minimum costs three vector instructions per
# matrix instruction (two v_minimum3_f32, and a compare, two selects and a move per four) of 2 cycles each on the same lanes
CYCLES_PER_256_PAIRS = 32.0 + 6.0
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9


def device_ms(launch, window_ms=300.0):
    """Milliseconds per call between two events, over as many back-to-back calls as fill the window (at least 3)."""
    for _ in range(3):
        launch()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    launch()
    stop.record()
    stop.synchronize()
    reps = int(max(3, min(5000, window_ms / max(1.0e-3, start.elapsed_time(stop)))))
    start.record()
    for _ in range(reps):
        launch()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def cdist_argmin(moved, target, limit_bytes=4 * 2 ** 30):
    """torch.cdist(...).argmin over chunks of source rows that keep the distance matrix under 4 GB."""
    rows = max(1, int(limit_bytes // (4 * target.shape[0])))
    return torch.cat([torch.cdist(moved[at:at + rows], target).argmin(dim=1) for at in range(0, moved.shape[0], rows)])


@pytest.mark.parametrize("k", [3000, 500000])
def test_bench_match(k):
    """Device time per endo_registration_match at M = 81 920 (a 256 x 320 frame) against K target rows, and torch.cdist + argmin on the
    same data in the same job.  Prints only."""
    m = 81920
    d = torch.device("cuda:0")
    rng = np.random.default_rng(k)
    target = (rng.uniform(-40.0, 40.0, (k, 3)) + np.array([150.0, -80.0, 60.0])).astype(np.float32)
    source = (target[rng.integers(0, k, m)] + rng.normal(0.0, 0.5, (m, 3))).astype(np.float32)
    model = registration.TargetModel(torch.from_numpy(target).to(d))
    src = torch.from_numpy(source).to(d)
    matcher = registration._Matcher(src, model)
    identity = registration._transform_array(1.0, None, None)
    ms = device_ms(lambda: matcher.launch(identity, float("inf")))
    pairs = float(m) * k
    bound_ms = 1000.0 * pairs / 256.0 * CYCLES_PER_256_PAIRS / (SIMDS * CLOCK_HZ)
    ms_cdist = device_ms(lambda: cdist_argmin(src, model.points))
    agree = float((matcher.index.long() == cdist_argmin(src, model.points)).float().mean())
    print()
    print("endo_registration_match M=%d K=%d: %.3f ms per match, %.3g pairs/s, %.0f %% of the MFMA + VALU bound (%.3f ms); "
          "torch.cdist + argmin: %.3f ms (%.2fx); same index on %.4f of the rows" % (
              m, k, ms, pairs / (ms * 1e-3), 100.0 * bound_ms / ms, bound_ms, ms_cdist, ms_cdist / ms, agree))
    assert matcher.sums.cpu()[0] == m


def test_bench_register_on_the_fixture():
    """Wall time per registration.register call on the fixture (M = 400, K = 1500, ~12 iterations: launch- and read-bound)."""
    source, target, _ = rr.fixture(0, 0.0, 40)
    d = torch.device("cuda:0")
    src, model = torch.from_numpy(source).to(d), registration.TargetModel(target)
    result = registration.register(src, model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        result = registration.register(src, model)
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / reps
    print()
    print("registration.register on the fixture: %.2f ms per call, %d iterations (%.3f ms per iteration)" % (
        ms, result.iterations, ms / (result.iterations + 1)))
    assert result.converged
