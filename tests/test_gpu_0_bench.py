"""bench.py's result line, plain and with --full.  A plain run carries the headline and what its own warm-up and timed steps
measured; --full adds the figures that need work of their own after the timed steps.  Like test_gpu_0_multirank.py, the file sorts
before the other GPU tests so that the benchmark processes start while this pytest process has not yet initialised the GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("dispatches_per_step", "depth_warp_fwd_bwd_ms_per_pair", "roofline_depth_warp", "cpu_baseline")


def _bench(*extra):
    env = dict(os.environ)
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "2"] + list(extra),
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_leaves_the_extra_figures_to_full():
    assert torch.cuda.device_count() >= 1, "GPU tests need an MI355X"
    plain = _bench()
    full = _bench("--full", "--no-cpu-baseline")          # the CPU baseline alone takes minutes; its flag is what keeps it out here
    for line in (plain, full):
        assert all(key in line for key in HEADLINE)
        assert line["value"] > 0 and line["skipped_steps"] == 0 and line["roofline"]["launches"] > 0
    assert not [key for key in FULL_ONLY if key in plain]
    assert plain["roofline"]["traffic"] is None
    assert [key for key in FULL_ONLY if key not in full] == ["cpu_baseline"]
    assert full["roofline_depth_warp"]["device_ms_per_pair"] > 0
    assert full["depth_warp_fwd_bwd_ms_per_pair"] == full["roofline_depth_warp"]["host_inclusive_ms_per_pair"]
