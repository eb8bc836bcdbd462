"""bench.py without --full: set-up, warm-up, the K timed steps and one JSON line with the headline fields -- none of what --full adds."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# fields that only a --full run measures
FULL_ONLY = {"gpu_ms_per_step", "steady_state", "sanity", "roundtrip_max_rel_err", "roofline", "kernels", "cpu_baseline", "power", "extra_timing",
             "clock_probe", "other_configs", "streaming_runs", "value_streaming", "c4_value", "collective", "rccl_ranks", "per_rank"}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("gpus", [1, 2])
def test_plain_run_prints_the_headline_only(gpus):
    """`bench.py --gpus N --steps K --warmup W` as the driver runs it; N = 2 starts its own two ranks, both on device 0 over gloo (the test
    hooks of tests/test_batch_gpu.py)."""
    env = dict(os.environ, PDWT_BENCH_ONE_GPU="1", PDWT_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "20", "--warmup", "5"],
                       capture_output=True, text=True, timeout=580, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "Mpixels/s fwd+inv DWT (4096² db4 L3)" and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["n_gpus"] == gpus and d["steps"] == 20 and d["warmup"] == 5 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(gpus * 4096 * 4096 / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert not FULL_ONLY & set(d), sorted(FULL_ONLY & set(d))
