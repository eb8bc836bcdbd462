"""bench.py --dump-outputs DIR: what the last timed step computed, as DIR/<name>.npy (float32 / float64, <= 64 MB in all), the same
from run to run with the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load_dir(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_dump_outputs_budget_and_fixed_sample(tmp_path):
    import bench
    rs = np.random.RandomState(0)
    arrays = [("image", rs.rand(3000, 3000).astype(np.float32)), ("band00", rs.rand(40, 50)), ("band01", rs.rand(2000, 1500).astype(np.float32)),
              ("norm1", np.array([2.5]))]
    budget = 16 * 10**6
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), arrays, budget)
    a, b = _load_dir(str(tmp_path / "a")), _load_dir(str(tmp_path / "b"))
    assert sorted(a) == ["band00", "band01", "image", "norm1"]
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= budget
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype in (np.float32, np.float64)
    # small arrays whole, in their dtype; a large one as a sample of its own elements
    assert np.array_equal(a["band00"], arrays[1][1]) and a["band00"].dtype == np.float64 and a["norm1"][0] == 2.5
    img = arrays[0][1].ravel()
    assert 0 < a["image"].size < img.size and np.isin(a["image"], img).all()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dump_is_reproducible(tmp_path):
    """Two runs of the headline config with the same arguments dump the same arrays bit for bit; --steps is the timed step count."""
    lines = []
    for sub in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--cpu-seconds", "0", "--settle-ms", "20",
                            "--no-others", "--no-roofline", "--dump-outputs", str(tmp_path / sub)], capture_output=True, text=True, timeout=280, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    assert all(d["steps"] == 7 and d["ms_per_step"] > 0 for d in lines)
    a, b = _load_dir(str(tmp_path / "a")), _load_dir(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) == ["image"]
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64 * 10**6
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    # the reconstruction of uniform [0, 255) pixels, seven forward + inverse pairs after the seeded input was set back
    assert -0.01 < a["image"].min() and a["image"].max() < 255.01
