"""bench.py's own contract: a plain run times exactly --steps generations and prints the headline line without the
--full legs; --dump-outputs writes what the timed path left after its last step, the same from run to run; above
64 MB the outputs are a fixed, seeded sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_outputs_over_the_limit_are_a_fixed_seeded_sample():
    rng = np.random.default_rng(0)
    arrays = {"big": rng.standard_normal((300, 1000)).astype(np.float32),
              "small": np.arange(10, dtype=np.float64)}
    assert bench.limit_outputs(arrays, limit=10 << 20) == arrays  # under the limit: untouched
    a, b = bench.limit_outputs(arrays, limit=400_000), bench.limit_outputs(dict(arrays), limit=400_000)
    assert sum(v.nbytes for v in a.values()) <= 400_000
    assert np.array_equal(a["small"], arrays["small"])
    assert 1024 <= a["big"].size < arrays["big"].size and a["big"].dtype == np.float32
    assert np.array_equal(a["big"], b["big"])  # the same elements every time
    assert np.isin(a["big"], arrays["big"]).all()


def _run(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(lines[-1])


@pytest.mark.gpu
def test_plain_run_and_its_outputs(tmp_path):
    """Two plain runs with the same arguments: the line carries the headline keys and nothing of --full, --steps is
    the number of timed steps, and the two dumps hold the same arrays (float32 / float64, under 64 MB)."""
    args = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--prefill", "30", "--hidden", "256", "--streams", "32"]
    outs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = _run(args + ["--dump-outputs", str(d)])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in out, key
        assert out["steps"] == 7 and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert abs(out["value"] - 7 * 32 / (out["ms_per_step"] * 1e-3 * 7)) < 1e-6 * out["value"]
        assert "roofline" not in out and "cpu_baseline" not in out and "replica_checksums" not in out
        outs.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
    a, b = outs
    assert set(a) >= set(bench.DUMP_F32) | set(bench.DUMP_F64) | {"training_stats"} and set(a) == set(b)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert a["hist"].shape == (20, 32, a["ih_w"].shape[0]) and a["hidden"].shape[0] == 32
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.allclose(a[k], b[k], rtol=1e-5, atol=1e-6 * max(float(np.abs(b[k]).max()), 1e-30)), k
