"""A plain `bench.py` run (no --full) times its steps and nothing else, and --dump-outputs writes what the last timed step
computed: C2's 64 groups, each SUM(val) equal to the sum over the same seeded inputs recomputed here on the CPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 64_000_000  # two 32 M-row fragments


def _c2_sums():
    """Exact int64 SUM(val) per key over bench.c2_numpy_generator's inputs (float64 bincounts of 16-bit halves stay exact)."""
    from workloads import SEED, fragment_rows
    lo, hi = np.zeros(64), np.zeros(64)
    for f, n in enumerate(fragment_rows(ROWS)):
        rng = np.random.Generator(np.random.PCG64(SEED + f))
        key = rng.integers(0, 64, n, dtype=np.int64)
        val = rng.integers(-2**31, 2**31, n, dtype=np.int64)
        lo += np.bincount(key, weights=val & 0xFFFF, minlength=64)
        hi += np.bincount(key, weights=val >> 16, minlength=64)
    return [int(h) * 65536 + int(l) for h, l in zip(hi, lo)]


def test_plain_run_times_the_steps_and_dumps_the_result(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HDK_BENCH_DETAIL=str(tmp_path / "detail.json"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HDK_BENCH_BACKEND"):
        env.pop(k, None)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--rows", str(ROWS),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.rstrip("\n").splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "int64"
    assert line["value"] == pytest.approx(ROWS / (line["ms_per_step"] * 1e-3), rel=1e-6)
    # nothing beyond the timed steps: no checks, CPU baseline, other configs, end-to-end leg or emulation
    assert line["checks"] is None and line["cpu_baseline"] is None
    assert not any(k in line for k in ("configs", "end_to_end", "multi_gpu_emulated"))
    assert sorted(os.listdir(out)) == ["key.npy", "s.npy"]
    key, s = np.load(out / "key.npy"), np.load(out / "s.npy")
    assert key.dtype == s.dtype == np.float64
    assert key.tolist() == list(range(64))
    assert s.tolist() == [float(v) for v in _c2_sums()]
