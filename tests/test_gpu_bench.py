"""bench.py's plain run on the GPU: exactly --steps timed MSMs in one region, none of the --full blocks on the line, and --dump-outputs holds the
point the last timed step returned -- bit-exact against the C oracle's MSM over the same bases (SRS::<Vesta>::create) and scalars (seed 1234)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_result(tmp_path):
    log_n, steps = 14, 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--log-n", str(log_n),
           "--dump-outputs", str(tmp_path)]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "KH_BENCH_FORCE_COLLECTIVE"):
        env.pop(k, None)
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and len(line["value_runs"]) == 1 and line["ms_per_step"] > 0 and line["full"] is False
    assert not {"cpu_baseline", "roofline", "prover", "value_host_scalars", "other_collective"} & set(line)
    sys.path.insert(0, ROOT)
    import bench
    n = 1 << log_n
    want, winf = cref.msm(0, cref.srs_generate(0, 0, n, threads=8), bench.rand_scalars(np.random.default_rng(1234), n), scalars_mont=True, threads=8)
    pt, inf = np.load(tmp_path / "msm_point.npy"), np.load(tmp_path / "msm_point_is_infinity.npy")
    assert pt.dtype == np.float64 and pt.shape == (2, 8) and inf.tolist() == [1.0 if winf else 0.0]
    words = pt.astype(np.uint64).reshape(8, 2)
    assert winf or np.array_equal(words[:, 0] | (words[:, 1] << np.uint64(32)), want)
