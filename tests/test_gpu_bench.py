"""GPU (-m gpu): a plain bench.py run -- the headline only -- on a small workload, with the outputs of its timed solve written out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_solve(tmp_path):
    env = dict(os.environ, SMG_BENCH_EXTRA_DIR=str(tmp_path))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small", "--steps", "7", "--warmup", "3",
                          "--dump-outputs", str(tmp_path / "dump")], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads(out.stdout.rstrip().splitlines()[-1])
    assert d["steps"] == 7 and d["warmup"] == 3 and d["n_gpus"] == 1
    assert d["unit"] == "V-cycles/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-4)
    assert d["roofline"] is None and "cpu_baseline" not in d and "extra_file" not in d
    assert not os.path.exists(tmp_path / "bench_extra.json")                                  # the full record is --full's
    z, rh = np.load(str(tmp_path / "dump" / "z.npy")), np.load(str(tmp_path / "dump" / "residual_history.npy"))
    assert z.dtype == rh.dtype == np.float64 and z.shape == (d["config"]["n_verts"],) and np.all(np.isfinite(z))
    assert len(rh) >= 10 and rh[-1] < 1e-3 * rh[0]                                            # warm-up + timed steps of one solve, converging
