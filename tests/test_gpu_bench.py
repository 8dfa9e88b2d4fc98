"""bench.py on a real MI355X (-m gpu), small sizes: a plain run times exactly --steps steps and writes what its last step
returned, the same bits in two runs of the same arguments; --full adds the measurements beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--cells", "20000", "--dims", "10", "--landmarks", "200"]


def _bench(*args):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    outs = [_bench("--steps", "3", "--warmup", "1", *SMALL, "--dump-outputs", str(tmp_path / run)) for run in ("a", "b")]
    for out in outs:
        assert out["metric"] == "cells/sec fit_predict" and out["unit"] == "cells/s" and out["higher_is_better"] is True
        assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "f64" and out["ms_per_step"] > 0
        assert abs(out["value"] * out["ms_per_step"] / 1e3 - 20000) < 1e-6 * 20000
        for key in ("cpu_baseline", "predict", "ms_per_step_host_to_host", "ms_per_step_mixed"):
            assert key not in out
    a, b = (np.load(tmp_path / run / "log_density.npy") for run in ("a", "b"))
    assert a.dtype == np.float64 and a.shape == (20000,) and np.all(np.isfinite(a))
    assert np.array_equal(a, b)


def test_full_run_keeps_the_measurements_beside_the_headline():
    out = _bench("--steps", "2", "--warmup", "1", *SMALL, "--landmark-method", "device", "--full", "--extra-steps", "1",
                 "--cpu-sample", "2000")
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["config"]["predict_equals_fit_predict_rel_max"] < 1e-8
    assert out["predict"]["value"] > 0 and out["predict"]["equals_fit_predict_rel_max"] < 1e-8
    assert out["ms_per_step_host_to_host"] > 0 and out["ms_per_step_mixed"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["predict"]["cpu_baseline"]["value"] > 0
