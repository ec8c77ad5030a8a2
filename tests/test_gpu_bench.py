"""bench.py's command line: a plain run times its steps and prints the result
line only; --dump-outputs writes the last timed step's result records;
--full adds the CPU baseline and the parity check against the oracle."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = ["--gpus", "1", "--nsub", "48", "--nchan", "64", "--nbin", "512",
         "--passes", "1"]


def _bench(args):
    out = subprocess.run([sys.executable, os.path.join(
        os.path.dirname(HERE), "bench.py")] + args, stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True, timeout=240)
    assert out.returncode == 0, out.stdout
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """A plain run (no --full) carries the headline fields and no CPU
    baseline or parity; --dump-outputs writes the gathered result records of
    the last timed step, the very bytes results_sha256 is taken over."""
    from pulseportraiture_amd import _lib
    d = _bench(SMALL + ["--steps", "2", "--warmup", "1", "--dump-outputs",
                        str(tmp_path / "out")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype",
              "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1
    # ms_per_step is the timed region over --steps: value = fits / time
    # (ms_per_step is printed to 1e-3 ms, value to 1e-2)
    assert d["value"] == pytest.approx(
        d["config"]["fits_per_step"] / (d["ms_per_step"] / 1e3),
        rel=6e-4 / d["ms_per_step"] + 1e-6)
    assert d["cpu_baseline"] is None and "parity" not in d
    assert os.listdir(tmp_path / "out") == ["results.npy"]
    r = np.load(tmp_path / "out" / "results.npy")
    assert r.dtype == np.float64 and r.shape == (48, _lib.RESULT_DOUBLES)
    assert hashlib.sha256(r.tobytes()).hexdigest() == d["results_sha256"]
    assert d["fits_converged_frac"] == 1.0


def test_bench_full_adds_cpu_baseline_and_parity():
    """--full: the oracle's fits of the first --cpu-sample sub-ints (one
    core, then --cpu-workers processes) and the device fits' parity with
    them, as a run without options gave before --full existed."""
    d = _bench(SMALL + ["--steps", "1", "--warmup", "1", "--full",
                        "--cpu-sample", "4", "--cpu-workers", "2"])
    assert d["cpu_baseline"]["value"] > 0
    assert d["cpu_baseline"]["all_core"]["workers"] == 2
    assert d["vs_cpu_baseline"] > 0
    assert d["parity"]["n"] == 4 and d["parity"]["ok"]
    assert d["parity_all_core"]["ok"]
