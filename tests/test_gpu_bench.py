"""bench.py as a command on the GPU: a plain run prints the headline line only
and --dump-outputs writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_headline_and_dump(tmp_path):
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                       cwd=ROOT, timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["unit"] == "edges/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["ms_per_step"] > 0
    nnz = r["config"]["nnz"]
    assert r["value"] == pytest.approx(nnz / (r["ms_per_step"] * 1e-3), rel=1e-9)
    # what --full measures is not in a plain run's line
    assert not {"roofline", "kernels", "cpu_baseline", "plan_ms"} & set(r)
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert {"aggregate", "codes", "bank_emb_out", "bank_cs"} <= set(got)
    assert sum(v.nbytes for v in got.values()) <= 64e6
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in got.values())
    c = r["config"]
    assert got["codes"].shape == (c["B"], c["F"] // c["D"])
    assert got["codes"].min() >= 0 and got["codes"].max() < c["M"]
    assert got["aggregate"].shape[1] == c["F"] and np.abs(got["aggregate"]).max() > 0
    assert got["aggregate_rows"].max() < c["B"] + c["B_prime"]
