"""GPU: bench.py as it is run for every change — the line of a plain run, and what `--dump-outputs` writes (the last timed step's logpdf, α and
a seeded probe of its factor) against the CPU oracle on the same inputs.  At N = 4 096, so that the test costs seconds."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import gp_oracle as o

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_line_and_dumped_outputs(agp, tmp_path):
    n, out = 4096, tmp_path / "outputs"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n", str(n), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "points/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["roofline"]["frac"] == pytest.approx(d["roofline"]["achieved"] / d["roofline"]["peak"], rel=1e-9)
    assert "cpu_baseline" not in d and "other_configs" not in d          # a plain run times the pair and nothing else

    lp_d, a_d, p_d = (np.load(out / f"{k}.npy") for k in ("logpdf", "alpha", "factor_probe"))
    assert lp_d.dtype == a_d.dtype == p_d.dtype == np.float64
    assert lp_d.shape == (1,) and a_d.shape == (n,) and p_d.shape == (n, 4)
    assert float(lp_d[0]) == d["logpdf"]
    x, y = o.synth_inputs(n, 3, 4)
    lp, post = o.logpdf_and_posterior(o.FiniteGP(o.GP(o.Kernel(o.SE)), x, 0.01), y)
    assert float(lp_d[0]) == pytest.approx(lp, rel=1e-10)
    assert np.linalg.norm(a_d - post.alpha) / np.linalg.norm(post.alpha) <= 1e-8
    xi = np.random.default_rng(20261016).standard_normal((n, 4))
    np.testing.assert_allclose(p_d, post.U.T @ xi, rtol=0, atol=1e-9)
