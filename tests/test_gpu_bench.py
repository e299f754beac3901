"""bench.py's contract: a plain run times the steps and prints the headline line only (the CPU baseline, parity legs,
other configurations, model selection and the drop-in call run with --full); --dump-outputs writes what the timed
path returned after its last step, the same on every run with the same arguments."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_bench_cli_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True, timeout=120,
                       cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _plain(tmp, tag):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    out = tmp / tag
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "4",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600,
                       env=e, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1]), out


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(lib, tmp_path):
    a, da = _plain(tmp_path, "a")
    b, db = _plain(tmp_path, "b")
    for line in (a, b):
        assert line["steps"] == 4 and line["warmup"] == 1 and line["n_gpus"] == 1
        assert line["unit"] == "points/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["ms_per_step"] > 0 and line["value"] > 0
        # rows of all ranks per second over the timed steps: value and ms_per_step describe the same window
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 - line["config"]["rows_per_gpu"]) <= 1e-6 * line["value"]
        for key in ("cpu_baseline", "parity", "parity_overlap", "other_configs", "model_selection", "dropin_call"):
            assert key not in line, key
    names = sorted(p.name for p in da.glob("*.npy"))
    assert names == sorted(p.name for p in db.glob("*.npy"))
    assert {"free_energy.npy", "qz_sample.npy", "weights_N.npy", "cluster_mean.npy", "cluster_cov.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(da / n), np.load(db / n)
        assert x.dtype == np.float64 and np.all(np.isfinite(x)), n
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += x.nbytes
    assert total <= 64 << 20
    K = a["config"]["K"]
    assert np.load(da / "free_energy.npy")[0] == a["free_energy"]
    q = np.load(da / "qz_sample.npy")
    assert q.shape[1] == K and q.shape[0] > 0
    np.testing.assert_allclose(q.sum(1), 1.0, atol=1e-9)
    assert np.load(da / "cluster_cov.npy").shape == (K, a["config"]["D"], a["config"]["D"])
    np.testing.assert_allclose(np.load(da / "weights_N.npy").sum(), a["config"]["rows_per_gpu"], rtol=1e-9)
