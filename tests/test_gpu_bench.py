"""bench.py as the benchmark driver runs it: a plain run times exactly --steps steps and prints only the headline line (the side
measurements are behind --full), and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step(dev, tmp_path):
    out = tmp_path / 'outputs'
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--config', '2', '--steps', '3', '--warmup', '1',
           '--dump-outputs', str(out)]
    pr = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    log = pr.stdout.decode(errors='replace')
    assert pr.returncode == 0, log[-3000:]
    res = json.loads(log.strip().splitlines()[-1])
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in res, key
    assert res['steps'] == 3 and res['ms_per_step'] > 0
    assert res['value'] == pytest.approx(1e3 / res['ms_per_step'], rel=1e-9)
    for key in ('secondary', 'value_fp32_exact', 'value_f64', 'objective_and_gradients', 'objective_over_t', 'cpu_baseline'):
        assert key not in res, key                       # --full only
    assert sorted(os.listdir(out)) == ['objective_terms.npy', 'per_dimension_terms.npy']
    obj = np.load(out / 'objective_terms.npy')
    terms = np.load(out / 'per_dimension_terms.npy')
    assert obj.dtype == np.float64 and obj.shape == (5,)
    assert terms.dtype == np.float64 and terms.shape == (64, 5)          # config 2: D = 64
    assert np.isfinite(obj).all() and np.isfinite(terms).all()
    assert obj[0] == res['objective']
    np.testing.assert_allclose(obj[1], terms.sum(), rtol=1e-9)           # f_hat = sum of the per-output-dim terms
