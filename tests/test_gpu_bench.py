"""bench.py without --full: the headline line only, exactly --steps timed steps, and --dump-outputs with the last timed step's
outputs - the same on two runs of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _run(mode, out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--config', 'dsprites',
                        '--batch', '4', '--mode', mode, '--dump-outputs', str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.parametrize('mode,names', [('train', ('elbo_terms', 'grads', 'loss', 'params')),
                                        ('infer', ('elbo_terms', 'mask', 'mean', 'pred'))])
def test_plain_run_line_and_outputs(tmp_path, mode, names):
    out = _run(mode, tmp_path / 'a')
    assert all(k in out for k in HEAD) and out['steps'] == 3 and out['ms_per_step'] > 0 and out['value'] > 0
    assert out['metric'] == 'refinement_iters_per_s' and out['higher_is_better'] is True
    for k in ('roofline', 'kernels', 'sustained', 'inference_step', 'exact_fp32', 'configs', 'cpu_baseline'):
        assert k not in out, k
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')}
    assert tuple(sorted(got)) == names
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10 ** 6
    assert got['elbo_terms'].shape == ((6, 3) if mode == 'train' else (5, 3))
    if mode == 'train':
        assert got['grads'].shape == got['params'].shape and np.abs(got['grads']).max() > 0
    else:
        assert got['pred'].shape == (4, 3, 64, 64) and got['mask'].shape == (4, 6, 1, 64, 64)
    # same arguments, same inputs: a second run computes the same ELBO trajectory
    _run(mode, tmp_path / 'b')
    again = np.load(tmp_path / 'b' / 'elbo_terms.npy')
    assert np.allclose(again, got['elbo_terms'], rtol=1e-4, atol=1e-3)
