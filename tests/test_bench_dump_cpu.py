"""bench.py --dump-outputs: the writer keeps every array under the 64 MB budget, float32, with the same seeded sample on every run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _arrays():
    rng = np.random.default_rng(5)
    # the infer-mode outputs of the headline workload (CLEVR6 128 x 128, K = 7, batch 32): 65 MB in float32
    return dict(pred=rng.standard_normal((32, 3, 128, 128)), mask=rng.random((32, 7, 1, 128, 128), dtype=np.float32),
                mean=rng.random((32, 7, 3, 128, 128), dtype=np.float32), elbo_terms=rng.standard_normal((5, 3)))


def test_small_outputs_are_written_whole(tmp_path):
    a = dict(loss=np.float32(1.5).reshape(()), elbo_terms=np.arange(18, dtype=np.float64).reshape(6, 3))
    bench.write_outputs(str(tmp_path), a)
    assert sorted(os.listdir(tmp_path)) == ['elbo_terms.npy', 'loss.npy']
    e = np.load(tmp_path / 'elbo_terms.npy')
    assert e.dtype == np.float32 and e.shape == (6, 3) and np.array_equal(e, a['elbo_terms'].astype(np.float32))
    assert np.load(tmp_path / 'loss.npy').reshape(-1).tolist() == [1.5]


def test_large_outputs_fit_the_budget_with_a_fixed_sample(tmp_path):
    a = _arrays()
    assert sum(v.astype(np.float32).nbytes for v in a.values()) > bench.DUMP_BUDGET
    d1, d2 = tmp_path / 'one', tmp_path / 'two'
    bench.write_outputs(str(d1), a)
    bench.write_outputs(str(d2), a)
    total = 0
    for name in ('pred', 'mask', 'mean', 'elbo_terms'):
        x, y = np.load(d1 / f'{name}.npy'), np.load(d2 / f'{name}.npy')
        assert x.dtype == np.float32 and np.array_equal(x, y)
        total += x.nbytes
        if name != 'elbo_terms':
            flat = a[name].astype(np.float32).reshape(-1)
            assert 0.9 * flat.size < x.size < flat.size
            assert np.isin(x, flat).all()                     # a sample of the array's own elements
    assert np.array_equal(np.load(d1 / 'elbo_terms.npy'), a['elbo_terms'].astype(np.float32))
    assert total <= bench.DUMP_BUDGET
