"""Multi-sample evaluation without a GPU: the float64 reference (tests/predictive_reference.py), the host arithmetic of ``Predictive``
(``iodine_amd.model.sample_bounds``) against it, and the argument checks of ``IODINE.predictive``, which raise before any library call."""
import functools

import pytest
import torch

from iodine_amd import synth
from iodine_amd.model import sample_bounds
from oracle import iodine_oracle as O

import predictive_reference as R

ARCH = O.tiny_arch(slots=3)
B, S = 2, 4


@functools.lru_cache(maxsize=None)
def _inputs():
    """(params, x, pm, plv, eps (S, B, K, L)) in float64, made once (read-only)"""
    pn = synth.make_params(O.param_shapes(ARCH), seed=41, dec_gain=3.0, posterior_scale=0.05)
    p = {k: torch.from_numpy(v).double() for k, v in pn.items()}
    imgs, _ = synth.make_images(B, ARCH.img_size, seed=3, kind='blobs')
    g = torch.Generator().manual_seed(11)
    K, L = ARCH.slots, ARCH.dim_latent
    pm = torch.randn(B, K, L, generator=g, dtype=torch.float64)
    plv = 0.5 * torch.randn(B, K, L, generator=g, dtype=torch.float64) - 1.0
    eps = torch.randn(S, B, K, L, generator=g, dtype=torch.float64)
    return p, torch.from_numpy(imgs).double(), pm, plv, eps


@functools.lru_cache(maxsize=None)
def _ref():
    p, x, pm, plv, eps = _inputs()
    return R.predictive(x, None, pm, plv, eps, p, ARCH)


def test_one_sample_bounds_coincide_exactly():
    p, x, pm, plv, eps = _inputs()
    r = R.predictive(x, None, pm, plv, eps[:1], p, ARCH)
    assert torch.equal(r['iwae'], r['log_w'][0]) and torch.equal(r['elbo_mc'], r['log_w'][0])
    assert float(r['pred_var'].abs().max()) == 0.0 and float(r['mask_var'].abs().max()) == 0.0
    assert torch.equal(r['votes'].sum(1), torch.ones(B, ARCH.img_size, ARCH.img_size, dtype=torch.int64))
    log_w, iwae, mc, _ = sample_bounds(r['ll'], r['z'], eps[:1], pm, plv)
    assert torch.equal(iwae, log_w[0]) and torch.equal(mc, log_w[0])


def test_iwae_is_at_least_the_monte_carlo_elbo():
    r = _ref()
    assert bool((r['iwae'] >= r['elbo_mc']).all())
    assert float((r['iwae'] - r['elbo_mc']).min()) > 0.0                 # (the samples do differ: Jensen's gap is open)
    _, iwae, mc, _ = sample_bounds(r['ll'], r['z'], _inputs()[4], _inputs()[2], _inputs()[3])
    assert bool((iwae >= mc).all())


def test_module_host_arithmetic_matches_the_reference():
    p, x, pm, plv, eps = _inputs()
    r = _ref()
    log_w, iwae, mc, elbo = sample_bounds(r['ll'], r['z'], eps, pm, plv)
    for name, got in (('log_w', log_w), ('iwae', iwae), ('elbo_mc', mc), ('elbo', elbo)):
        assert got.dtype == torch.float64
        assert torch.allclose(got, r[name], rtol=1e-12, atol=1e-9), name
    assert r['votes'].shape == (B, ARCH.slots, ARCH.img_size, ARCH.img_size) and int(r['votes'].sum(1).min()) == S == int(r['votes'].sum(1).max())


def test_zero_noise_unit_variance_posterior():
    """eps = 0 and logvar = 0: z = mu, log q(z) = log N(0; 0, 1) per entry, so log_w = ll - sum mu^2 / 2"""
    p, x, pm, _, eps = _inputs()
    zero, lv = torch.zeros_like(eps[:2]), torch.zeros_like(pm)
    r = R.predictive(x, None, pm, lv, zero, p, ARCH)
    want = r['ll'] - 0.5 * (pm ** 2).sum((-2, -1))[None]
    assert torch.allclose(r['log_w'], want, rtol=1e-13, atol=1e-10)
    assert torch.equal(r['z'][0], pm) and torch.equal(r['log_w'][0], r['log_w'][1])
    log_w = sample_bounds(r['ll'], r['z'], zero, pm, lv)[0]
    assert torch.allclose(log_w, want, rtol=1e-14, atol=1e-11)


def test_all_ones_weights_reproduce_the_unweighted_values():
    p, x, pm, plv, eps = _inputs()
    r = _ref()
    w = torch.ones(B, 1, ARCH.img_size, ARCH.img_size, dtype=torch.float64)
    rw = R.predictive(x, w, pm, plv, eps, p, ARCH)
    for k in ('ll', 'log_w', 'iwae', 'elbo_mc', 'elbo', 'pred_mean', 'mask_var'):
        assert torch.equal(rw[k], r[k]), k
    r2 = R.predictive(x, 2.0 * w, pm, plv, eps, p, ARCH)
    assert torch.allclose(r2['ll'], 2.0 * r['ll'], rtol=1e-14)


def test_argument_checks_raise_before_any_library_call():
    from util import hip_arch
    from iodine_amd import IODINE
    m = IODINE(hip_arch(ARCH))                                            # on the CPU: a library call would raise 'ROCm device'
    K, L, Si = ARCH.slots, ARCH.dim_latent, ARCH.img_size
    pm, plv = torch.zeros(B, K, L), torch.zeros(B, K, L)
    x = torch.zeros(B, 3, Si, Si)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match='samples'):
            m.predictive(x, samples=bad, posterior=(pm, plv))
    with pytest.raises(RuntimeError, match='eps must have shape'):
        m.predictive(x, samples=3, posterior=(pm, plv), eps=torch.zeros(2, B, K, L))
    with pytest.raises(RuntimeError, match='eps must have shape'):
        m.predictive(x, samples=3, posterior=(pm, plv), eps=torch.zeros(3, B, K, L + 1))
    with pytest.raises(ValueError, match='weights'):
        m.predictive(None, samples=2, posterior=(pm, plv), weights=torch.ones(B, Si, Si))
    assert m.posterior.mean is None
    with pytest.raises(RuntimeError, match='no posterior'):
        m.predictive(x, samples=2)
    with pytest.raises(ValueError, match='posterior must be'):
        m.predictive(x, samples=2, posterior=(pm, plv[:, :2]))
    with pytest.raises(ValueError, match='images'):
        m.predictive(x[:1], samples=2, posterior=(pm, plv))
    with pytest.raises(RuntimeError, match='ROCm device'):                # every argument is fine: the first device step refuses the CPU
        m.predictive(x, samples=2, posterior=(pm, plv))
