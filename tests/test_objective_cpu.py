"""Objective controls (model.sigma / model.beta / model.iter_weights) without a device: the reference restatement against the oracle,
the power of the chosen inputs to tell wrong compositions from the right one, the host-side refusals, the ABI entry and the engine flags.

Tiny architecture of the step tests (O.tiny_arch(): K = 3, T = 2, S = 16, L = 8; B = 2)."""
import os
import re

import numpy as np
import pytest
import torch

from iodine_amd import IODINE, _args, _lib
from iodine_amd.model import arch_namespace
from oracle import iodine_oracle as O
from util import rel_err, rel_l2

import objective_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = O.tiny_arch()
B = 2
GRAD_GATE, POST_GATE = 1e-3, 1e-4       # the GPU tests' gates: parameter-gradient rel-L2 (test_gpu_train), posterior mean (test_gpu_reconstruct)


# ---- 1. the restatement at the defaults IS the oracle ------------------------------------------------------------------------------
def test_defaults_pin_train_forward_and_grads():
    params, x, eps = R.inputs(ARCH, B)
    ref, gref = O.train_step_grads(x, eps, params, ARCH)
    out, g = R.train_step_grads(x, eps, params, ARCH, ARCH.sigma, 1.0, 'linspace')
    fwd = R.train_forward(x, eps, params, ARCH, ARCH.sigma, 1.0, None)
    fref = O.train_forward(x, eps, params, ARCH)
    for k in ('loss', 'elbos', 'kls', 'lls', 'post_mean', 'post_logvar', 'final_mask', 'final_mean'):
        assert torch.equal(out[k], ref[k]), k
        assert torch.equal(fwd[k].detach(), fref[k].detach()), k
    for n in gref:
        assert torch.equal(g[n], gref[n]), n


def test_defaults_pin_reconstruct():
    params, x, eps = R.inputs(ARCH, B)
    ref = O.reconstruct(x, eps, params, ARCH)
    out = R.reconstruct(x, eps, params, ARCH, ARCH.sigma, 1.0)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


def test_weight_names():
    assert R.weights(None, 2) == R.weights('linspace', 2) == [1 / 3, 2 / 3, 1.0]
    assert R.weights('uniform', 3) == [0.25] * 4 and R.weights('last', 2) == [0.0, 0.0, 1.0]


# ---- 2. the chosen inputs tell wrong builds from the right one -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def f64_inputs():
    return R.inputs(ARCH, B, dtype=torch.float64)


def test_beta_missing_from_the_inner_gradient_is_visible(f64_inputs):
    """(a) beta only in the reported ELBO: the posterior mean after reconstruct moves by >= 10 x the GPU gate"""
    params, x, eps = f64_inputs
    good = R.reconstruct(x, eps, params, ARCH, R.SIGMA, R.BETA)
    bad = R.reconstruct(x, eps, params, ARCH, R.SIGMA, R.BETA, beta_inner=1.0)
    assert torch.equal(good['elbos'][0], bad['elbos'][0])                   # the reported ELBO of evaluation 0 cannot tell them apart
    e = rel_err(bad['post_mean'], good['post_mean'])
    print(f'(a) posterior mean, beta not in the inner gradient: {e:.2e}')
    assert e >= 10 * POST_GATE


def test_sigma_missing_from_the_encoding_is_visible(f64_inputs):
    """(c) sigma in the likelihood, the construction-time sigma in the likelihood channels of the encoding"""
    params, x, eps = f64_inputs
    good = R.reconstruct(x, eps, params, ARCH, R.SIGMA, R.BETA)
    bad = R.reconstruct(x, eps, params, ARCH, R.SIGMA, R.BETA, sigma_enc=ARCH.sigma)
    assert torch.equal(good['elbos'][0], bad['elbos'][0])
    e = rel_err(bad['post_mean'], good['post_mean'])
    print(f'(c) posterior mean, construction-time sigma in the encoding: {e:.2e}')
    assert e >= 10 * POST_GATE


@pytest.mark.parametrize('w', ['uniform', 'last', (0.0, 0.5, 1.0), (1.0, 0.0, 0.5)], ids=str)
def test_weights_missing_from_the_gradients_are_visible(f64_inputs, w):
    """(b) weights only in the loss value: the refinement-network gradients of the default weighting differ from the right ones by
    >= 10 x the gate - all of them taken together and every single tensor but refine.lstm.weight_hh (h_0 = 0, so at T = 2 it only sees
    iteration 1, whose seed is w_T x d ELBO_T: the same wherever w_T = 1)"""
    params, x, eps = f64_inputs
    _, good = R.train_step_grads(x, eps, params, ARCH, R.SIGMA, R.BETA, w)
    _, bad = R.train_step_grads(x, eps, params, ARCH, R.SIGMA, R.BETA, 'linspace')
    names = [n for n in good if n.startswith('refine.')]
    cat = lambda g: np.concatenate([g[n].numpy().ravel() for n in names])
    errs = {n: rel_l2(bad[n].numpy(), good[n].numpy()) for n in names if n != 'refine.lstm.weight_hh'}
    print(f'(b) {w}: refine.* gradients together {rel_l2(cat(bad), cat(good)):.2e}, smallest single tensor {min(errs.values()):.2e}')
    assert rel_l2(cat(bad), cat(good)) >= 10 * GRAD_GATE
    assert min(errs.values()) >= 10 * GRAD_GATE, errs


# ---- 3. host validation, before any library call ----------------------------------------------------------------------------------
def _module(K=3, T=2):
    return IODINE(arch_namespace(8, T, K, 16, (32, 2, 32), (32, 2)))     # tiny arch, parameters on the CPU


def _refused(m, match):
    """every entry point raises ValueError before the device check (which would raise RuntimeError for CPU tensors)"""
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match=match):
        m.reconstruct(x)
    with pytest.raises(ValueError, match=match):
        m.encode(x)
    with pytest.raises(ValueError, match=match):
        m.elbo(x)
    with pytest.raises(ValueError, match=match):
        m(x)
    assert m._handle is None                                            # nothing reached the library


@pytest.mark.parametrize('value', [0.0, -0.1, float('nan'), float('inf'), 'x', None, True])
def test_bad_sigma_is_refused_on_the_host(value):
    m = _module()
    m.sigma = value
    _refused(m, r'model\.sigma')


@pytest.mark.parametrize('value', [-1e-9, float('nan'), float('inf'), '1'])
def test_bad_beta_is_refused_on_the_host(value):
    m = _module()
    m.beta = value
    _refused(m, r'model\.beta')


@pytest.mark.parametrize('value,match', [
    ([1.0, 1.0], r'2 entries.*n_iters = 2.*3 weights'), ([1.0] * 4, r'4 entries.*3 weights'), ([1.0, -0.5, 1.0], r'iter_weights\[1\]'),
    ([0.0, 0.0, 0.0], 'all zero'), ([0.0, 1e-60, 0.0], 'all zero'), ([1.0, float('nan'), 1.0], r'iter_weights\[1\]'),
    ('geometric', "'linspace', 'uniform', 'last'"), (3, "'linspace', 'uniform', 'last'")], ids=str)
def test_bad_iter_weights_are_refused_on_the_host(value, match):
    m = _module()
    m.iter_weights = value
    _refused(m, match)


def _objective(m, T):
    return _args.read_objective(m.sigma, m.beta, m.iter_weights, T)


def test_valid_objectives_pass_the_host_checks():
    m = _module(T=2)
    assert m.beta == 1.0 and m.iter_weights is None and m.sigma == 0.10
    assert _objective(m, 2) == (0.10, 1.0, ())
    m.sigma, m.beta, m.iter_weights = 0.3, 0, 'uniform'
    assert _objective(m, 2) == (0.3, 0.0, (1 / 3,) * 3) and _objective(m, 4)[2] == (0.2,) * 5      # names follow n_iters
    m.iter_weights = 'last'
    assert _objective(m, 3)[2] == (0.0, 0.0, 0.0, 1.0)
    m.iter_weights = torch.tensor([0.0, 0.5, 1.0])
    assert _objective(m, 2)[2] == (0.0, 0.5, 1.0)
    m.iter_weights = 'linspace'
    assert _objective(m, 2)[2] == ()
    # what a schedule produces: numpy scalars and one-element tensors are numbers too
    m.sigma, m.beta = np.float32(0.5), torch.tensor(2.0)
    assert _objective(m, 2)[:2] == (0.5, 2.0)
    m.sigma, m.beta, m.iter_weights = np.float64(0.3), np.int64(1), np.array([0.0, 0.5, 1.0], dtype=np.float32)
    assert _objective(m, 2) == (0.3, 1.0, (0.0, 0.5, 1.0))
    m.beta = torch.tensor([1.0, 2.0])
    with pytest.raises(ValueError, match=r'model\.beta.*type Tensor'):
        _objective(m, 2)
    m.beta, m.iter_weights = 1.0, None
    with pytest.raises(RuntimeError, match='ROCm device'):              # a valid objective goes on to the device check
        m.reconstruct(torch.zeros(1, 3, 16, 16))


# ---- 4. ABI, engine ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_set_objective():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    assert re.search(r'\bint iodine_set_objective\(iodine_handle\* h, double sigma, double beta, const double\* iter_weights, '
                     r'int n_weights\);', header)
    assert 'iodine_set_objective' in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, 'iodine_set_objective')
    assert L.iodine_set_objective(None, 0.1, 1.0, None, 0) == 1         # IODINE_ERR_INVALID on a null handle, no device touched
    assert L.iodine_abi_version() == 3                                  # additive: the ABI version stays
    assert 'iodine_set_objective' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_engine_parser_takes_the_objective_flags():
    from iodine_amd import engine
    ap = engine.make_parser()
    d = ap.parse_args([])
    assert d.sigma is None and d.beta == 1.0 and d.beta_warmup == 0 and d.iter_weights == 'linspace'
    a = ap.parse_args(['--sigma', '0.3', '--beta', '4', '--beta-warmup', '100', '--iter-weights', 'last'])
    assert (a.sigma, a.beta, a.beta_warmup, a.iter_weights) == (0.3, 4.0, 100, 'last')
    with pytest.raises(SystemExit):
        ap.parse_args(['--iter-weights', 'geometric'])


def test_beta_warmup_ramp():
    from iodine_amd.engine import beta_warmup
    assert [beta_warmup(s, 4.0, 4) for s in range(7)] == [0.0, 1.0, 2.0, 3.0, 4.0, 4.0, 4.0]
    assert beta_warmup(0, 2.0, 0) == 2.0 and beta_warmup(5, 2.0, 0) == 2.0


def test_train_sets_beta_per_step():
    """engine.train hands the ramp to the model before every step and leaves the final weight behind"""
    from iodine_amd import engine

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))
            self.beta, self.seen = 1.0, []

        def forward(self, x):
            self.seen.append(self.beta)
            return self.w * x.sum()

    m = Model()
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    data = [(torch.ones(1),)] * 2
    engine.train(m, opt, data, 'cpu', 5, log=lambda *a: None, beta=3.0, beta_warmup_steps=3)
    assert m.seen == [0.0, 1.0, 2.0, 3.0, 3.0] and m.beta == 3.0
    m.seen, m.beta = [], 0.5
    engine.train(m, opt, data, 'cpu', 2, log=lambda *a: None)
    assert m.seen == [0.5, 0.5]                                         # beta=None leaves model.beta alone
