"""Run shape (model.K / model.n_iters set after construction): the ABI entry, the host-side refusals that come before any device work,
the engine's evaluate override, and the CPU oracle at a changed (K, T) against the reference's fixtures (gen_runshape.py)."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from iodine_amd import IODINE, _lib, synth
from iodine_amd.model import arch_namespace
from oracle import iodine_oracle as O
from util import load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_CASES = ['runshape_k6_t5_b1', 'runshape_k2_t2_b2']


def runshape_setup(g, dtype=torch.float64):
    """(constructed arch, run arch, params, x, eps) exactly as gen_runshape.py built them."""
    K0, T0, K, T, B, S, L = (int(g[f'meta_{k}']) for k in ('K', 'T', 'run_K', 'run_T', 'B', 'S', 'L'))
    sw, sx, se = (int(v) for v in g['meta_seeds'])
    assert str(g['meta_family']) == 'dsprites'
    arch = O.dsprites_arch(slots=K0, iters=T0)
    assert arch.img_size == S and arch.dim_latent == L
    pn = synth.make_params(O.param_shapes(arch), seed=sw, dec_gain=float(g['meta_dec_gain']),
                           posterior_scale=float(g['meta_post_scale']))
    params = {k: torch.from_numpy(v).to(dtype) for k, v in pn.items()}
    x = eps = None
    if str(g['meta_kind']) != 'none':
        x = torch.from_numpy(synth.make_images(B, S, seed=sx, kind=str(g['meta_kind']))[0]).to(dtype)
        eps = torch.from_numpy(synth.make_eps(T, B, K, L, seed=se)).to(dtype)
    return arch, dataclasses.replace(arch, slots=K, iters=T), params, x, eps


def _module(K=3, T=2):
    return IODINE(arch_namespace(8, T, K, 16, (32, 2, 32), (32, 2)))     # tiny arch, parameters on the CPU


def test_header_declares_and_library_exports_set_run_shape():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    assert re.search(r'\bint iodine_set_run_shape\(iodine_handle\* h, int slots, int iters\);', header)
    assert 'iodine_set_run_shape' in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, 'iodine_set_run_shape')
    assert L.iodine_set_run_shape(None, 4, 3) == 1              # IODINE_ERR_INVALID on a null handle, no device touched
    assert L.iodine_abi_version() == 3                          # additive: the ABI version stays


@pytest.mark.parametrize('attr,value', [('K', 17), ('K', 0), ('K', 2.5), ('n_iters', 0), ('n_iters', -1)])
def test_bad_run_shape_is_refused_on_the_host(attr, value):
    """ValueError naming the limit, before the device check (which would raise RuntimeError for CPU tensors)."""
    m = _module()
    setattr(m, attr, value)
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match=r'1\.\.16' if attr == 'K' else '>= 1'):
        m.reconstruct(x)
    with pytest.raises(ValueError):
        m.encode(x)
    with pytest.raises(ValueError):
        m.elbo(x)
    with pytest.raises(ValueError):
        m(x)
    with pytest.raises(ValueError):
        m.max_batch()


@pytest.mark.parametrize('shape', [(2, 17, 8), (2, 3, 9), (2, 0, 8), (3, 8), (1, 2, 3, 8)])
def test_decode_checks_z_on_the_host(shape):
    m = _module()
    with pytest.raises(ValueError, match=r'\(B, K, 8\)'):
        m.decode(torch.zeros(shape))


def test_decode_takes_k_from_z_and_keeps_model_k():
    """a valid z of another slot count passes the host checks (and then needs the device) without touching model.K"""
    m = _module(K=3)
    with pytest.raises(RuntimeError, match='ROCm device'):
        m.decode(torch.zeros(2, 1, 8))
    assert m.K == 3 and m.max_batch(K=1) >= m.max_batch()


def test_max_batch_follows_the_run_shape():
    m = _module(K=3, T=2)
    base, base_t = m.max_batch(), m.max_batch(training=True)
    m.K, m.n_iters = 12, 8
    assert m.max_batch() < base and m.max_batch(training=True) < base_t
    assert m.max_batch(K=3, T=2) == base


def test_evaluate_applies_and_restores_slots_and_iters():
    from iodine_amd import engine

    class Model:
        K, n_iters = 7, 5

        def eval(self):
            return self

    class Recorder:
        def __init__(self):
            self.aris, self.seen = [], []

        def reset(self):
            self.aris = []

        def evaluate(self, model, data):
            self.seen.append((model.K, model.n_iters))
            self.aris.append(1.0)

    class Loader(list):
        dataset = [0, 1]

    loader = Loader([(torch.zeros(1, 3, 8, 8), [torch.zeros(1, 8, 8)])] * 2)
    m, ev = Model(), Recorder()
    out = engine.evaluate(m, loader, 'cpu', evaluator=ev, slots=11, iters=7)
    assert out is ev and ev.seen == [(11, 7), (11, 7)] and ev.global_mean == 1.0
    assert (m.K, m.n_iters) == (7, 5)
    ev.seen.clear()
    engine.evaluate(m, loader, 'cpu', evaluator=ev, iters=9)
    assert ev.seen == [(7, 9), (7, 9)] and (m.K, m.n_iters) == (7, 5)

    class Failing(Recorder):
        def evaluate(self, model, data):
            raise KeyError('boom')
    with pytest.raises(KeyError):
        engine.evaluate(m, loader, 'cpu', evaluator=Failing(), slots=2)
    assert (m.K, m.n_iters) == (7, 5)


def _close_to_summary(t, g, key, tol):
    a = t.detach().double().flatten()
    ss, ref_ss = float((a * a).sum()), float(g[key + '.sumsq'])
    step = max(1, a.numel() // 16)
    rms = np.sqrt(ref_ss / a.numel())
    return (tuple(t.shape) == tuple(g[key + '.shape']) and abs(ss - ref_ss) <= tol * ref_ss + 1e-300
            and np.abs(a[::step][:16].numpy() - g[key + '.sample']).max() <= tol * rms + 1e-300)


@pytest.mark.parametrize('case', RUN_CASES)
def test_oracle_at_changed_run_shape_matches_reference(case):
    """The oracle takes K / T from its Arch; at (K', T') with the constructed model's weights it reproduces the reference module
    whose attributes were set to (K', T') after construction."""
    g = load_golden(case)
    _, arch, params, x, eps = runshape_setup(g)
    ref = O.reconstruct(x, eps, params, arch)
    assert rel_err(ref['elbos'], g['f64.recon.elbos']) < 1e-9
    assert rel_err(ref['post_mean'], g['f64.recon.post_mean']) < 1e-8
    assert rel_err(ref['post_logvar'], g['f64.recon.post_logvar']) < 1e-8
    assert rel_err(ref['pred'], g['f64.recon.pred']) < 1e-6
    assert rel_err(ref['mask'], g['f64.recon.mask']) < 1e-6
    assert _close_to_summary(ref['mean'], g, 'f64.recon.mean', 1e-8)
    assert (ref['mask'][:, :, 0].argmax(1).numpy() == g['f64.recon.argmax']).all()
    out, grads = O.train_step_grads(x, eps, params, arch)
    assert abs(out['loss'].item() - float(g['f64.train.loss'])) <= 1e-10 * abs(float(g['f64.train.loss']))
    assert rel_err(out['elbos'], g['f64.train.elbos']) < 1e-9
    bad = [n for n in params if not _close_to_summary(grads[n], g, f'f64.train.grad.{n}', 1e-6)]
    assert not bad, bad


def test_oracle_decodes_a_single_slot_like_the_reference():
    g = load_golden('runshape_decode_k1_b2')
    arch, _, params, _, _ = runshape_setup(g)
    z = torch.from_numpy(g['z']).double()
    assert z.shape == (2, 1, arch.dim_latent)
    mean, logits = O.decoder(z, params, arch)
    mask = torch.softmax(logits, dim=1)
    pred = (mask * mean).sum(1)
    for name, t in (('pred', pred), ('mask', mask), ('mean', mean)):
        assert rel_err(t, g[f'f64.decode.{name}']) < 1e-6, name
