"""One set of weights at another slot / iteration count: ``model.K`` / ``model.n_iters`` set after construction (the reference reads
both on every call, lib/modeling/iodine.py:81-83,123-126; ``decode(z)`` takes K from z, iodine.py:430) against the CPU oracle at
dataclasses.replace(arch, slots=K', iters=T') with the same parameters, and against the reference's own fixtures (gen_runshape.py)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from iodine_amd import _lib, synth
from iodine_amd.ari import ari_tables, compute_ari
from oracle import ari_oracle as A
from oracle import iodine_oracle as O
from test_runshape_cpu import runshape_setup
from util import grad_views, load_golden, make_hip_model, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _library_has_run_shape():
    """No device work before this: a library without the entry point would size its buffers by the constructor's shape while the
    module sizes its tensors by model.K - every test here must stop before its first launch then."""
    assert hasattr(_lib.lib(), 'iodine_set_run_shape'), 'libiodine_hip.so has no iodine_set_run_shape'


def _params(arch, seed):
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    return {k: torch.from_numpy(v) for k, v in pn.items()}


def _inputs(arch, B, seed, K, T):
    """images and the (T+1, B, K, L) noise of a call at run shape (K, T)"""
    imgs, gt = synth.make_images(B, arch.img_size, seed=seed, kind='blobs')
    return torch.from_numpy(imgs), torch.from_numpy(synth.make_eps(T, B, K, arch.dim_latent, seed=seed + 1)), gt


def _check_reconstruct(m, x, eps, arch, K, T, tag):
    """reconstruct + encode at the module's current (K, T) vs the oracle; returns a list of failures"""
    run = dataclasses.replace(arch, slots=K, iters=T)
    ref = O.reconstruct(x, eps, m._oracle_params, run)
    xd, ed = x.to(DEV), eps.to(DEV)
    pred, mask, mean = m.reconstruct(xd, ed)
    B, S, L = x.shape[0], arch.img_size, arch.dim_latent
    bad = []
    if tuple(mask.shape) != (B, K, 1, S, S) or tuple(mean.shape) != (B, K, 3, S, S) or tuple(m.elbo_terms.shape) != (T, 3):
        return [(tag, 'shape', tuple(mask.shape), tuple(m.elbo_terms.shape))]
    if tuple(m.posterior.mean.shape) != (B, K, L) or tuple(m.z.shape) != (B, K, L) or tuple(m.mask.shape) != (B, K, 1, S, S):
        return [(tag, 'state shape')]
    checks = [('elbo', rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']), 1e-4), ('kl', rel_err(m.elbo_terms[:, 1].cpu(), ref['kls']), 1e-4),
              ('pred', rel_err(pred.cpu(), ref['pred']), 2e-4), ('mask', rel_err(mask.cpu(), ref['mask']), 2e-4),
              ('mean', rel_err(mean.cpu(), ref['mean']), 2e-4),
              ('post_mean', rel_err(m.posterior.mean.cpu(), ref['post_mean']), 2e-4),
              ('post_logvar', rel_err(m.posterior.logvar.cpu(), ref['post_logvar']), 2e-4)]
    agree = (mask[:, :, 0].argmax(1).cpu() == ref['mask'][:, :, 0].argmax(1)).float().mean().item()
    z = m.encode(xd, ed)
    checks.append(('z', rel_err(z.cpu(), ref['z']), 2e-4))
    bad += [(tag, n, e) for n, e, tol in checks if not e < tol]
    if not agree >= 0.999:
        bad.append((tag, 'argmax', agree))
    from iodine_amd.model import logger
    if f'mask_{K - 1}' not in logger or tuple(logger[f'mask_{K - 1}'].shape) != (S, S):
        bad.append((tag, 'logger'))
    return bad


def _model(arch, params, options=None):
    m = make_hip_model(arch, params, options=options)
    m._oracle_params = params
    return m


@pytest.mark.parametrize('prec', [1, 0], ids=['split_f16x3', 'exact_fp32'])
@pytest.mark.parametrize('family', ['tiny', 'cfg1'])
def test_reconstruct_at_other_slot_and_iteration_counts(family, prec):
    """K' in {1, 2, K + 3, 16} x T' in {1, T + 3} on ONE model built at (K, T): every call re-plans for the shape it reads"""
    arch = O.tiny_arch(slots=3, iters=2) if family == 'tiny' else O.dsprites_arch(slots=4, iters=3)
    m = _model(arch, _params(arch, seed=61), options={'conv_precision': prec})
    bad = []
    for K in (1, 2, arch.slots + 3, 16):
        for T in (1, arch.iters + 3):
            x, eps, _ = _inputs(arch, 2, seed=7 * K + T, K=K, T=T)
            m.K, m.n_iters = K, T
            bad += _check_reconstruct(m, x, eps, arch, K, T, (K, T))
    assert not bad, bad
    m.K, m.n_iters = arch.slots, arch.iters                      # and back at the constructed shape
    x, eps, _ = _inputs(arch, 2, seed=3, K=arch.slots, T=arch.iters)
    assert not _check_reconstruct(m, x, eps, arch, arch.slots, arch.iters, 'constructed')


def test_paper_setting_cfg3_weights_at_eleven_slots_seven_iterations():
    """the generalisation run of the paper: CLEVR6 weights (K = 7, T = 5) evaluated with K = 11 and more iterations (BASELINE cfg5's
    shape); K' = 11 > 9 takes the unfused encoding + first refinement layer.  Image 0 vs the oracle, ARI tables at K' vs the ARI oracle,
    and engine.evaluate(slots=, iters=) on the same module"""
    from iodine_amd import engine
    arch = O.clevr_arch(slots=7, iters=5)
    params = _params(arch, seed=71)
    m = _model(arch, params)
    K, T = 11, 7
    x, eps, gt = _inputs(arch, 2, seed=72, K=K, T=T)
    m.K, m.n_iters = K, T
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    assert tuple(mask.shape) == (2, K, 1, 128, 128)
    ref = O.reconstruct(x[:1], eps[:, :1].contiguous(), params, dataclasses.replace(arch, slots=K, iters=T))
    assert rel_err(pred[:1].cpu(), ref['pred']) < 2e-4
    assert rel_err(mask[:1].cpu(), ref['mask']) < 2e-4
    assert rel_err(mean[:1].cpu(), ref['mean']) < 2e-4
    assert rel_err(m.posterior.mean[:1].cpu(), ref['post_mean']) < 2e-4
    assert (mask[:1, :, 0].argmax(1).cpu() == ref['mask'][:, :, 0].argmax(1)).float().mean() >= 0.999
    tables = ari_tables(mask, gt)
    assert tables.shape == (2, max(len(g) for g in gt), K)
    onehot = A.binarize_argmax(mask.cpu().numpy())
    for b in range(2):
        assert (tables[b, :len(gt[b])] == A.contingency(gt[b], onehot[b])).all()
    ari_ref = A.compute_mask_ari(gt[0], A.binarize_argmax(ref['mask'].numpy())[0])
    assert abs(compute_ari(tables[0, :len(gt[0])]) - ari_ref) < 1e-2

    class Loader(list):
        dataset = [0, 1]
    m.K, m.n_iters = 7, 5
    loader = Loader([(x, [torch.from_numpy(g) for g in gt])])
    ev = engine.evaluate(m, loader, DEV, slots=K, iters=T)
    assert (m.K, m.n_iters) == (7, 5) and len(ev.aris) == 2 and all(np.isfinite(ev.aris))
    assert tuple(m.mask.shape) == (2, K, 1, 128, 128) and tuple(m.elbo_terms.shape) == (T, 3)


@pytest.mark.parametrize('case', ['runshape_k6_t5_b1', 'runshape_k2_t2_b2'])
def test_run_shape_against_reference_fixture(case):
    """the reference module built at cfg1 (K = 4, T = 3) with its attributes set afterwards: the same on the HIP module"""
    g = load_golden(case)
    arch0, run, params, x, eps = runshape_setup(g, torch.float32)
    m = make_hip_model(arch0, params)
    m.K, m.n_iters = run.slots, run.iters
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    assert abs(loss.item() - float(g['f64.train.loss'])) <= 1e-4 * abs(float(g['f64.train.loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f64.train.elbos']) < 1e-4
    bad = []
    for n, p in m.named_parameters():
        a = p.grad.double().cpu().flatten()
        ss, ref_ss = float((a * a).sum()), float(g[f'f64.train.grad.{n}.sumsq'])
        step = max(1, a.numel() // 16)
        rms = np.sqrt(ref_ss / a.numel())
        if abs(ss - ref_ss) > 2e-3 * ref_ss + 1e-12 or np.abs(a[::step][:16].numpy() - g[f'f64.train.grad.{n}.sample']).max() > 2e-3 * rms + 1e-7:
            bad.append((n, ss, ref_ss))
    assert not bad, bad
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f64.recon.elbos']) < 1e-4
    assert rel_err(m.posterior.mean.cpu(), g['f64.recon.post_mean']) < 2e-4
    assert rel_err(pred.cpu(), g['f64.recon.pred']) < 2e-4 and rel_err(mask.cpu(), g['f64.recon.mask']) < 2e-4
    a = mean.double().cpu().flatten()
    assert abs(float((a * a).sum()) - float(g['f64.recon.mean.sumsq'])) <= 1e-4 * float(g['f64.recon.mean.sumsq'])
    assert (mask[:, :, 0].argmax(1).cpu().numpy() == g['f64.recon.argmax']).mean() >= 0.999


def test_decode_single_slot_against_reference_fixture():
    g = load_golden('runshape_decode_k1_b2')
    arch0, _, params, _, _ = runshape_setup(g, torch.float32)
    m = make_hip_model(arch0, params)
    pred, mask, mean = m.decode(torch.from_numpy(g['z']).to(DEV))
    assert tuple(mask.shape) == (2, 1, 1, 64, 64) and m.K == arch0.slots
    for name, t in (('pred', pred), ('mask', mask), ('mean', mean)):
        assert rel_err(t.cpu(), g[f'f64.decode.{name}']) < 2e-4, name


def _train_vs_oracle(m, arch, K, T, B, seed, paths=(False,), tol=1e-3, loss_tol=1e-5):
    """one training step at (K, T) on each path (chunked: batch_cap 1) vs ONE oracle step"""
    x, eps, _ = _inputs(arch, B, seed, K, T)
    out, grads = O.train_step_grads(x, eps, m._oracle_params, dataclasses.replace(arch, slots=K, iters=T))
    for chunked in paths:
        m.K, m.n_iters = K, T
        m.set_option('batch_cap', 1 if chunked else 0)
        m.zero_grad(set_to_none=True)
        loss = m(x.to(DEV), eps.to(DEV))
        loss.backward()
        m.set_option('batch_cap', 0)
        assert abs(loss.item() - out['loss'].item()) <= loss_tol * abs(out['loss'].item()), (K, T, chunked)
        assert tuple(m.elbo_terms.shape) == (T + 1, 3)
        bad = [(n, rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy()))) for n, p in m.named_parameters()
               if not rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy())) < tol]
        assert not bad, (K, T, chunked, bad)


@pytest.mark.parametrize('family', ['tiny', 'cfg1'])
def test_training_step_at_other_run_shapes_matches_oracle(family):
    """every gradient tensor at (K', T') on the plain and the chunked (batch_cap) path"""
    arch = O.tiny_arch(slots=3, iters=2) if family == 'tiny' else O.dsprites_arch(slots=3, iters=2)
    m = _model(arch, _params(arch, seed=81))
    for K, T in ((arch.slots + 3, arch.iters + 1), (1, 1), (2, arch.iters + 2)):
        _train_vs_oracle(m, arch, K, T, 2, seed=10 * K + T, paths=(False, True))


def test_backward_differentiates_the_forward_as_it_ran():
    """model.K / n_iters changed between loss = model(x) and loss.backward(): the gradients of the forward's shape (the reference's
    autograd graph is fixed at forward time); the next call then runs at the new shape"""
    arch = O.dsprites_arch(slots=3, iters=2)
    params = _params(arch, seed=91)
    m = _model(arch, params)
    K, T = 5, 3
    x, eps, _ = _inputs(arch, 2, seed=92, K=K, T=T)
    m.K, m.n_iters = K, T
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV))
    m.K, m.n_iters = 2, 1
    loss.backward()
    out, grads = O.train_step_grads(x, eps, params, dataclasses.replace(arch, slots=K, iters=T))
    assert abs(loss.item() - out['loss'].item()) <= 1e-5 * abs(out['loss'].item())
    bad = [n for n, p in m.named_parameters() if not rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy())) < 1e-3]
    assert not bad, bad
    x2, eps2, _ = _inputs(arch, 2, seed=93, K=2, T=1)
    assert not _check_reconstruct(m, x2, eps2, arch, 2, 1, 'after')


def test_library_refusals_are_host_side_return_codes():
    """iodine_set_run_shape's limits, a pending training forward discarded by a shape change (IODINE_ERR_STATE), an installed workspace
    too small for the run shape (IODINE_ERR_WORKSPACE): each returned before any launch; the handle keeps working afterwards"""
    arch = O.tiny_arch(slots=2, iters=2)
    params = _params(arch, seed=95)
    m = _model(arch, params)
    x, eps, _ = _inputs(arch, 1, seed=96, K=2, T=2)
    xd, ed = x.to(DEV), eps.to(DEV)
    m.reconstruct(xd, ed)
    L, h = _lib.lib(), m._handle
    assert L.iodine_set_run_shape(h, 17, 2) == 1 and b'1..16' in L.iodine_last_error(h)
    assert L.iodine_set_run_shape(h, 0, 2) == 1 and L.iodine_set_run_shape(h, 2, 0) == 1
    small = L.iodine_workspace_bytes(h, 1, 0)
    assert L.iodine_set_run_shape(h, 16, 5) == 0
    assert L.iodine_workspace_bytes(h, 1, 0) > small
    # the wrapper's workspace was sized for (2, 2): a reconstruct at (16, 5) must be refused before it runs
    S, Ld = arch.img_size, arch.dim_latent
    f = dict(device=DEV, dtype=torch.float32)
    e16 = torch.zeros((6, 1, 16, Ld), **f)
    outs = [torch.empty((1, 3, S, S), **f), torch.empty((1, 16, 1, S, S), **f), torch.empty((1, 16, 3, S, S), **f),
            torch.empty((1, 16, Ld), **f), torch.empty((1, 16, Ld), **f), torch.empty((1, 16, Ld), **f), torch.empty((5, 3), **f)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.iodine_reconstruct(h, st, 1, _lib.ptr(xd), _lib.ptr(e16), *[_lib.ptr(t) for t in outs])
    assert rc == 4, L.iodine_last_error(h)
    assert L.iodine_set_run_shape(h, 2, 2) == 0
    # the state of the last successful call is still read at its own shape
    z = torch.empty((1, 2, Ld), **f)
    assert L.iodine_last_elbo_outputs(h, st, 1, _lib.ptr(z), None, None, None, None) == 0
    # a pending training forward is discarded by a shape change
    m(xd, ed)
    assert L.iodine_set_run_shape(h, 3, 2) == 0
    flat = torch.zeros(sum(p.numel() for p in m.parameters()), **f)
    assert L.iodine_train_backward_flat(h, st, None, _lib.ptr(flat), 0) == 3
    assert L.iodine_set_run_shape(h, 2, 2) == 0
    torch.cuda.synchronize()
    assert not _check_reconstruct(m, x, eps, arch, 2, 2, 'after refusals')


@pytest.mark.parametrize('path', ['generic_k5', 'padded_latent6', 'ref_stride3'])
def test_other_paths_at_other_run_shapes(path):
    """the generic path (5 x 5 decoder), the padded handle (DIM_LATENT 6: PadShim forwards the run shape, its scratch grows with it),
    REF.STRIDE 3 - training step and reconstruct at K' != K vs the oracle"""
    base = O.tiny_arch(slots=3, iters=2)
    arch = dict(generic_k5=dataclasses.replace(base, ref_kernel=5, dec_kernel=5,
                                               encoding=tuple(e for e in O.FULL_ENCODING if e != 'coordinate')),
                padded_latent6=dataclasses.replace(base, dim_latent=6),
                ref_stride3=dataclasses.replace(base, ref_stride=3))[path]
    m = _model(arch, _params(arch, seed=101))
    for K, T in ((5, 3), (1, 2), (2, 1)):
        _train_vs_oracle(m, arch, K, T, 2, seed=K + 10 * T, tol=2e-3, loss_tol=1e-4)
        x, eps, _ = _inputs(arch, 2, seed=K + 20 * T, K=K, T=T)
        bad = _check_reconstruct(m, x, eps, arch, K, T, (K, T))
        assert not bad, bad
    if path == 'padded_latent6':                            # the chunked path behind the padded handle at a grown shape
        _train_vs_oracle(m, arch, 6, 3, 2, seed=5, paths=(True,), tol=2e-3, loss_tol=1e-4)


def test_decode_takes_the_slot_count_from_z():
    arch = O.dsprites_arch(slots=4, iters=3)
    params = _params(arch, seed=111)
    m = _model(arch, params)
    for K in (1, 3, arch.slots + 2):
        z = torch.from_numpy(synth.make_eps(0, 2, K, arch.dim_latent, seed=K)[0])
        pred, mask, mean = m.decode(z.to(DEV))
        mr, lg = O.decoder(z, params, arch)
        kr = torch.softmax(lg, dim=1)
        assert tuple(mask.shape) == (2, K, 1, 64, 64) and m.K == arch.slots
        assert rel_err(mean.cpu(), mr) < 2e-4 and rel_err(mask.cpu(), kr) < 2e-4 and rel_err(pred.cpu(), (kr * mr).sum(1)) < 2e-4
    # every slot of a reconstruct's z decoded alone (the disentanglement experiment of the reference's notes.md)
    x, eps, _ = _inputs(arch, 2, seed=112, K=arch.slots, T=arch.iters)
    z = m.encode(x.to(DEV), eps.to(DEV))
    for k in range(arch.slots):
        pred, mask, mean = m.decode(z[:, k:k + 1])
        mr, _ = O.decoder(z[:, k:k + 1].cpu(), params, arch)
        assert rel_err(mean.cpu(), mr) < 2e-4 and rel_err(mask.cpu(), torch.ones_like(mask.cpu())) < 1e-6
        assert rel_err(pred.cpu(), mr[:, 0]) < 2e-4
    assert not _check_reconstruct(m, x, eps, arch, arch.slots, arch.iters, 'after decodes')


def _round_trip(m, arch, x, eps_k, x2, eps2, K2, T2):
    """K -> K' (+ a training step there) -> K: what the last calls at K return"""
    xd, ed = x.to(DEV), eps_k.to(DEV)
    m.K, m.n_iters = arch.slots, arch.iters
    m.reconstruct(xd, ed)
    m.K, m.n_iters = K2, T2
    m.reconstruct(x2.to(DEV), eps2.to(DEV))
    m.zero_grad(set_to_none=True)
    m(x2.to(DEV), eps2.to(DEV)).backward()
    m.K, m.n_iters = arch.slots, arch.iters
    rec = [t.clone() for t in m.reconstruct(xd, ed)]
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    torch.cuda.synchronize()
    return rec, loss.detach().clone(), [p.grad.clone() for p in m.parameters()]


def test_no_stale_state_after_a_round_trip():
    """K -> K' -> K (with a training step at K') is bitwise a fresh model at K, eager and (graph mode, alternating shapes) replayed"""
    arch = O.dsprites_arch(slots=4, iters=3)
    params = _params(arch, seed=121)
    x, eps, _ = _inputs(arch, 2, seed=122, K=4, T=3)
    x2, eps2, _ = _inputs(arch, 2, seed=123, K=7, T=5)
    fresh = make_hip_model(arch, params)
    r0 = [t.clone() for t in fresh.reconstruct(x.to(DEV), eps.to(DEV))]
    fresh.zero_grad(set_to_none=True)
    l0 = fresh(x.to(DEV), eps.to(DEV))
    l0.backward()
    g0 = [p.grad.clone() for p in fresh.parameters()]
    m = make_hip_model(arch, params)
    rec, loss, grads = _round_trip(m, arch, x, eps, x2, eps2, 7, 5)
    assert all(torch.equal(a, b) for a, b in zip(rec, r0))
    assert torch.equal(loss, l0.detach()) and all(torch.equal(a, b) for a, b in zip(grads, g0))
    # graph mode: the shapes alternate, each one's graphs are captured and replayed; results bitwise those of the eager path
    e2 = make_hip_model(arch, params)
    e2.K, e2.n_iters = 7, 5
    r2 = [t.clone() for t in e2.reconstruct(x2.to(DEV), eps2.to(DEV))]
    mg = make_hip_model(arch, params)
    mg.set_option('graph', 1)
    with torch.cuda.stream(torch.cuda.Stream()):
        for _ in range(3):
            rec, loss, grads = _round_trip(mg, arch, x, eps, x2, eps2, 7, 5)
            mg.K, mg.n_iters = 7, 5
            rk = mg.reconstruct(x2.to(DEV), eps2.to(DEV))
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(rec, r0))
            assert torch.equal(loss, l0.detach()) and all(torch.equal(a, b) for a, b in zip(grads, g0))
            assert all(torch.equal(a, b) for a, b in zip(rk, r2))
    assert mg.profile_read('graph_replays')[1] > 0
