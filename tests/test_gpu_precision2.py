"""Option conv_precision 2 at the handle level: the weight-stationary decoder convs on one fp16 MFMA per product, everything else as
conv_precision 1.  The device is compared with the fp64 oracle (the project's parity budgets: ELBO 1e-3 relative, arg-max masks 99.9 %,
SURVEY.md 8d) AND with the CPU emulation of the mode (tests/f16x1_reference.py): it must be nearer to the rounding model than to the
truth.  Paths the kernel does not run keep the bits of conv_precision 1; switching on a live model returns every setting's first bits."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16x1_reference as R
from iodine_amd import synth
from oracle import iodine_oracle as O
from util import golden_setup, grad_views, load_golden, make_hip_model, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P2 = {'conv_precision': 2}


@functools.lru_cache(maxsize=None)
def _tiny():
    """the ``tiny`` golden's inputs (fp32 and fp64) with the oracle's and the emulation's reconstruct: computed once, read-only"""
    g = load_golden('tiny')
    arch, params, x, eps, _ = golden_setup(g)
    p64 = {k: v.double() for k, v in params.items()}
    ref = O.reconstruct(x.double(), eps.double(), p64, arch)
    emu = R.emulated(O.reconstruct)(x.double(), eps.double(), p64, arch)
    return dict(arch=arch, params=params, p64=p64, x=x, eps=eps, ref=ref, emu=emu)


def _fresh(arch, B, seed):
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    imgs, _ = synth.make_images(B, arch.img_size, seed=seed + 1, kind='blobs')
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=seed + 2))
    return params, torch.from_numpy(imgs), eps


def _assert_reconstruct(m, x, eps, ref, emu, what):
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    elbos = m.elbo_terms[:, 0].cpu().double()
    dev = ((elbos - ref['elbos']).abs() / ref['elbos'].abs()).max().item()
    agree = (mask[:, :, 0].argmax(1).cpu() == ref['mask'][:, :, 0].argmax(1)).double().mean().item()
    print(f'[{what}] ELBO worst evaluation vs fp64 {dev:.2e}, pred max abs {(pred.cpu().double() - ref["pred"]).abs().max():.2e}, '
          f'arg-max agreement {100 * agree:.3f} %')
    assert dev <= 1e-3, dev
    assert agree >= 0.999, agree
    for name, got, key in (('elbos', elbos, 'elbos'), ('pred', pred.cpu(), 'pred'), ('posterior.mean', m.posterior.mean.cpu(), 'post_mean')):
        e_emu, e_ref = rel_err(got, emu[key]), rel_err(got, ref[key])
        print(f'[{what}] {name}: vs emulation {e_emu:.2e}, vs fp64 {e_ref:.2e}')
        assert e_emu < e_ref, (name, e_emu, e_ref)
    return pred, mask, mean


def test_tiny_golden_reconstruct():
    c = _tiny()
    m = make_hip_model(c['arch'], c['params'], options=P2)
    _assert_reconstruct(m, c['x'], c['eps'], c['ref'], c['emu'], 'tiny')


@pytest.mark.parametrize('kw', [dict(dec_layers=3), dict(chan=64)], ids=['dec_layers=3', 'chan=64'])
def test_fresh_inputs_more_layers_and_channels(kw):
    """dec_layers 3: two weight-stationary layers, a kernel's own tmax_out feeds the next; chan 64: the other instantiation"""
    arch = O.tiny_arch(**kw)
    params, x, eps = _fresh(arch, 2, seed=11)
    p64 = {k: v.double() for k, v in params.items()}
    ref = O.reconstruct(x.double(), eps.double(), p64, arch)
    emu = R.emulated(O.reconstruct)(x.double(), eps.double(), p64, arch)
    m = make_hip_model(arch, params, options=P2)
    _assert_reconstruct(m, x, eps, ref, emu, str(kw))


def _render(mean, logits):
    mask = F.softmax(logits, dim=1)
    return (mask * mean).sum(1), mask


def test_decode_and_elbo_on_tiny():
    c = _tiny()
    arch, p64 = c['arch'], c['p64']
    m2 = make_hip_model(arch, c['params'], options=P2)
    m1 = make_hip_model(arch, c['params'])
    z = c['ref']['z'].float()
    ref_pred, ref_mask = _render(*O.decoder(z.double(), p64, arch))
    emu_pred, emu_mask = _render(*R.emulated(O.decoder)(z.double(), p64, arch))
    got, base = m2.decode(z.to(DEV)), m1.decode(z.to(DEV))
    assert not torch.equal(got[0], base[0]) and not torch.equal(got[2], base[2])
    for name, g, e, r in (('pred', got[0], emu_pred, ref_pred), ('mask', got[1], emu_mask, ref_mask)):
        e_emu, e_ref = rel_err(g.cpu(), e), rel_err(g.cpu(), r)
        print(f'[decode] {name}: vs emulation {e_emu:.2e}, vs fp64 {e_ref:.2e}')
        assert e_emu < e_ref, (name, e_emu, e_ref)
    # elbo(x) from the initial posterior
    x, eps0 = c['x'], c['eps'][0]
    B, K = x.shape[0], arch.slots
    pm = p64['posterior.init_mean'][None, None].repeat(B, K, 1)
    plv = p64['posterior.init_logvar'][None, None].repeat(B, K, 1)
    ref = O.elbo_terms(x.double(), pm, plv, eps0.double(), p64, arch)
    emu = R.emulated(O.elbo_terms)(x.double(), pm, plv, eps0.double(), p64, arch)
    e2 = m2.elbo(x.to(DEV), eps0.to(DEV)).item()
    mean2 = m2.mean.cpu()
    e1 = m1.elbo(x.to(DEV), eps0.to(DEV)).item()
    assert e2 != e1 and not torch.equal(mean2, m1.mean.cpu())
    print(f'[elbo] {e2!r}: vs emulation {abs(e2 - emu["elbo"].item()):.3e}, vs fp64 {abs(e2 - ref["elbo"].item()):.3e}; conv_precision 1 {e1!r}')
    assert abs(e2 - emu['elbo'].item()) < abs(e2 - ref['elbo'].item())
    assert rel_err(mean2, emu['mean']) < rel_err(mean2, ref['mean'])


def _train_step(m, x, eps):
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss


def test_training_step_on_tiny():
    """The emulation's own worst tensor is 3.1e-3 from fp64 (refine.lstm.weight_ih): outside the 1e-3 gradient budget by construction, so
    the per-tensor deviations are printed, not gated; the gate is that the device follows the rounding model."""
    c = _tiny()
    arch, p64, x, eps = c['arch'], c['p64'], c['x'], c['eps']
    out, gr = O.train_step_grads(x.double(), eps.double(), p64, arch)
    out16, ge = R.emulated(O.train_step_grads)(x.double(), eps.double(), p64, arch)
    m = make_hip_model(arch, c['params'], options=P2)
    loss = _train_step(m, x, eps)
    assert abs(loss.item() - out['loss'].item()) <= 1e-3 * abs(out['loss'].item())
    names = [n for n, _ in m.named_parameters()]
    got = {n: p.grad.cpu().double().numpy() for n, p in m.named_parameters()}
    for n in names:
        print(f'[train, tiny] {n}: vs fp64 {rel_l2(*grad_views(n, got[n], gr[n].numpy())):.2e}, vs emulation {rel_l2(*grad_views(n, got[n], ge[n].numpy())):.2e}')
    cat = lambda d: np.concatenate([np.asarray(grad_views(n, got[n], np.asarray(d[n]))[1]).ravel() for n in names])
    mine = np.concatenate([np.asarray(grad_views(n, got[n], got[n])[0]).ravel() for n in names])
    e_emu, e_ref = rel_l2(mine, cat(ge)), rel_l2(mine, cat(gr))
    print(f'[train, tiny] loss {loss.item()!r} (fp64 {out["loss"].item()!r}, emulation {out16["loss"].item()!r}); all gradients: vs emulation {e_emu:.2e}, vs fp64 {e_ref:.2e}')
    assert e_emu < e_ref, (e_emu, e_ref)
    # with option graph the step replays and gives the eager step's loss bits
    m.set_option('graph', 1)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(3):                                      # eager, capture, replay
            again = _train_step(m, x, eps)
            assert torch.equal(again.detach(), loss.detach())
    torch.cuda.synchronize()
    assert m.profile_read('graph_replays')[1] > 0


def _bits(m, x, eps):
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    return pred.clone(), mask.clone(), mean.clone(), m.elbo_terms.clone()


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('which', ['img_size=48', 'conv_variant=1'])
def test_paths_without_the_weight_stationary_kernel_keep_the_bits_of_precision_1(which):
    arch = O.tiny_arch(img_size=48) if which == 'img_size=48' else O.tiny_arch()
    extra = {} if which == 'img_size=48' else {'conv_variant': 1}
    params, x, eps = _fresh(arch, 2, seed=23)
    one = _bits(make_hip_model(arch, params, options=dict({'conv_precision': 1}, **extra)), x, eps)
    two = _bits(make_hip_model(arch, params, options=dict(P2, **extra)), x, eps)
    assert _same(one, two)


def test_switching_on_one_model():
    c = _tiny()
    x, eps = c['x'], c['eps']
    m = make_hip_model(c['arch'], c['params'], options={'conv_precision': 1})
    first = {}
    for prec in (1, 2, 1, 0, 2):
        m.set_option('conv_precision', prec)
        got = _bits(m, x, eps)
        if prec in first:
            assert _same(first[prec], got), prec
        first[prec] = got
    assert not _same(first[1], first[2]) and not _same(first[0], first[2]) and not _same(first[0], first[1])
    assert _same(first[2], _bits(make_hip_model(c['arch'], c['params'], options=P2), x, eps))
    with pytest.raises(RuntimeError):
        m.set_option('conv_precision', 3)
    m.set_option('conv_precision', 2)                          # (the wrapper records the refused value: set a valid one again)

    # a switch between the forward and the backward of a differentiable decode: what a 0 <-> 1 switch does, refused or correct
    def switched(a, b):
        m.set_option('conv_precision', a)
        z = c['ref']['z'].float().to(DEV).requires_grad_(True)
        pred, _, _ = m.decode(z)
        m.set_option('conv_precision', b)
        try:
            pred.square().sum().backward()
        except RuntimeError as e:
            return ('refused', str(e))
        return ('ran', z.grad.clone())
    m.set_option('conv_precision', 2)
    z = c['ref']['z'].float().to(DEV).requires_grad_(True)
    m.decode(z)[0].square().sum().backward()
    want = z.grad.clone()
    today, now = switched(0, 1), switched(2, 1)
    print('[switch between forward and backward] 0 -> 1:', today[0], '| 2 -> 1:', now[0])
    assert now[0] == today[0]
    if now[0] == 'ran':
        assert torch.equal(now[1], want)
    m.set_option('conv_precision', 2)
    assert _same(first[2], _bits(m, x, eps))                   # ... and the model is usable afterwards


def test_predictive_and_edit_keep_their_invariants():
    c = _tiny()
    arch = c['arch']
    m = make_hip_model(arch, c['params'], options=P2)
    x = c['x'].to(DEV)
    m.reconstruct(x, c['eps'].to(DEV))
    post = (m.posterior.mean.clone(), m.posterior.logvar.clone())
    B, K, L = post[0].shape
    g = torch.Generator().manual_seed(3)
    eps = torch.randn(4, B, K, L, generator=g).to(DEV)
    full = m.predictive(x, samples=4, posterior=post, eps=eps)
    try:
        m.set_option('batch_cap', B)                            # four chunks of one sample
        part = m.predictive(x, samples=4, posterior=post, eps=eps)
    finally:
        m.set_option('batch_cap', 0)
    for f in ('pred_mean', 'pred_var', 'votes', 'll'):
        assert torch.equal(getattr(full, f), getattr(part, f)), f
    # each sample's image is the bits decode(z[s]) returns
    assert torch.equal(m.decode(full.z[0])[0], m.decode(full.z[0].clone())[0])
    # edit == decode of the edited scene, bitwise
    z = m.z.clone()
    image, slot = [0, B - 1], [0, K - 1]
    zn = torch.randn(2, L, generator=g).to(DEV)
    out = m.edit(z, image, slot, zn, return_mask=True, return_mean=True)
    ze = z[torch.as_tensor(image, device=z.device)].clone()
    ze[torch.arange(2), torch.as_tensor(slot)] = zn
    pred, mask, mean = m.decode(ze)
    assert torch.equal(out.pred, pred) and torch.equal(out.mask, mask) and torch.equal(out.mean, mean[torch.arange(2), torch.as_tensor(slot)])
    assert not torch.equal(pred, make_hip_model(arch, c['params']).decode(ze)[0])   # ... at precision 2
