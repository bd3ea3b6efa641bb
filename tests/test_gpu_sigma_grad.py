"""A differentiable ``model.sigma`` (option sigma_grad, iodine_last_sigma_grad) and ``model.stable_encoding`` on the device.

Ground truth: the float64 run of tests/sigma_reference.py (sigma a tensor autograd sees; test_sigma_grad_cpu pins its closed form to
autograd).  Gates are the project's own (tests/test_gpu_objective.py): gradients - the parameters' rel-L2 per tensor, sigma's relative error -
below GATE = 1e-3, values below VGATE = 1e-4; "bitwise" is torch.equal.  Every sigma-gradient comparison first asserts that the reference
scalar is not a cancellation: the sum of g1 (x - mu) is at least twice 3 x the sum of the pixel weights.

Worst figures measured on an MI355X (all cases of this file): sigma.grad 6.4e-7 relative (K = 16; 1.8e-9 on the exact-fp32 path), parameter
gradients 2.8e-6 rel-L2 (K = 16), loss 4.1e-7 (dSprites architecture); elbo: sigma.grad 9.7e-8, parameters 4.6e-7; stable mode on the pinned
scene: encoding channels 2.2e-5 at worst (layer-normed mask gradient; channel 8 5.5e-6), pred / mask / mean / posterior / loss <= 1.1e-6;
channel 8 of stable against plain mode on ordinary inputs 1.8e-7, pred / mask / mean / posterior of either mode there <= 3.8e-6.  The cancellation ratio of the reference scalars is 2.09 .. 12.6."""
import dataclasses
import functools
import math

import pytest
import torch

from iodine_amd import _lib
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

import sigma_reference as R
import weights_reference as W
from clip_reference import moving_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE, VGATE = 1e-3, 1e-4
BASE = O.tiny_arch()                                            # S = 16, K = 3, T = 2
B = 2
SIGMA = float(torch.tensor(0.1, dtype=torch.float32))           # the float32 value a device tensor holds
SIGMA_K16 = float(torch.tensor(0.05, dtype=torch.float32))      # sixteen slots fit the blobs closely: at 0.1 the cancellation ratio is 1.7,
                                                                # below the precondition; 2.09 at 0.05 (the float32 oracle stays finite there)

ARCHS = {
    'tiny': BASE,
    'k1': dataclasses.replace(BASE, slots=1),
    'k16': dataclasses.replace(BASE, slots=16),                 # the statistic count of pass 1 at its bound
    's12': dataclasses.replace(BASE, img_size=12),              # generic path; P = 144 is no multiple of 64: partial waves
    'dsprites': O.dsprites_arch(slots=4, iters=2),              # 64 px, 32 channels: split first layer
    'padded': dataclasses.replace(BASE, dim_latent=6),          # a padded inner handle
}


@functools.lru_cache(maxsize=None)
def _inputs(arch_key):
    return R.inputs(ARCHS[arch_key], B)


def _pixel_w(arch_key):
    return W.pattern(B, ARCHS[arch_key].img_size)


@functools.lru_cache(maxsize=None)
def _state(arch_key):
    """a carried state: (post_mean, post_logvar, h, c) after the T iterations of a float64 reconstruct-like loop"""
    a = ARCHS[arch_key]
    params, x, eps = _inputs(arch_key)
    p64 = {k: v.double() for k, v in params.items()}
    pm, plv, hidden, _, _ = R.s_loop(x.double(), None, eps.double(), p64, a, False, R.as_sigma(SIGMA))
    return (pm.detach(), plv.detach(), hidden[0].reshape(B, a.slots, -1), hidden[1].reshape(B, a.slots, -1))


# name -> (architecture, keywords of the reference, how the module is called)
CASES = {
    'base': ('tiny', {}, {}),
    'k1': ('k1', {}, {}),
    'k16': ('k16', dict(sigma=SIGMA_K16), {}),
    's12_generic': ('s12', {}, {}),
    'dsprites': ('dsprites', {}, {}),
    'padded_l6': ('padded', {}, {}),
    'pixel_weights': ('tiny', dict(w=True), {}),
    'iw_beta': ('tiny', dict(iw=(0.5, 0.0, 2.0), beta=0.5), {}),
    'clip': ('tiny', dict(clip=True), {}),
    'from_state': ('tiny', dict(state=True), {}),
    'chunked': ('tiny', {}, dict(options={'batch_cap': 1})),
}


@functools.lru_cache(maxsize=None)
def _reference(case):
    arch_key, kw, _ = CASES[case]
    a = ARCHS[arch_key]
    params, x, eps = _inputs(arch_key)
    p64 = {k: v.double() for k, v in params.items()}
    x64 = x.double()
    if kw.get('clip'):
        x64 = moving_clip(x64, a.iters + 1)
    return R.train_step_grads(x64, eps.double(), p64, a, kw.get('sigma', SIGMA), beta=kw.get('beta', 1.0), iw=kw.get('iw'),
                              w=_pixel_w(arch_key) if kw.get('w') else None, init=_state(arch_key) if kw.get('state') else None)


def _model(case, options=None):
    arch_key, kw, how = CASES[case]
    params, _, _ = _inputs(arch_key)
    m = make_hip_model(ARCHS[arch_key], params, options={**how.get('options', {}), **(options or {})})
    m.beta, m.iter_weights = kw.get('beta', 1.0), kw.get('iw')
    return m


def _call(case, m, sigma, **fwd):
    """one training step of ``case`` with ``m.sigma = sigma`` -> loss"""
    arch_key, kw, _ = CASES[case]
    a = ARCHS[arch_key]
    _, x, eps = _inputs(arch_key)
    x = moving_clip(x, a.iters + 1) if kw.get('clip') else x
    if kw.get('w'):
        fwd['weights'] = _pixel_w(arch_key).float().to(DEV)
    if kw.get('state'):
        fwd['state'] = tuple(t.float().to(DEV) for t in _state(arch_key))
    m.sigma = sigma
    m.zero_grad(set_to_none=True)
    return m(x.to(DEV), eps.to(DEV), **fwd)


def _sigma_leaf(case='base'):
    return torch.tensor(CASES[case][1].get('sigma', SIGMA), dtype=torch.float32, device=DEV, requires_grad=True)


def _check(case, m, loss, s, tag):
    out, grads, g_auto, g_closed = _reference(case)
    assert out['ratio'] >= 2.0, (tag, out['ratio'])                     # precondition: not a cancellation
    ref_loss = out['loss'].item()
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy())), n) for n, p in m.named_parameters() if p.grad is not None)
    es = abs(s.grad.item() - g_auto.item()) / abs(g_auto.item())
    print(f'[{tag}] ratio {out["ratio"]:.2f}; loss {loss.item():.6f} vs {ref_loss:.6f}; sigma.grad {s.grad.item():.6f} vs {g_auto.item():.6f} '
          f'rel {es:.2e}; worst parameter gradient {worst[1]} {worst[0]:.2e}')
    assert abs(loss.item() - ref_loss) <= VGATE * abs(ref_loss), tag
    assert es < GATE, (tag, s.grad.item(), g_auto.item())
    assert worst[0] < GATE, (tag, worst)


# ---- 1. sigma.grad of a training step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [1, 0], ids=['split_f16x3', 'exact_fp32'])
def test_base_case_both_precisions_and_detached_sigma_is_bitwise_the_same_step(prec):
    """measured: sigma.grad 7.5e-8 (split-fp16) / 1.8e-9 (exact fp32) relative; the loss and every parameter gradient are the bits of the same
    call with a float sigma, and a non-leaf sigma (log_sigma.exp()) hands log_sigma sigma x the same gradient"""
    m = _model('base', {'conv_precision': prec})
    s = _sigma_leaf()
    loss = _call('base', m, s)
    loss.backward()
    _check('base', m, loss, s, f'base prec {prec}')
    got = (loss.detach().clone(), m.elbo_terms.clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    m2 = _model('base', {'conv_precision': prec})
    l2 = _call('base', m2, SIGMA)
    l2.backward()
    assert torch.equal(l2.detach(), got[0]) and torch.equal(m2.elbo_terms, got[1])
    assert all(torch.equal(p.grad, got[2][n]) for n, p in m2.named_parameters())
    # ... and on the SAME handle: the option goes off again with a sigma that does not require grad
    l3 = _call('base', m, s.detach())
    l3.backward()
    assert torch.equal(l3.detach(), got[0]) and all(torch.equal(p.grad, got[2][n]) for n, p in m.named_parameters())
    assert _lib.lib().iodine_last_sigma_grad(m._handle, None, _lib.ptr(torch.empty(3, device=DEV)), 3) == 3       # IODINE_ERR_STATE
    log_sigma = torch.tensor(math.log(0.1), dtype=torch.float32, device=DEV, requires_grad=True)
    l4 = _call('base', m, log_sigma.exp())
    l4.backward()
    assert abs(log_sigma.grad.item() - m.sigma.item() * s.grad.item()) <= 1e-5 * abs(log_sigma.grad.item())


@pytest.mark.parametrize('case', [c for c in CASES if c != 'base'])
def test_sigma_grad_of_a_training_step(case):
    m = _model(case)
    s = _sigma_leaf(case)
    assert s.item() == CASES[case][1].get('sigma', SIGMA)
    loss = _call(case, m, s)
    loss.backward()
    torch.cuda.synchronize()
    _check(case, m, loss, s, case)


def test_auxiliary_cotangents_leave_sigma_grad_unchanged():
    """attach_state with a mask cotangent and attach_frames = [0, T]: mean, mask, z and the state do not depend on sigma (the float64
    reference shows exactly zero: test_sigma_grad_cpu), so sigma.grad is the bits of the plain step"""
    m = _model('base')
    s = _sigma_leaf()
    loss = _call('base', m, s)
    loss.backward()
    plain = s.grad.clone()
    s.grad = None
    T = BASE.iters
    loss = _call('base', m, s, attach_state=True, attach_frames=[0, T])
    g = torch.Generator().manual_seed(3)
    wm = torch.randn(m.mask.shape, generator=g).to(DEV)
    aux = (wm * m.mask).sum() + (m.frames['mask'][0] ** 2).sum() + m.frames['z'][1].sum()
    (loss + aux).backward()
    assert torch.equal(s.grad, plain)
    out, _, g_auto, _ = _reference('base')
    assert abs(s.grad.item() - g_auto.item()) < GATE * abs(g_auto.item())


def test_graph_mode_for_three_steps():
    eager, graphed = _model('base'), _model('base', {'graph': 1})
    for step in range(3):                                                   # eager, captured, replayed
        outs = []
        for m in (eager, graphed):
            s = _sigma_leaf()
            loss = _call('base', m, s)
            loss.backward()
            torch.cuda.synchronize()
            outs.append((loss.detach().clone(), s.grad.clone(), [p.grad.clone() for p in m.parameters()]))
        (l0, s0, g0), (l1, s1, g1) = outs
        assert torch.equal(l0, l1) and torch.equal(s0, s1), step
        assert all(torch.equal(u, v) for u, v in zip(g0, g1)), step
    assert graphed.profile_read('graph_replays')[1] > 0
    _check('base', graphed, l1, s, 'graph')


# ---- 2. elbo / weighted_elbo --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['elbo', 'weighted', 'chunked'])
def test_sigma_grad_of_elbo(how):
    params, x, eps = _inputs('tiny')
    p64 = {k: v.double() for k, v in params.items()}
    w = _pixel_w('tiny') if how == 'weighted' else None
    terms, grads, g_auto, g_closed, ratio = R.elbo_grads(x.double(), eps[0].double(), p64, BASE, SIGMA, beta=0.5, w=w)
    assert ratio >= 2.0
    m = make_hip_model(BASE, params, options={'batch_cap': 1} if how == 'chunked' else None)
    m.beta = 0.5
    s = _sigma_leaf()
    m.sigma = s
    m.zero_grad(set_to_none=True)
    if w is None:
        e = m.elbo(x.to(DEV), eps[0].to(DEV))
    else:
        e = m.weighted_elbo(x.to(DEV), w.float().to(DEV), eps[0].to(DEV))
    (2.0 * e).backward()
    es = abs(s.grad.item() - 2.0 * g_auto.item()) / abs(2.0 * g_auto.item())
    worst = max(rel_l2(*grad_views(n, p.grad.cpu().numpy(), 2.0 * grads[n].numpy())) for n, p in m.named_parameters() if p.grad is not None)
    print(f'[elbo {how}] ratio {ratio:.2f}; elbo {e.item():.6f} vs {terms["elbo"].item():.6f}; sigma.grad rel {es:.2e}; worst parameter gradient {worst:.2e}')
    assert abs(e.item() - terms['elbo'].item()) <= VGATE * abs(terms['elbo'].item())
    assert es < GATE and worst < GATE
    # a forward that ran without the option left nothing to read
    m.sigma = SIGMA
    m(x.to(DEV), eps.to(DEV))
    assert _lib.lib().iodine_last_sigma_grad(m._handle, None, _lib.ptr(torch.empty(3, device=DEV)), 3) == 3       # IODINE_ERR_STATE
    assert b'sigma_grad' in _lib.lib().iodine_last_error(m._handle)


# ---- 3. stable mode on the pinned 0 / 0 scene ------------------------------------------------------------------------------------------
def _enc17(m, B_, K, S):
    return m.debug_buffer('enc').cpu().view(B_, K, S, S, 20)[..., :17].permute(0, 1, 4, 2, 3)


def test_stable_mode_on_the_pinned_scene():
    arch, params, x, eps = R.pinned_scene()
    p64 = {k: v.double() for k, v in params.items()}
    trace = []
    ref = R.reconstruct(x.double(), eps.double(), p64, arch, arch.sigma, stable=True, trace=trace)
    ref_loss = R.train_forward(x.double(), eps.double(), p64, arch, R.as_sigma(arch.sigma), stable=True)['loss'].item()
    m = make_hip_model(arch, params)
    assert not torch.isfinite(m(x.to(DEV), eps.to(DEV))).item()                  # off: the reference's 0 / 0, as today
    m.stable_encoding = True
    m.set_option('stop_after_iters', 1)
    m.reconstruct(x.to(DEV), eps.to(DEV))
    m.set_option('stop_after_iters', -1)
    Bq, K, S = 2, arch.slots, arch.img_size
    enc, ref_enc = _enc17(m, Bq, K, S), trace[0]['enc']
    assert torch.isfinite(enc).all()
    assert float((enc[:, :, 8].sum(1) - 1).abs().max()) <= 5e-7                  # K = 3 roundings of 2^-24 and the sum's
    errs = {c: rel_err(enc[:, :, c], ref_enc[:, :, c]) for c in range(17)}
    print('[pinned enc] per channel', {c: f'{e:.1e}' for c, e in errs.items()})
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    figs = dict(pred=rel_err(pred.cpu(), ref['pred']), mask=rel_err(mask.cpu(), ref['mask']), mean=rel_err(mean.cpu(), ref['mean']),
                post_mean=rel_err(m.posterior.mean.cpu(), ref['post_mean']), elbos=rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']))
    loss = m(x.to(DEV), eps.to(DEV))
    figs['loss'] = abs(loss.item() - ref_loss) / abs(ref_loss)
    print('[pinned stable]', {k: f'{v:.1e}' for k, v in figs.items()}, 'loss', loss.item(), ref_loss)
    assert all(torch.isfinite(t).all() for t in (pred, mask, mean, m.posterior.mean, loss))
    assert all(e < VGATE for c, e in errs.items()), errs
    assert all(v < VGATE for v in figs.values()), figs


def test_stable_mode_fused_and_unfused_first_layer_agree():
    """the pinned scene at 32 px / 64 channels, where the fused encoding + first layer kernel runs (option refine_l0_fused): one definition
    of the channel, so the encoding is bitwise the same; the rest to the tolerances of tests/test_gpu_refl0.py:74-77"""
    import numpy as np
    from iodine_amd import synth
    arch = O.tiny_arch(slots=3, iters=2, img_size=32, chan=64, mlp=32, ref_layers=2, dec_layers=2)
    pn = synth.make_params(O.param_shapes(arch), seed=5, dec_gain=2.0, posterior_scale=0.05)
    pn['decoder.conv.bias'] = np.array([-6.0, -6.0, -6.0, 0.0], dtype=np.float32)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    x = torch.from_numpy(synth.make_images(2, arch.img_size, seed=3, kind='blobs')[0]) * 0.3
    x[0] = 1.0
    eps = torch.from_numpy(synth.make_eps(arch.iters, 2, arch.slots, arch.dim_latent, seed=4))
    xd, ed = x.to(DEV), eps.to(DEV)
    res = {}
    for fused in (1, 0):
        m = make_hip_model(arch, params, options={'refine_l0_fused': fused})
        if fused:
            m.set_option('stop_after_iters', 1)
            m.reconstruct(xd, ed)
            m.set_option('stop_after_iters', -1)
            assert torch.isnan(m.debug_buffer('enc')).any()                      # the edge is hit at this shape too
        m.stable_encoding = True
        m.set_option('stop_after_iters', 1)
        m.reconstruct(xd, ed)
        enc, act = m.debug_buffer('enc').cpu().clone(), m.debug_buffer('ract0', 0).cpu().clone()
        m.set_option('stop_after_iters', -1)
        pred, _, _ = m.reconstruct(xd, ed)
        m.zero_grad(set_to_none=True)
        loss = m(xd, ed)
        loss.backward()
        assert torch.isfinite(enc).all() and torch.isfinite(pred).all() and torch.isfinite(loss).item()
        res[fused] = (enc, act, pred.cpu(), {n: p.grad.cpu().clone() for n, p in m.named_parameters()})
    assert torch.equal(res[1][0], res[0][0])
    assert rel_err(res[1][1], res[0][1]) < 2e-6
    assert rel_err(res[1][2], res[0][2]) < 1e-4
    for n in res[0][3]:
        assert rel_l2(res[1][3][n].numpy(), res[0][3][n].numpy()) < 1e-4, n


# ---- 4. stable mode on ordinary inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['base', 'dsprites'])
def test_stable_mode_on_ordinary_inputs(case):
    """where nothing underflows the two forms are the same function: stable mode meets the gates against the SAME float64 reference as the
    plain mode, and channel 8 of the two differs by rounding only"""
    arch_key = CASES[case][0]
    a = ARCHS[arch_key]
    _, x, eps = _inputs(arch_key)
    out, grads, _, _ = _reference(case)
    params, _, _ = _inputs(arch_key)
    rec = R.reconstruct(x.double(), eps.double(), {k: v.double() for k, v in params.items()}, a, SIGMA)      # the plain form, float64
    ch8 = {}
    for stable in (False, True):
        m = _model(case)
        m.sigma = SIGMA
        m.stable_encoding = stable
        m.set_option('stop_after_iters', 1)
        m.reconstruct(x.to(DEV), eps.to(DEV))
        m.set_option('stop_after_iters', -1)
        ch8[stable] = _enc17(m, B, a.slots, a.img_size)[:, :, 8].clone()
        pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
        figs = dict(pred=rel_err(pred.cpu(), rec['pred']), mask=rel_err(mask.cpu(), rec['mask']), mean=rel_err(mean.cpu(), rec['mean']),
                    post_mean=rel_err(m.posterior.mean.cpu(), rec['post_mean']), post_logvar=rel_err(m.posterior.logvar.cpu(), rec['post_logvar']),
                    elbos=rel_err(m.elbo_terms[:, 0].cpu(), rec['elbos']))
        print(f'[{case} stable={stable}] reconstruct', {k: f'{v:.1e}' for k, v in figs.items()})
        assert all(v < VGATE for v in figs.values()), (stable, figs)
        loss = _call(case, m, SIGMA)
        loss.backward()
        terms = m.elbo_terms.cpu()
        worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy())), n) for n, p in m.named_parameters())
        print(f'[{case} stable={stable}] loss {loss.item():.6f} vs {out["loss"].item():.6f}; elbos {rel_err(terms[:, 0], out["elbos"]):.1e}; '
              f'worst gradient {worst[1]} {worst[0]:.2e}')
        assert abs(loss.item() - out['loss'].item()) <= VGATE * abs(out['loss'].item())
        assert rel_err(terms[:, 0], out['elbos']) < VGATE and rel_err(terms[:, 2], out['lls']) < VGATE
        assert worst[0] < GATE, worst
    d = rel_err(ch8[True], ch8[False])
    print(f'[{case}] channel 8, stable vs plain: {d:.1e}')
    assert d < 1e-5


# ---- 5. the defaults change no bit ---------------------------------------------------------------------------------------------------
def test_options_off_change_no_bit():
    params, x, eps = _inputs('tiny')

    def snapshot(m):
        m.zero_grad(set_to_none=True)
        loss = m(x.to(DEV), eps.to(DEV))
        loss.backward()
        out = {'loss': loss.detach().clone(), 'terms': m.elbo_terms.clone()}
        out.update({'g.' + n: p.grad.clone() for n, p in m.named_parameters()})
        pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
        out.update(pred=pred.clone(), mask=mask.clone(), mean=mean.clone(), pm=m.posterior.mean.clone(), rterms=m.elbo_terms.clone())
        return out

    a = snapshot(make_hip_model(BASE, params))                              # a handle that never heard of the options
    m = make_hip_model(BASE, params, options={'sigma_grad': 0, 'stable_encoding': 0})
    b = snapshot(m)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, differ
    # ... and a handle that had both on and off again
    m.set_option('sigma_grad', 1)
    m.stable_encoding = True
    snapshot(m)
    m.set_option('sigma_grad', 0)
    m.stable_encoding = False
    c = snapshot(m)
    differ = [k for k in a if not torch.equal(a[k], c[k])]
    assert not differ, differ


# ---- 6. the engine's --learn-sigma ------------------------------------------------------------------------------------------------------
def test_engine_learns_sigma(tmp_path):
    """log_sigma in its own param group of the fused Adam: it moves, the loss falls, the checkpoint carries the entry"""
    import numpy as np
    from iodine_amd import IODINE, engine
    from iodine_amd.checkpoint import load_checkpoint
    from iodine_amd.data import make_dataloader
    from iodine_amd.model import arch_namespace
    from iodine_amd.optim import make_optimizer
    torch.manual_seed(0)
    m = IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))).to(DEV)
    opt = make_optimizer(m, base_lr=3e-3)
    ls = engine.make_log_sigma(m.sigma, torch.device(DEV))
    opt.add_param_group({'params': [ls], 'lr': 3e-3, 'weight_decay': 0.0})
    dl = make_dataloader(engine.SyntheticScenes(8, 16), batch_size=4, shuffle=False)
    ck = str(tmp_path / 'model.pth')
    losses = engine.train(m, opt, dl, torch.device(DEV), max_steps=12, print_every=1000, checkpoint_path=ck, log_sigma=ls)
    assert len(losses) == 12 and np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3])
    assert isinstance(m.sigma, float) and m.sigma != 0.1 and abs(m.sigma - math.exp(ls.item())) < 1e-7
    assert int(opt.state[ls]['step']) == 12
    extra = load_checkpoint(ck, IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))))
    assert torch.equal(extra['log_sigma'], ls.detach().cpu())
