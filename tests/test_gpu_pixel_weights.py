"""Per-pixel observation weights on the device: ``weights=`` of forward / encode / reconstruct, ``weighted_elbo`` and engine.clip_backward, handed to the
library through iodine_set_pixel_weights (one-shot) and packed into lane 3 of the image the pixel kernels read.

Ground truth: the float64 run of tests/weights_reference.py (the oracle's pieces with ``w`` as an argument; test_pixel_weights_cpu pins it to
the oracle at w = 1 and shows that the weight pattern tells the wrong compositions apart by >= 10 x these gates).  Gates are the project's
own: parameter-gradient rel-L2 < 1e-3 per tensor (util.grad_views for the mask-logit bias), loss / ELBO terms 1e-4 relative
(tests/test_gpu_train.py, test_gpu_objective.py); inference tensors at the tolerances of tests/test_gpu_reconstruct.py / test_gpu_refl0.py
(ELBO terms and the posterior 1e-4, images and masks 2e-4); chunked against unchunked 1e-5 (test_gpu_objective.py); "bitwise" is torch.equal.

All cases run the tiny architecture (K = 3, T = 2, S = 16, L = 8, B = 2) unless the case is about another shape; the fused first
refinement layer needs tiny_arch(3, 2, 32, chan=64).

What a zero weight takes out is the OBJECTIVE: the image channels of the refinement input and its likelihood-shaped channels stay
unweighted by design, so the pixels under a zero weight still reach the refinement network as input.  The "zeros" tests therefore compare
bit for bit (a) a single weighted_elbo() - value and every gradient - and evaluation 0 of a training step at the full encoding, and (b) the WHOLE
training step at an encoding without the channels that read x unweighted (image, mask_posterior, likelihood, leave_one_out_likelihood)."""
import dataclasses
import functools

import pytest
import torch

from iodine_amd.engine import clip_backward
from iodine_amd.model import logger
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

import weights_reference as W
from clip_reference import moving_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE, VGATE = 1e-3, 1e-4
BASE = O.tiny_arch()
B = 2
T = BASE.iters
ARCHS = {
    'tiny': BASE,
    'generic': dataclasses.replace(BASE, ref_kernel=5, dec_kernel=5),       # kernels = (5, 5): the generic path
    'padded': dataclasses.replace(BASE, dim_latent=6),                      # L = 6: a padded inner handle
    'fused': O.tiny_arch(3, 2, 32, chan=64),                                # the smallest shape that runs refine_l0_fused
    # no channel of the refinement input reads x except through the weighted gradients
    'objective_only': dataclasses.replace(BASE, encoding=tuple(e for e in O.FULL_ENCODING if e not in (
        'image', 'mask_posterior', 'likelihood', 'leave_one_out_likelihood'))),
}


@functools.lru_cache(maxsize=None)
def _inputs(arch_key):
    a = ARCHS[arch_key]
    params, x, eps = W.inputs(a, B)
    return params, x, eps, W.pattern(B, a.img_size)


def _p64(params):
    return {k: v.double() for k, v in params.items()}


@functools.lru_cache(maxsize=None)
def _ref_step(arch_key):
    """float64 training step of the reference under the pattern, computed once per architecture"""
    params, x, eps, w = _inputs(arch_key)
    return W.train_step_grads(x.double(), w, eps.double(), _p64(params), ARCHS[arch_key])


@functools.lru_cache(maxsize=None)
def _ref_recon(arch_key):
    params, x, eps, w = _inputs(arch_key)
    return W.reconstruct(x.double(), w, eps.double(), _p64(params), ARCHS[arch_key])


def _train_step(m, x, eps, w=None, **kw):
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV), weights=None if w is None else w.to(DEV), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss


def _check_step(m, loss, out, grads, tag):
    ref_loss = out['loss'].item()
    terms = m.elbo_terms.cpu()
    errs = {n: rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy())) for n, p in m.named_parameters()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f'[{tag}] loss {loss.item():.6f} vs {ref_loss:.6f}; elbo {rel_err(terms[:, 0], out["elbos"]):.1e} kl {rel_err(terms[:, 1], out["kls"]):.1e} '
          f'll {rel_err(terms[:, 2], out["lls"]):.1e}; worst gradient {worst[0]} {worst[1]:.2e}')
    assert abs(loss.item() - ref_loss) <= VGATE * abs(ref_loss)
    assert rel_err(terms[:, 0], out['elbos']) < VGATE
    assert rel_err(terms[:, 1], out['kls']) < VGATE
    assert rel_err(terms[:, 2], out['lls']) < VGATE
    bad = [(n, e) for n, e in errs.items() if not e < GATE]
    assert not bad, (tag, bad)


def _check_recon(m, outs, ref, tag):
    pred, mask, mean = outs
    terms = m.elbo_terms.cpu()
    errs = dict(elbo=rel_err(terms[:, 0], ref['elbos']), kl=rel_err(terms[:, 1], ref['kls']), ll=rel_err(terms[:, 2], ref['lls']),
                post_mean=rel_err(m.posterior.mean.cpu(), ref['post_mean']), post_logvar=rel_err(m.posterior.logvar.cpu(), ref['post_logvar']),
                pred=rel_err(pred.cpu(), ref['pred']), mask=rel_err(mask.cpu(), ref['mask']), mean=rel_err(mean.cpu(), ref['mean']))
    print(f'[{tag}] ' + ' '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    for k in ('elbo', 'kl', 'll', 'post_mean', 'post_logvar'):
        assert errs[k] < 1e-4, (k, errs[k])
    for k in ('pred', 'mask', 'mean'):
        assert errs[k] < 2e-4, (k, errs[k])


def _snapshot(m, x, eps, w=None):
    """everything a training step and a reconstruct hand their caller"""
    loss = _train_step(m, x, eps, w)
    out = dict(loss=loss.detach().clone(), terms=m.elbo_terms.clone())
    out.update({'g.' + n: p.grad.clone() for n, p in m.named_parameters()})
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV), weights=None if w is None else w.to(DEV))
    out.update(pred=pred, mask=mask, mean=mean, pm=m.posterior.mean.clone(), plv=m.posterior.logvar.clone(), rterms=m.elbo_terms.clone())
    return out


def _differ(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


# ---- 1. training step vs the float64 reference --------------------------------------------------------------------------------------
STEP_CASES = {
    'split_f16x3': ('tiny', {'conv_precision': 1}), 'exact_fp32': ('tiny', {'conv_precision': 0}),
    'fuse_l0=0': ('tiny', {'fuse_l0': 0}), 'head_fused=0': ('tiny', {'head_fused': 0}), 'wgrad_accum=1': ('tiny', {'wgrad_accum': 1}),
    'generic': ('generic', {}), 'padded': ('padded', {}),
}


@pytest.mark.parametrize('case', list(STEP_CASES))
def test_training_step_matches_reference(case):
    arch_key, options = STEP_CASES[case]
    params, x, eps, w = _inputs(arch_key)
    m = make_hip_model(ARCHS[arch_key], params, options=options)
    loss = _train_step(m, x, eps, w)
    _check_step(m, loss, *_ref_step(arch_key), case)
    assert torch.equal(logger['likelihood'], m.elbo_terms[-1, 2])           # the logger's likelihood is the weighted one


def test_weight_dtypes_and_shapes_are_the_same_call():
    """(B, S, S), float64, and a bool mask against its float form: bit for bit what the (B, 1, S, S) float32 tensor computes"""
    params, x, eps, w = _inputs('tiny')
    m = make_hip_model(BASE, params)
    a = _snapshot(m, x, eps, w.float())
    assert not _differ(a, _snapshot(m, x, eps, w.float()[:, 0]))
    assert not _differ(a, _snapshot(m, x, eps, w.float().double()))
    keep = w > 0.8
    assert not _differ(_snapshot(m, x, eps, keep), _snapshot(m, x, eps, keep.float()))
    assert _differ(a, _snapshot(m, x, eps, keep))


# ---- 2. the fused first refinement layer -------------------------------------------------------------------------------------------
def test_fused_first_layer_under_weights():
    arch = ARCHS['fused']
    params, x, eps, w = _inputs('fused')
    xd, ed, wd = x.to(DEV), eps.to(DEV), w.to(DEV)
    enc = {}
    for fused in (1, 0):
        m = make_hip_model(arch, params, options={'refine_l0_fused': fused})
        loss = _train_step(m, x, eps, w)
        _check_step(m, loss, *_ref_step('fused'), f'refine_l0_fused={fused}')
        outs = m.reconstruct(xd, ed, weights=wd)
        _check_recon(m, outs, _ref_recon('fused'), f'reconstruct, refine_l0_fused={fused}')
        m.set_option('stop_after_iters', 1)                                 # (debug runs materialise the encoding in both forms)
        m.reconstruct(xd, ed, weights=wd)
        enc[fused] = m.debug_buffer('enc').cpu().clone()
        m.set_option('stop_after_iters', -1)
    assert torch.equal(enc[1], enc[0])                                      # one definition of the per-pixel terms: bitwise
    m.set_option('stop_after_iters', 1)
    m.reconstruct(xd, ed)
    assert not torch.equal(m.debug_buffer('enc').cpu(), enc[0])             # ... and the weights are in it


# ---- 3. exactness: no weights = weights of ones -----------------------------------------------------------------------------------
@pytest.mark.parametrize('arch_key', ['tiny', 'fused'])
def test_unit_weights_change_no_bit(arch_key):
    params, x, eps, _ = _inputs(arch_key)
    S = ARCHS[arch_key].img_size
    a = _snapshot(make_hip_model(ARCHS[arch_key], params), x, eps)
    b = _snapshot(make_hip_model(ARCHS[arch_key], params), x, eps, torch.ones(B, 1, S, S))
    assert not _differ(a, b)
    out, grads = W.train_step_grads(x.double(), torch.ones(B, 1, S, S, dtype=torch.float64), eps.double(), _p64(params), ARCHS[arch_key])
    assert abs(b['loss'].item() - out['loss'].item()) <= VGATE * abs(out['loss'].item())       # (and they are the oracle's numbers)


# ---- 4. zeros -----------------------------------------------------------------------------------------------------------------------
def _flip_inside_rectangles(x):
    x2 = x.clone()
    for i, (y0, x0) in enumerate(W.rectangles(x.shape[0], x.shape[-1])):
        x2[i, :, y0:y0 + 6, x0:x0 + 5] = 1.0 - x2[i, :, y0:y0 + 6, x0:x0 + 5]
    return x2


def test_pixels_of_zero_weight_do_not_reach_the_objective():
    params, x, eps, w = _inputs('tiny')
    x2 = _flip_inside_rectangles(x)
    # (a) full encoding: one elbo() - value and every gradient - and evaluation 0 of a training step
    res = []
    for v in (x, x2):
        m = make_hip_model(BASE, params)
        m.zero_grad(set_to_none=True)
        e = m.weighted_elbo(v.to(DEV), w.to(DEV), eps[0].to(DEV), differentiable=True)
        e.backward()
        snap = dict(elbo=e.detach().clone(), terms=m.elbo_terms.clone())
        snap.update({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
        _train_step(m, v, eps, w)
        snap['step0'] = m.elbo_terms[0].clone()
        res.append(snap)
    assert len(res[0]) > 4 and not _differ(res[0], res[1])
    with torch.no_grad():                                                   # ... which unweighted they do change
        m = make_hip_model(BASE, params)
        assert not torch.equal(m.elbo(x.to(DEV), eps[0].to(DEV)), m.elbo(x2.to(DEV), eps[0].to(DEV)))
    # (b) an encoding that reads x through the weighted gradients only: the whole step, loss and gradients
    a = ARCHS['objective_only']
    params, x, eps, w = _inputs('objective_only')
    x2 = _flip_inside_rectangles(x)
    m = make_hip_model(a, params)
    l1 = _train_step(m, x, eps, w)
    _check_step(m, l1, *_ref_step('objective_only'), 'objective-only encoding')
    g1 = {n: p.grad.clone() for n, p in m.named_parameters()}
    t1 = m.elbo_terms.clone()
    l2 = _train_step(m, x2, eps, w)
    assert torch.equal(l1, l2) and torch.equal(t1, m.elbo_terms)
    assert not [n for n, p in m.named_parameters() if not torch.equal(p.grad, g1[n])]
    l3 = _train_step(m, x2, eps, w + 1e-3)                                  # the same change under a weight that is not zero is seen
    assert not torch.equal(l1, l3)


def test_an_image_of_all_zero_weights():
    """finite outputs, no log-likelihood, and the other image of the batch computes what it computes alone"""
    params, x, eps, w = _inputs('tiny')
    w = w.float().clone()
    w[1] = 0.0
    m = make_hip_model(BASE, params)
    outs = m.reconstruct(x.to(DEV), eps.to(DEV), weights=w.to(DEV), trajectory=True)
    both = dict(pred=outs[0], mask=outs[1], mean=outs[2], pm=m.posterior.mean, plv=m.posterior.logvar, z=m.z)
    assert all(bool(torch.isfinite(t).all()) for t in both.values()) and bool(torch.isfinite(m.elbo_terms).all())
    ll = m.trajectory['ll'].clone()
    assert float(ll[:, 1].abs().max()) == 0.0 and float(ll[:, 0].abs().min()) > 0.0
    loss = _train_step(m, x, eps, w)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    outs1 = m.reconstruct(x[:1].to(DEV), eps[:, :1].to(DEV), weights=w[:1].to(DEV), trajectory=True)
    alone = dict(pred=outs1[0], mask=outs1[1], mean=outs1[2], pm=m.posterior.mean, plv=m.posterior.logvar, z=m.z)
    differ = [k for k in both if not torch.equal(both[k][:1], alone[k])]
    assert not differ, differ
    assert torch.equal(ll[:, :1], m.trajectory['ll'])


# ---- 5. clips ----------------------------------------------------------------------------------------------------------------------
def test_per_frame_weights_of_a_clip_match_reference():
    params, x, eps, _ = _inputs('tiny')
    clip = moving_clip(x, T + 1)
    w5 = W.clip_pattern(B, T + 1, BASE.img_size)
    out, grads = W.train_step_grads(clip.double(), w5, eps.double(), _p64(params), BASE)
    m = make_hip_model(BASE, params)
    loss = _train_step(m, clip, eps, w5)
    _check_step(m, loss, out, grads, 'clip, per-frame weights')
    g = {n: p.grad.clone() for n, p in m.named_parameters()}
    l4 = _train_step(m, clip, eps, w5[:, :, 0])                             # (B, E, S, S): the same call
    assert torch.equal(loss, l4) and all(torch.equal(p.grad, g[n]) for n, p in m.named_parameters())
    ref = W.reconstruct(clip[:, :T].double(), w5[:, :T], eps.double(), _p64(params), BASE)
    outs = m.reconstruct(clip[:, :T].contiguous().to(DEV), eps.to(DEV), weights=w5[:, :T].to(DEV))
    _check_recon(m, outs, ref, 'reconstruct of a clip, per-frame weights')


def test_a_4d_weight_is_its_broadcast_over_the_frames():
    params, x, eps, w = _inputs('tiny')
    m = make_hip_model(BASE, params)
    for E in (T + 1, T):
        clip = moving_clip(x, E)
        full = w[:, None].expand(B, E, 1, BASE.img_size, BASE.img_size).contiguous()
        if E == T + 1:
            la = _train_step(m, clip, eps, w)
            ga = [p.grad.clone() for p in m.parameters()]
            lb = _train_step(m, clip, eps, full)
            assert torch.equal(la, lb) and all(torch.equal(u, p.grad) for u, p in zip(ga, m.parameters()))
        else:
            a = m.reconstruct(clip.to(DEV), eps.to(DEV), weights=w.to(DEV)) + (m.posterior.mean, m.elbo_terms)
            b = m.reconstruct(clip.to(DEV), eps.to(DEV), weights=full.to(DEV)) + (m.posterior.mean, m.elbo_terms)
            assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_a_clip_continued_from_a_state_under_weights():
    params, x, eps, _ = _inputs('tiny')
    clip = moving_clip(x, 2 * T)
    w5 = W.clip_pattern(B, 2 * T, BASE.img_size)
    eps2 = W.inputs(BASE, B, seed=W.SEED + 10)[2]
    p64 = _p64(params)
    r1 = W.reconstruct(clip[:, :T].double(), w5[:, :T], eps.double(), p64, BASE)
    r2 = W.reconstruct(clip[:, T:].double(), w5[:, T:], eps2.double(), p64, BASE, init=r1['state'])
    m = make_hip_model(BASE, params)
    m.reconstruct(clip[:, :T].contiguous().to(DEV), eps.to(DEV), weights=w5[:, :T].to(DEV))
    outs = m.reconstruct(clip[:, T:].contiguous().to(DEV), eps2.to(DEV), state=m.refinement_state(), weights=w5[:, T:].to(DEV))
    _check_recon(m, outs, r2, 'clip + state + weights')


def test_exact_bptt_over_a_weighted_clip_equals_the_one_call_gradient():
    """engine.clip_backward(bptt='exact') re-runs every chunk's forward: each run needs its slice of the weights, boundary frame included.
    Against ONE forward over all 2 T + 1 frames on the device, at the gate of the clip tests (rel-L2 < 1e-3 per tensor), and against the
    float64 reference of that forward."""
    params, x, _, _ = _inputs('tiny')
    F = 2 * T + 1
    clip = moving_clip(x, F)
    w5 = W.clip_pattern(B, F, BASE.img_size)
    wc = (0.2, 0.3, 0.5)
    long_arch = dataclasses.replace(BASE, iters=2 * T)
    eps = W.inputs(long_arch, B)[2]
    m = make_hip_model(BASE, params)
    m.iter_weights = wc
    m.zero_grad(set_to_none=True)
    loss, terms = clip_backward(m, clip.to(DEV), eps.to(DEV), bptt='exact', weights=w5.to(DEV))
    torch.cuda.synchronize()
    one = make_hip_model(BASE, params)
    one.n_iters, one.iter_weights = 2 * T, wc + wc[1:]
    l1 = _train_step(one, clip, eps, w5)
    assert torch.equal(terms, one.elbo_terms) and abs(loss.item() - l1.item()) <= 1e-6 * abs(l1.item())
    errs = {n: rel_l2(*grad_views(n, p.grad.cpu().numpy(), q.grad.cpu().numpy()))
            for (n, p), (_, q) in zip(m.named_parameters(), one.named_parameters())}
    print('[exact BPTT vs one call] worst', max(errs.items(), key=lambda kv: kv[1]))
    assert all(e < GATE for e in errs.values()), errs
    out, grads = W.train_step_grads(clip.double(), w5, eps.double(), _p64(params), long_arch, iw=wc + wc[1:])
    _check_step(one, l1, out, grads, 'the one-call forward vs the reference')
    # the weights of the wrong frames are another gradient: the slicing is what makes the two agree
    m.zero_grad(set_to_none=True)
    clip_backward(m, clip.to(DEV), eps.to(DEV), bptt='exact', weights=w5.flip(1).to(DEV))
    assert max(rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy()) for p, q in zip(m.parameters(), one.parameters())) > 10 * GATE


# ---- 6. other entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('given', [False, True], ids=['initial_posterior', 'given_posterior'])
def test_elbo_value_and_gradients_match_reference(given):
    params, x, eps, w = _inputs('tiny')
    p64 = _p64(params)
    pm = plv = None
    if given:
        rec = _ref_recon('tiny')
        pm, plv = rec['post_mean'], rec['post_logvar']
    terms, gpm, gplv, gd = W.elbo_grads(x.double(), w, eps[0].double(), p64, BASE, pm, plv)
    m = make_hip_model(BASE, params)
    if given:
        m.posterior.mean = pm.float().to(DEV).requires_grad_(True)
        m.posterior.logvar = plv.float().to(DEV).requires_grad_(True)
    with torch.no_grad():
        plain = m.weighted_elbo(x.to(DEV), w.to(DEV), eps[0].to(DEV))
    t = m.elbo_terms.cpu()[0]
    print(f'[elbo given={given}] {plain.item():.6f} vs {terms["elbo"].item():.6f}')
    assert abs(plain.item() - terms['elbo'].item()) <= VGATE * abs(terms['elbo'].item())
    assert abs(t[1].item() - terms['kl'].item()) <= VGATE * abs(terms['kl'].item())
    assert abs(t[2].item() - terms['ll'].item()) <= VGATE * abs(terms['ll'].item())
    m.zero_grad(set_to_none=True)
    e = m.weighted_elbo(x.to(DEV), w.to(DEV), eps[0].to(DEV), differentiable=True)
    assert torch.equal(e.detach(), plain)
    e.backward()
    torch.cuda.synchronize()
    live = ('decoder.',) if given else ('decoder.', 'posterior.')
    bad = []
    for n, p in m.named_parameters():
        if n.startswith(live):
            err = rel_l2(*grad_views(n, p.grad.cpu().numpy(), gd[n].numpy()))
            if not err < GATE:
                bad.append((n, err))
    if given:
        for n, got, ref in (('posterior.mean', m.posterior.mean.grad, gpm), ('posterior.logvar', m.posterior.logvar.grad, gplv)):
            err = rel_l2(got.cpu().numpy(), ref.numpy())
            if not err < GATE:
                bad.append((n, err))
    assert not bad, bad


def test_reconstruct_and_its_trajectory_match_reference():
    params, x, eps, w = _inputs('tiny')
    ref = _ref_recon('tiny')
    m = make_hip_model(BASE, params)
    outs = m.reconstruct(x.to(DEV), eps.to(DEV), weights=w.to(DEV), trajectory=True)
    _check_recon(m, outs, ref, 'reconstruct')
    ll = m.trajectory['ll'].cpu()
    assert tuple(ll.shape) == (T, B) and rel_err(ll, ref['lls_img']) < VGATE                 # per image: sum_p w_p sum_c ...
    assert rel_err(ll.mean(1), m.elbo_terms.cpu()[:, 2]) < 1e-6
    assert torch.equal(logger['likelihood'], m.elbo_terms[-1, 2])
    z = m.encode(x.to(DEV), eps.to(DEV), weights=w.to(DEV))
    assert rel_err(z.cpu(), ref['z']) < 1e-4


def test_chunked_calls_equal_the_unchunked_ones():
    params, x, eps, w = _inputs('tiny')
    whole = make_hip_model(BASE, params)
    parts = make_hip_model(BASE, params, options={'batch_cap': 1})
    assert parts.max_batch() == 1 and parts.max_batch(training=True) == 1
    a, b = _snapshot(whole, x, eps, w), _snapshot(parts, x, eps, w)
    errs = {k: rel_l2(b[k].cpu().numpy(), a[k].cpu().numpy()) for k in a}
    print('[chunked] worst', max(errs.items(), key=lambda kv: kv[1]))
    assert all(e < 1e-5 for e in errs.values()), errs
    res = []
    for m in (whole, parts):
        m.posterior.mean = m.posterior.logvar = None
        m.zero_grad(set_to_none=True)
        e = m.weighted_elbo(x.to(DEV), w.to(DEV), eps[0].to(DEV), differentiable=True)
        e.backward()
        res.append((e.detach(), m.elbo_terms.clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert abs(res[0][0].item() - res[1][0].item()) <= 1e-5 * abs(res[0][0].item())
    assert rel_err(res[1][1].cpu(), res[0][1].cpu()) < 1e-5
    assert all(rel_l2(res[1][2][n].cpu().numpy(), g.cpu().numpy()) < 1e-5 for n, g in res[0][2].items())


def test_graph_mode_reads_the_staged_weights():
    """eager, captured, replayed: equal results; then another weight tensor of the same shape gives the other, correct answer - the
    captured graph reads the staging buffer, not a stale copy"""
    params, x, eps, w = _inputs('tiny')
    eager, graphed = make_hip_model(BASE, params), make_hip_model(BASE, params, options={'graph': 1})
    w2 = (w.flip(0) * 0.5 + 0.1).contiguous()
    for step, wi in enumerate((w, w, w, w2, w)):
        outs = [_snapshot(m, x, eps, wi.clone()) for m in (eager, graphed)]
        assert not _differ(*outs), step
        if step == 2:
            first = outs[1]
        if step == 3:
            assert not torch.equal(outs[1]['loss'], first['loss']) and not torch.equal(outs[1]['pm'], first['pm'])
            out, grads = W.train_step_grads(x.double(), w2, eps.double(), _p64(params), BASE)
            assert abs(outs[1]['loss'].item() - out['loss'].item()) <= VGATE * abs(out['loss'].item())
            bad = [n for n in grads if not rel_l2(*grad_views(n, outs[1]['g.' + n].cpu().numpy(), grads[n].numpy())) < GATE]
            assert not bad, bad
    assert not _differ(outs[1], first)
    assert graphed.profile_read('graph_replays')[1] > 0


# ---- 7. one-shot -------------------------------------------------------------------------------------------------------------------
def test_weights_hold_for_one_call():
    params, x, eps, w = _inputs('tiny')
    plain = _snapshot(make_hip_model(BASE, params), x, eps)
    m = make_hip_model(BASE, params)
    weighted = _snapshot(m, x, eps, w)
    assert _differ(plain, weighted)
    assert not _differ(plain, _snapshot(m, x, eps))                          # a call with weights, then the calls without
    with torch.no_grad():
        e0 = make_hip_model(BASE, params).elbo(x.to(DEV), eps[0].to(DEV))
        m.posterior.mean = m.posterior.logvar = None
        ew = m.weighted_elbo(x.to(DEV), w.to(DEV), eps[0].to(DEV))
        m.posterior.mean = m.posterior.logvar = None
        assert not torch.equal(ew, e0) and torch.equal(m.elbo(x.to(DEV), eps[0].to(DEV)), e0)
    # the library itself: a pointer set and not renewed is gone after the next call that takes x, a refused one included
    from iodine_amd import _lib
    L, h = _lib.lib(), m._handle
    wd = w.float()[:, 0].contiguous().to(DEV)
    _lib.check(L.iodine_set_pixel_weights(h, _lib.ptr(wd), 0), h, 'iodine_set_pixel_weights')
    assert L.iodine_elbo(h, None, 0, None, None, None, None, None) != 0     # refused on the host (batch 0): it still consumes the weights
    assert not _differ(plain, _snapshot(m, x, eps))
    assert L.iodine_set_pixel_weights(h, _lib.ptr(wd), 1) != 0              # per_frame needs a clip: frames is 0
    assert b'per_frame' in L.iodine_last_error(h)
    assert not _differ(plain, _snapshot(m, x, eps))
