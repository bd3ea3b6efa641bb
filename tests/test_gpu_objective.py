"""Objective controls on the device: ``model.sigma`` (likelihood scale), ``model.beta`` (KL weight) and ``model.iter_weights`` (loss
weights of the T + 1 ELBO evaluations), read when a call starts and handed to the library through iodine_set_objective.

Ground truth: the float64 run of tests/objective_reference.py (the oracle's pieces with the three knobs as arguments; test_objective_cpu pins
it to the oracle at the defaults and shows that these inputs tell wrong compositions apart).  Gates are the project's own: parameter-gradient
rel-L2 < 1e-3 per tensor (util.grad_views for the mask-logit bias), loss / ELBO 1e-4 relative (tests/test_gpu_train.py,
test_gpu_train_aux.py); inference tensors at the tolerances of tests/test_gpu_reconstruct.py; "bitwise" is torch.equal.

All cases run the tiny architecture (K = 3, T = 2, S = 16, L = 8, B = 2) unless the case is about another shape."""
import dataclasses
import functools

import pytest
import torch

from iodine_amd import _args, _lib
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

import aux_reference as A
import objective_reference as R
from clip_reference import moving_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE, VGATE = 1e-3, 1e-4
BASE = O.tiny_arch()
B = 2
S0 = BASE.sigma

# name -> (sigma, beta, iter_weights)
CASES = {
    'sigma0.3': (R.SIGMA, 1.0, None),
    'beta4': (S0, R.BETA, None),
    'beta0': (S0, 0.0, None),
    'uniform': (S0, 1.0, 'uniform'),
    'last': (S0, 1.0, 'last'),
    'w_0_.5_1': (S0, 1.0, (0.0, 0.5, 1.0)),
    'w_1_0_.5': (S0, 1.0, (1.0, 0.0, 0.5)),                  # a zero in the middle
    'w_1_.5_0': (S0, 1.0, (1.0, 0.5, 0.0)),                  # w_T = 0: the last pass still reduces / emits the coordinate and bias gradients
    'all': (R.SIGMA, R.BETA, (0.25, 1.0, 0.5)),
}
ZERO_CASES = ('all', 'last', 'w_1_0_.5', 'w_1_.5_0')          # the combined case and the zero-weight cases: w_0 = 0, a zero inside, w_T = 0
ARCHS = {
    'tiny': BASE,
    'generic': dataclasses.replace(BASE, ref_kernel=5, dec_kernel=5),       # kernels = (5, 5): the generic path
    'padded': dataclasses.replace(BASE, dim_latent=6),                      # L = 6: a padded inner handle
}


@functools.lru_cache(maxsize=None)
def _inputs(arch_key):
    return R.inputs(ARCHS[arch_key], B)


@functools.lru_cache(maxsize=None)
def _reference(arch_key, case):
    """float64 training step of the reference, computed once per (architecture, case)"""
    params, x, eps = _inputs(arch_key)
    sigma, beta, w = CASES[case]
    p64 = {k: v.double() for k, v in params.items()}
    return R.train_step_grads(x.double(), eps.double(), p64, ARCHS[arch_key], sigma, beta, w)


def _set(m, sigma, beta, w):
    m.sigma, m.beta, m.iter_weights = sigma, beta, w
    return m


def _train_step(m, x, eps):
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss


def _check_step(m, loss, out, grads, beta, tag):
    ref_loss = out['loss'].item()
    terms = m.elbo_terms.cpu()
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy())), n) for n, p in m.named_parameters())
    print(f'[{tag}] loss {loss.item():.6f} vs {ref_loss:.6f}; elbo {rel_err(terms[:, 0], out["elbos"]):.1e} kl {rel_err(terms[:, 1], out["kls"]):.1e} '
          f'll {rel_err(terms[:, 2], out["lls"]):.1e}; worst gradient {worst[1]} {worst[0]:.2e}')
    assert abs(loss.item() - ref_loss) <= VGATE * abs(ref_loss)
    assert rel_err(terms[:, 0], out['elbos']) < VGATE                       # column 0: ll - beta * kl
    assert rel_err(terms[:, 1], out['kls']) < VGATE                         # columns 1 - 2 stay raw
    assert rel_err(terms[:, 2], out['lls']) < VGATE
    assert rel_err(terms[:, 2] - beta * terms[:, 1], terms[:, 0]) < 1e-5
    bad = []
    for n, p in m.named_parameters():
        e = rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy()))
        if not e < GATE:
            bad.append((n, e))
    assert not bad, (tag, bad)


def _run_case(arch_key, case, options):
    params, x, eps = _inputs(arch_key)
    sigma, beta, w = CASES[case]
    m = _set(make_hip_model(ARCHS[arch_key], params, options=options), sigma, beta, w)
    loss = _train_step(m, x, eps)
    out, grads = _reference(arch_key, case)
    _check_step(m, loss, out, grads, beta, f'{arch_key} {case} {options}')


# ---- 1. training step vs the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [1, 0], ids=['split_f16x3', 'exact_fp32'])
@pytest.mark.parametrize('case', list(CASES))
def test_training_step_matches_reference(case, prec):
    _run_case('tiny', case, {'conv_precision': prec})


@pytest.mark.parametrize('option', [('head_fused', 0), ('wgrad_accum', 1), ('fuse_l0', 0)], ids=lambda o: f'{o[0]}={o[1]}')
@pytest.mark.parametrize('case', ZERO_CASES)
def test_training_step_on_the_other_launch_paths(case, option):
    _run_case('tiny', case, {option[0]: option[1]})


@pytest.mark.parametrize('arch_key', ['generic', 'padded'])
def test_training_step_on_generic_and_padded_handles(arch_key):
    _run_case(arch_key, 'all', {})


@pytest.mark.parametrize('case', ['last', 'w_1_0_.5', 'w_1_.5_0'])
def test_zero_weights_on_the_generic_path(case):
    _run_case('generic', case, {})


def test_many_weightings_on_one_handle():
    """more distinct weight tables than the handle keeps (64): the unreferenced ones are freed, a forward that is still pending keeps
    its table, and an early weighting that comes back computes what it computed"""
    params, x, eps = _inputs('tiny')
    m = _set(make_hip_model(BASE, params), *CASES['w_1_0_.5'])
    loss = _train_step(m, x, eps)
    out, grads = _reference('tiny', 'w_1_0_.5')
    _check_step(m, loss, out, grads, 1.0, 'first weighting')
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    pending = m(x.to(DEV), eps.to(DEV))                                      # its table must survive what follows
    L, h = _lib.lib(), m._handle
    for j in range(70):
        wl = (_lib.C.c_double * 3)(1.0 + j, 2.0, 3.0)
        _lib.check(L.iodine_set_objective(h, 0.1, 1.0, wl, 3), h, 'iodine_set_objective')
    m._objective = None
    pending.backward()
    torch.cuda.synchronize()
    differ = [n for n, p in m.named_parameters() if not torch.equal(p.grad, want[n])]
    assert not differ, differ
    loss = _train_step(m, x, eps)                                            # the first weighting again: its table is found by content
    assert all(torch.equal(p.grad, want[n]) for n, p in m.named_parameters())


# ---- 2. inference vs the reference --------------------------------------------------------------------------------------------------
def _check_recon(m, outs, ref, tag):
    pred, mask, mean = outs
    errs = dict(elbo=rel_err(m.elbo_terms.cpu()[:, 0], ref['elbos']), kl=rel_err(m.elbo_terms.cpu()[:, 1], ref['kls']),
                ll=rel_err(m.elbo_terms.cpu()[:, 2], ref['lls']), post_mean=rel_err(m.posterior.mean.cpu(), ref['post_mean']),
                post_logvar=rel_err(m.posterior.logvar.cpu(), ref['post_logvar']), pred=rel_err(pred.cpu(), ref['pred']),
                mask=rel_err(mask.cpu(), ref['mask']), mean=rel_err(mean.cpu(), ref['mean']))
    print(f'[{tag}] ' + ' '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    # test_gpu_reconstruct: ELBO terms and the posterior 1e-4, images and masks 2e-4 (oracle on fresh inputs)
    for k in ('elbo', 'kl', 'll', 'post_mean', 'post_logvar'):
        assert errs[k] < 1e-4, (k, errs[k])
    for k in ('pred', 'mask', 'mean'):
        assert errs[k] < 2e-4, (k, errs[k])


def test_reconstruct_matches_reference():
    params, x, eps = _inputs('tiny')
    ref = R.reconstruct(x.double(), eps.double(), {k: v.double() for k, v in params.items()}, BASE, R.SIGMA, R.BETA)
    m = _set(make_hip_model(BASE, params), R.SIGMA, R.BETA, None)
    outs = m.reconstruct(x.to(DEV), eps.to(DEV))
    _check_recon(m, outs, ref, 'reconstruct')
    z = m.encode(x.to(DEV), eps.to(DEV))
    assert rel_err(z.cpu(), ref['z']) < 1e-4


def test_reconstruct_of_a_clip_continued_from_a_state_matches_reference():
    params, x, eps = _inputs('tiny')
    T = BASE.iters
    clip = moving_clip(x, 2 * T)
    eps2 = R.inputs(BASE, B, seed=R.SEED + 10)[2]
    p64 = {k: v.double() for k, v in params.items()}
    r1 = R.reconstruct(clip[:, :T].double(), eps.double(), p64, BASE, R.SIGMA, R.BETA)
    r2 = R.reconstruct(clip[:, T:].double(), eps2.double(), p64, BASE, R.SIGMA, R.BETA, init=r1['state'])
    m = _set(make_hip_model(BASE, params), R.SIGMA, R.BETA, None)
    m.reconstruct(clip[:, :T].to(DEV), eps.to(DEV))
    outs = m.reconstruct(clip[:, T:].contiguous().to(DEV), eps2.to(DEV), state=m.refinement_state())
    _check_recon(m, outs, r2, 'clip + state')


# ---- 3. elbo(x), plain and differentiable ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('given', [False, True], ids=['initial_posterior', 'given_posterior'])
def test_elbo_value_and_gradients_match_reference(given):
    params, x, eps = _inputs('tiny')
    p64 = {k: v.double() for k, v in params.items()}
    pm = plv = None
    if given:
        rec = R.reconstruct(x.double(), eps.double(), p64, BASE, R.SIGMA, R.BETA)
        pm, plv = rec['post_mean'], rec['post_logvar']
    terms, gpm, gplv, gd = R.elbo_grads(x.double(), eps[0].double(), p64, BASE, R.SIGMA, R.BETA, pm, plv)
    m = _set(make_hip_model(BASE, params), R.SIGMA, R.BETA, None)
    if given:
        m.posterior.mean = pm.float().to(DEV).requires_grad_(True)
        m.posterior.logvar = plv.float().to(DEV).requires_grad_(True)
    with torch.no_grad():
        plain = m.elbo(x.to(DEV), eps[0].to(DEV))
    t = m.elbo_terms.cpu()[0]
    print(f'[elbo given={given}] {plain.item():.6f} vs {terms["elbo"].item():.6f}')
    assert abs(plain.item() - terms['elbo'].item()) <= VGATE * abs(terms['elbo'].item())
    assert abs(t[1].item() - terms['kl'].item()) <= VGATE * abs(terms['kl'].item())
    assert abs(t[2].item() - terms['ll'].item()) <= VGATE * abs(terms['ll'].item())
    m.zero_grad(set_to_none=True)
    e = m.elbo(x.to(DEV), eps[0].to(DEV), differentiable=True)
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


# ---- 4. read per call ---------------------------------------------------------------------------------------------------------------
def _snapshot(m, x, eps):
    loss = _train_step(m, x, eps)
    out = dict(loss=loss.detach().clone(), terms=m.elbo_terms.clone())
    out.update({'g.' + n: p.grad.clone() for n, p in m.named_parameters()})
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    out.update(pred=pred, mask=mask, mean=mean, pm=m.posterior.mean.clone(), plv=m.posterior.logvar.clone(), rterms=m.elbo_terms.clone())
    return out


def test_sigma_is_read_per_call():
    """a module built with SIGMA 0.1 whose sigma is then set to 0.3 IS a module built with SIGMA 0.3, bit for bit"""
    params, x, eps = _inputs('tiny')
    assert BASE.sigma == 0.1
    late = make_hip_model(BASE, params)
    late.sigma = 0.3
    a = _snapshot(late, x, eps)
    b = _snapshot(make_hip_model(dataclasses.replace(BASE, sigma=0.3), params), x, eps)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, differ
    c = _snapshot(make_hip_model(BASE, params), x, eps)                      # ... and not the module it was built as
    assert not torch.equal(a['loss'], c['loss']) and not torch.equal(a['pm'], c['pm'])


# ---- 5. the defaults change no bit ---------------------------------------------------------------------------------------------------
def test_explicit_defaults_change_no_bit():
    params, x, eps = _inputs('tiny')
    a = _snapshot(make_hip_model(BASE, params), x, eps)
    m = _set(make_hip_model(BASE, params), BASE.sigma, 1.0, 'linspace')
    b = _snapshot(m, x, eps)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, differ
    # the default weighting as an explicit table: the same numbers through the table path, within rounding
    m.iter_weights = R.weights('linspace', BASE.iters)
    c = _snapshot(m, x, eps)
    assert abs(c['loss'].item() - a['loss'].item()) <= 1e-6 * abs(a['loss'].item())
    assert all(rel_l2(c[k].cpu().numpy(), a[k].cpu().numpy()) < 1e-5 for k in a if k.startswith('g.'))


# ---- 6. snapshot at the forward ------------------------------------------------------------------------------------------------------
def test_backward_differentiates_the_forward_as_it_ran():
    params, x, eps = _inputs('tiny')
    sigma, beta, w = CASES['all']
    m = _set(make_hip_model(BASE, params), sigma, beta, w)
    _train_step(m, x, eps)
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV))
    m.beta, m.iter_weights, m.sigma = 0.5, 'last', 0.7                       # the attributes ...
    wl = (_lib.C.c_double * 3)(0.0, 0.0, 1.0)                                # ... and the handle itself, behind the module's back
    _lib.check(_lib.lib().iodine_set_objective(m._handle, 0.7, 0.5, wl, 3), m._handle, 'iodine_set_objective')
    m._objective = None
    loss.backward()
    torch.cuda.synchronize()
    differ = [n for n, p in m.named_parameters() if not torch.equal(p.grad, want[n])]
    assert not differ, differ
    # the next forward runs the new objective
    _set(m, *CASES['last'])
    l2 = _train_step(m, x, eps)
    out, grads = _reference('tiny', 'last')
    _check_step(m, l2, out, grads, 1.0, 'after the snapshot')


# ---- 7. attach_state with a non-default objective ---------------------------------------------------------------------------------
def test_loss_plus_aux_under_an_objective_matches_reference():
    params, x, eps = _inputs('tiny')
    sigma, beta, w = CASES['all']
    W = A.aux_weights(BASE, B, seed=60)
    p64 = {k: v.double() for k, v in params.items()}
    _, ref = R.train_step_grads(x.double(), eps.double(), p64, BASE, sigma, beta, w, aux=W)
    m = _set(make_hip_model(BASE, params), sigma, beta, w)
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV), attach_state=True)
    (loss + A.hip_aux(m, W)).backward()
    torch.cuda.synchronize()
    errs = {n: rel_l2(p.grad.cpu().numpy(), ref[n].numpy()) for n, p in m.named_parameters()}      # (mask_logits has a cotangent: all of conv.bias)
    print(f'[loss + aux] worst {max(errs.values()):.2e}')
    assert all(e < GATE for e in errs.values()), errs


# ---- 8. chunked paths ---------------------------------------------------------------------------------------------------------------
def test_chunked_calls_equal_the_unchunked_ones():
    params, x, eps = _inputs('tiny')
    sigma, beta, w = CASES['all']
    whole = _set(make_hip_model(BASE, params), sigma, beta, w)
    parts = _set(make_hip_model(BASE, params, options={'batch_cap': 1}), sigma, beta, w)
    assert parts.max_batch() == 1 and parts.max_batch(training=True) == 1
    a, b = _snapshot(whole, x, eps), _snapshot(parts, x, eps)
    errs = {k: rel_l2(b[k].cpu().numpy(), a[k].cpu().numpy()) for k in a}
    print('[chunked] worst', max(errs.items(), key=lambda kv: kv[1]))
    assert all(e < 1e-5 for e in errs.values()), errs
    with torch.no_grad():
        for m in (whole, parts):
            m.posterior.mean = m.posterior.logvar = None
        ea, eb = whole.elbo(x.to(DEV), eps[0].to(DEV)), parts.elbo(x.to(DEV), eps[0].to(DEV))
    assert abs(ea.item() - eb.item()) <= 1e-5 * abs(ea.item())
    assert rel_err(parts.elbo_terms.cpu(), whole.elbo_terms.cpu()) < 1e-5


# ---- 9. graph mode ------------------------------------------------------------------------------------------------------------------
def test_graph_mode_keys_on_the_objective():
    params, x, eps = _inputs('tiny')
    eager, graphed = make_hip_model(BASE, params), make_hip_model(BASE, params, options={'graph': 1})
    for step, beta in enumerate((1.0, 2.0, 2.0, 2.0)):                       # beta 2: eager, captured, replayed
        outs = []
        for m in (eager, graphed):
            m.beta = beta
            loss = _train_step(m, x, eps)
            outs.append((loss.detach().clone(), m.elbo_terms.clone(), [p.grad.clone() for p in m.parameters()]))
        (l0, t0, g0), (l1, t1, g1) = outs
        assert torch.equal(l0, l1) and torch.equal(t0, t1), step
        assert all(torch.equal(u, v) for u, v in zip(g0, g1)), step
    assert graphed.profile_read('graph_replays')[1] > 0


# ---- 10. shape change ---------------------------------------------------------------------------------------------------------------
def test_explicit_weights_do_not_follow_n_iters_but_names_do(monkeypatch):
    params, x, _ = _inputs('tiny')
    m = make_hip_model(BASE, params)
    m.iter_weights = [1.0, 1.0, 1.0]
    eps = R.inputs(BASE, B)[2]
    _train_step(m, x, eps)
    m.n_iters = 3
    eps3 = R.inputs(dataclasses.replace(BASE, iters=3), B)[2]
    with pytest.raises(ValueError, match=r'3 entries.*n_iters = 3.*4 weights'):
        m(x.to(DEV), eps3.to(DEV))
    # the library refuses the same on its own: IODINE_ERR_INVALID at iodine_train_forward, naming both numbers
    wl = (_lib.C.c_double * 3)(1.0, 1.0, 1.0)
    _lib.check(_lib.lib().iodine_set_objective(m._handle, 0.1, 1.0, wl, 3), m._handle)
    m._objective, m.iter_weights = None, 'uniform'
    monkeypatch.setattr(_args, 'read_objective', lambda *a, _f=_args.read_objective: (*_f(*a)[:2], (1.0, 1.0, 1.0)))
    with pytest.raises(RuntimeError, match=r'3 iteration weights.*4 ELBO'):
        m(x.to(DEV), eps3.to(DEV))
    monkeypatch.undo()
    m._objective = None
    p64 = {k: v.double() for k, v in params.items()}
    a3 = dataclasses.replace(BASE, iters=3)
    out, grads = R.train_step_grads(x.double(), eps3.double(), p64, a3, BASE.sigma, 1.0, 'uniform')
    loss = _train_step(m, x, eps3)
    _check_step(m, loss, out, grads, 1.0, 'uniform at T = 3')
