"""Reference for the objective controls (model.sigma / model.beta / model.iter_weights), composed from the oracle's public pieces.

A restatement of ``O._loop`` / ``O.train_forward`` / ``O.reconstruct`` / ``O.train_step_grads`` (oracle/iodine_oracle.py) that takes the three
knobs as arguments: the pieces get ``dataclasses.replace(arch, sigma=...)``, ``elbo = ll - beta * kl`` stands in front of
``torch.autograd.grad`` and the weights enter the final sum.  At (arch.sigma, 1, linspace) it IS the oracle, op for op
(test_objective_cpu pins that with torch.equal).  ``beta_inner`` / ``sigma_enc`` build the wrong compositions the CPU tests tell apart:
a KL weight that reaches the reported ELBO but not the inner gradient, and a likelihood scale that reaches the likelihood but not the
likelihood-shaped channels of the refinement input.  ``x`` may be a clip (B, E, 3, S, S), frame i in evaluation i, and ``init`` an initial
(post_mean, post_logvar, h, c), as in clip_reference."""
import dataclasses

import torch
import torch.nn.functional as F

from iodine_amd import synth
from oracle import iodine_oracle as O

SEED = 211          # parameters; the scene is SEED + 1, the noise SEED + 2.  test_objective_cpu shows that with these seeds the chosen
                    # knob values tell the correct composition from the wrong ones; the GPU tests use the same inputs
SIGMA, BETA = 0.3, 4.0


def weights(spec, T):
    """the T + 1 loss weights of ``spec``: None / 'linspace', 'uniform', 'last' or an explicit sequence"""
    n = T + 1
    if spec is None or spec == 'linspace':
        return [(i + 1) / n for i in range(n)]
    if spec == 'uniform':
        return [1.0 / n] * n
    if spec == 'last':
        return [0.0] * T + [1.0]
    assert len(spec) == n
    return [float(w) for w in spec]


def inputs(arch, B, seed=SEED, dtype=torch.float32, E=None):
    """(params, x, eps): blob scenes, the noise of T + 1 draws"""
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v).to(dtype) for k, v in pn.items()}
    x = torch.from_numpy(synth.make_images(B, arch.img_size, seed=seed + 1, kind='blobs')[0]).to(dtype)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=seed + 2)).to(dtype)
    return params, x, eps


def _frame(x, i):
    return x if x.dim() == 4 else x[:, i]


def obj_elbo_terms(x, pm, plv, eps, p, a, sigma, beta):
    """O.elbo_terms at ``sigma`` with elbo = ll - beta * kl (kl and ll stay raw)"""
    t = O.elbo_terms(x, pm, plv, eps, p, dataclasses.replace(a, sigma=sigma))
    t['elbo'] = t['ll'] - beta * t['kl']
    return t


def obj_loop(x, eps, p, a, training, sigma, beta, init=None, beta_inner=None, sigma_enc=None):
    """O._loop under (sigma, beta).  Returns (pm, plv, hidden, elbos, kls, lls).  beta_inner: the KL weight of the differentiated inner
    ELBO (default beta); sigma_enc: the scale of the likelihood channels of the encoding (default sigma)."""
    B = x.shape[0]
    K, T = a.slots, a.iters
    a = dataclasses.replace(a, sigma=sigma)
    if init is None:
        pm = p['posterior.init_mean'][None, None].repeat(B, K, 1)
        plv = p['posterior.init_logvar'][None, None].repeat(B, K, 1)
        hidden = None
    else:
        pm, plv = init[0].detach().clone(), init[1].detach().clone()
        hidden = (init[2].detach().reshape(B * K, -1).clone(), init[3].detach().reshape(B * K, -1).clone())
    if not pm.requires_grad:
        pm.requires_grad_(True)
        plv.requires_grad_(True)
    elbos, kls, lls = [], [], []
    for i in range(T):
        xi = _frame(x, i)
        t = O.elbo_terms(xi, pm, plv, eps[i], p, a)
        t['elbo'] = t['ll'] - beta * t['kl']
        inner = t['elbo'] if beta_inner is None else t['ll'] - beta_inner * t['kl']
        g_mean, g_mask, g_pm, g_plv = torch.autograd.grad(
            B * inner, [t['mean'], t['mask'], pm, plv], retain_graph=training)
        elbos.append(t['elbo']); kls.append(t['kl']); lls.append(t['ll'])
        if sigma_enc is not None:
            with torch.no_grad():
                k_ll = O.gaussian_log_likelihood(xi[:, None], t['mean'], sigma_enc)
                t = dict(t, k_ll=k_ll, ll_px=torch.logsumexp(torch.log(t['mask'] + 1e-12) + k_ll, dim=1))
        enc, latent = O.input_encoding(xi, t, pm, plv, g_mean, g_mask, g_pm, g_plv, a)
        d_mean, d_logvar, hidden = O.refine(enc, latent, hidden, p, a)
        if not training:
            d_mean, d_logvar = d_mean.detach(), d_logvar.detach()
            hidden = (hidden[0].detach(), hidden[1].detach())
        pm = pm.detach() + d_mean
        plv = plv.detach() + d_logvar
        if not pm.requires_grad:
            pm.requires_grad_(True)
            plv.requires_grad_(True)
    return pm, plv, hidden, elbos, kls, lls


def train_forward(x, eps, p, a, sigma, beta, w, beta_inner=None, sigma_enc=None):
    """O.train_forward under the objective: loss = -sum_i w_i ELBO_i; adds the final evaluation's tensors (attached to the graph)"""
    w = weights(w, a.iters)
    pm, plv, _, elbos, kls, lls = obj_loop(x, eps, p, a, True, sigma, beta, None, beta_inner, sigma_enc)
    t = obj_elbo_terms(_frame(x, a.iters), pm, plv, eps[a.iters], p, a, sigma, beta)
    elbos.append(t['elbo']); kls.append(t['kl']); lls.append(t['ll'])
    total = 0
    for wi, e in zip(w, elbos):
        total = total + wi * e
    return dict(loss=-total, elbos=torch.stack(elbos), kls=torch.stack(kls), lls=torch.stack(lls), post_mean=pm, post_logvar=plv,
                final_mask=t['mask'], final_mean=t['mean'], final_z=t['z'], final_logits=t['logits'])


def train_step_grads(x, eps, p, a, sigma, beta, w, aux=None, **wrong):
    """O.train_step_grads under the objective.  aux: {name: W} over aux_reference.TENSORS - the gradient is then that of
    loss + sum_t <W_t, t> on the final evaluation's tensors."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    out = train_forward(x, eps, q, a, sigma, beta, w, **wrong)
    total = out['loss']
    if aux:
        ts = dict(z=out['final_z'], mean=out['final_mean'], mask=out['final_mask'], mask_logits=out['final_logits'],
                  post_mean=out['post_mean'], post_logvar=out['post_logvar'])
        total = total + sum((aux[n].to(ts[n].dtype) * ts[n]).sum() for n in aux)
    names = list(q.keys())
    grads = torch.autograd.grad(total, [q[n] for n in names], allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, gd


def reconstruct(x, eps, p, a, sigma, beta, init=None, **wrong):
    """O.reconstruct under (sigma, beta); adds the state after T updates"""
    q = {k: v.detach() for k, v in p.items()}
    pm, plv, hidden, elbos, kls, lls = obj_loop(x, eps, q, a, False, sigma, beta, init, **wrong)
    with torch.no_grad():
        z = O.sample(pm, plv, eps[a.iters])
        mean, logits = O.decoder(z, q, a)
        mask = F.softmax(logits, dim=1)
        pred = torch.sum(mask * mean, dim=1)
    B, K = x.shape[0], a.slots
    return dict(pred=pred, mask=mask, mean=mean, z=z, post_mean=pm.detach(), post_logvar=plv.detach(),
                elbos=torch.stack([e.detach() for e in elbos]), kls=torch.stack([k.detach() for k in kls]),
                lls=torch.stack([l.detach() for l in lls]),
                state=(pm.detach(), plv.detach(), hidden[0].reshape(B, K, -1), hidden[1].reshape(B, K, -1)))


def elbo_grads(x, eps, p, a, sigma, beta, pm=None, plv=None):
    """One elbo(x) under (sigma, beta) from the posterior (pm, plv) - None: the initial one - with autograd:
    (terms, d / d pm, d / d plv (None from the initial posterior), {name: d / d param})"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    B, K = x.shape[0], a.slots
    given = pm is not None
    if given:
        pm, plv = pm.detach().clone().requires_grad_(True), plv.detach().clone().requires_grad_(True)
    else:
        pm = q['posterior.init_mean'][None, None].repeat(B, K, 1)
        plv = q['posterior.init_logvar'][None, None].repeat(B, K, 1)
    t = obj_elbo_terms(x, pm, plv, eps, q, a, sigma, beta)
    names = list(q.keys())
    leaves = [q[n] for n in names] + ([pm, plv] if given else [])
    grads = torch.autograd.grad(t['elbo'], leaves, allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    return ({k: t[k].detach() for k in ('elbo', 'kl', 'll')}, grads[-2] if given else None, grads[-1] if given else None, gd)
