"""Reference for a differentiable ``model.sigma`` and for ``model.stable_encoding``, composed from the oracle's public pieces.

A restatement of ``O._loop`` / ``O.train_forward`` / ``O.reconstruct`` (oracle/iodine_oracle.py) in which sigma is a TENSOR that autograd
sees - ``O.gaussian_log_likelihood`` takes ``math.log`` of its scale, which would cut the graph - next to the other knobs of a call: ``beta``
(elbo = ll - beta kl), ``iw`` (the T + 1 loss weights, objective_reference.weights), ``w`` (per-pixel observation weights in front of the pixel
sum, as in weights_reference) and ``stable``: channel ``mask_posterior`` of the encoding as ``softmax_k(sum_c l_kc)`` instead of the oracle's
``exp(sum_c l_kc) / sum_k exp(sum_c l_kc)``.  The inner ``torch.autograd.grad`` has no ``create_graph`` and ``O.input_encoding`` detaches, so
sigma reaches the loss only through the likelihood of each evaluation, as in the reference (iodine.py:343).

``closed_form`` is the identity the library implements:
    d/dsigma [ w sum_c logsumexp_k(log(m_k + 1e-12) + l_kc) ] = ( sum_{k,c} g1_kc (x_c - mu_kc) - 3 w ) / sigma,   g1 = w r (x - mu) / sigma^2
``x`` may be a clip (B, E, 3, S, S), frame i in evaluation i (``w`` then (B, 1, S, S) or (B, E, 1, S, S)), ``init`` an initial
(post_mean, post_logvar, h, c).  Inputs: objective_reference.inputs."""
import math

import torch
import torch.nn.functional as F

from oracle import iodine_oracle as O

from objective_reference import inputs, weights as iter_weights           # noqa: F401  (re-exported: one set of inputs)

_BEFORE_MASK_POSTERIOR = (('image', 3), ('means', 3), ('mask', 1), ('mask_logits', 1))


def _frame(x, i):
    return x if x is None or x.dim() == 4 else x[:, i]


def as_sigma(sigma, dtype=torch.float64, requires_grad=False):
    s = sigma.detach().to(dtype).reshape(()) if torch.is_tensor(sigma) else torch.tensor(float(sigma), dtype=dtype)
    return s.clone().requires_grad_(requires_grad)


def s_terms(x, w, pm, plv, eps, p, a, sigma, beta=1.0):
    """O.elbo_terms with a tensor sigma, pixel weights w (None: 1) and elbo = ll - beta kl; k_ll / ll_px stay raw (they describe the scene)"""
    z = O.sample(pm, plv, eps)
    mean, logits = O.decoder(z, p, a)
    mask = F.softmax(logits, dim=1)
    kl = O.kl_unit_gaussian(pm, plv).mean(0).sum()
    k_ll = -(x[:, None] - mean) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - 0.5 * math.log(2 * math.pi)
    ll_px = torch.logsumexp(torch.log(mask + 1e-12) + k_ll, dim=1)
    ll = (ll_px if w is None else w * ll_px).mean(0).sum()
    return dict(z=z, mean=mean, logits=logits, mask=mask, k_ll=k_ll, ll_px=ll_px, kl=kl, ll=ll, elbo=ll - beta * kl)


def closed_form(x, w, t, sigma):
    """(d ll / d sigma by the identity, sum of g1 (x - mu) over everything, 3 x the sum of the weights): the second over the third is the
    cancellation ratio of the scalar"""
    with torch.no_grad():
        s = sigma.detach()
        a = torch.log(t['mask'] + 1e-12) + t['k_ll']
        r = torch.exp(a - torch.logsumexp(a, dim=1, keepdim=True))
        d = x[:, None] - t['mean']
        wt = torch.ones_like(x[:, :1]) if w is None else w.expand_as(x[:, :1])
        g1 = wt[:, None] * r * d / s ** 2
        pos = (g1 * d).sum(dim=(1, 2, 3, 4))                              # per image
        neg = 3.0 * wt.sum(dim=(1, 2, 3))
        return ((pos - neg) / s).mean(0), pos.sum(), neg.sum()


def stable_channel(enc, t, a):
    """``enc`` with the mask_posterior channel replaced by softmax_k(sum_c l_kc)"""
    if 'mask_posterior' not in a.encoding:
        return enc
    idx = sum(n for name, n in _BEFORE_MASK_POSTERIOR if name in a.encoding)
    enc = enc.clone()
    enc[:, :, idx] = F.softmax(t['k_ll'].detach().sum(dim=2), dim=1)
    return enc


def s_loop(x, w, eps, p, a, training, sigma, beta=1.0, stable=False, init=None, trace=None):
    """O._loop under the knobs.  Returns (pm, plv, hidden, terms of the T evaluations, their closed forms)."""
    B = x.shape[0]
    K, T = a.slots, a.iters
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
    ts, cfs = [], []
    for i in range(T):
        xi, wi = _frame(x, i), _frame(w, i)
        t = s_terms(xi, wi, pm, plv, eps[i], p, a, sigma, beta)
        g_mean, g_mask, g_pm, g_plv = torch.autograd.grad(B * t['elbo'], [t['mean'], t['mask'], pm, plv], retain_graph=training)
        ts.append(t); cfs.append(closed_form(xi, wi, t, sigma))
        enc, latent = O.input_encoding(xi, t, pm, plv, g_mean, g_mask, g_pm, g_plv, a)
        if stable:
            enc = stable_channel(enc, t, a)
        if trace is not None:
            trace.append(dict(enc=enc))
        d_mean, d_logvar, hidden = O.refine(enc, latent, hidden, p, a)
        if not training:
            d_mean, d_logvar = d_mean.detach(), d_logvar.detach()
            hidden = (hidden[0].detach(), hidden[1].detach())
        pm = pm.detach() + d_mean
        plv = plv.detach() + d_logvar
        if not pm.requires_grad:
            pm.requires_grad_(True)
            plv.requires_grad_(True)
    return pm, plv, hidden, ts, cfs


def train_forward(x, eps, p, a, sigma, beta=1.0, iw=None, w=None, stable=False, init=None):
    """loss = -sum_i iw_i ELBO_i with everything attached to the graph (sigma included); ``dll`` = the closed form per evaluation,
    ``ratio`` = the smallest cancellation ratio over the evaluations"""
    T = a.iters
    pm, plv, hidden, ts, cfs = s_loop(x, w, eps, p, a, True, sigma, beta, stable, init)
    t = s_terms(_frame(x, T), _frame(w, T), pm, plv, eps[T], p, a, sigma, beta)
    ts.append(t); cfs.append(closed_form(_frame(x, T), _frame(w, T), t, sigma))
    iws = iter_weights(iw, T)
    total = 0
    for wi, e in zip(iws, ts):
        total = total + wi * e['elbo']
    return dict(loss=-total, elbos=torch.stack([e['elbo'] for e in ts]), kls=torch.stack([e['kl'] for e in ts]),
                lls=torch.stack([e['ll'] for e in ts]), dll=torch.stack([c[0] for c in cfs]),
                ratio=min(float(c[1] / c[2]) for c in cfs if float(c[2]) > 0), iw=iws, post_mean=pm, post_logvar=plv, hidden=hidden,
                final_mask=t['mask'], final_mean=t['mean'], final_z=t['z'], final_logits=t['logits'], terms=ts)


def train_step_grads(x, eps, p, a, sigma, beta=1.0, iw=None, w=None, stable=False, init=None, aux=None):
    """-> (detached outputs, {name: d total / d parameter}, d total / d sigma by autograd, d loss / d sigma by the closed form).
    aux: a function of the attached outputs returning a scalar added to the loss (auxiliary terms on the final state / on ``terms``)."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    s = as_sigma(sigma, x.dtype, True)
    out = train_forward(x, eps, q, a, s, beta, iw, w, stable, init)
    total = out['loss'] if aux is None else out['loss'] + aux(out)
    names = list(q.keys())
    grads = torch.autograd.grad(total, [q[n] for n in names] + [s], allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    closed = -sum(wi * d for wi, d in zip(out['iw'], out['dll']))
    keep = ('loss', 'elbos', 'kls', 'lls', 'dll', 'post_mean', 'post_logvar', 'final_mask', 'final_mean', 'final_z', 'final_logits')
    det = {k: out[k].detach() for k in keep}
    det['ratio'] = out['ratio']
    return det, gd, grads[-1].detach(), closed.detach()


def reconstruct(x, eps, p, a, sigma, beta=1.0, w=None, stable=False, init=None, trace=None):
    """O.reconstruct under the knobs (detached)"""
    q = {k: v.detach() for k, v in p.items()}
    s = as_sigma(sigma, x.dtype)
    pm, plv, hidden, ts, _ = s_loop(x, w, eps, q, a, False, s, beta, stable, init, trace)
    with torch.no_grad():
        z = O.sample(pm, plv, eps[a.iters])
        mean, logits = O.decoder(z, q, a)
        mask = F.softmax(logits, dim=1)
        pred = torch.sum(mask * mean, dim=1)
    return dict(pred=pred, mask=mask, mean=mean, z=z, post_mean=pm.detach(), post_logvar=plv.detach(),
                elbos=torch.stack([t['elbo'].detach() for t in ts]), kls=torch.stack([t['kl'].detach() for t in ts]),
                lls=torch.stack([t['ll'].detach() for t in ts]))


def elbo_grads(x, eps, p, a, sigma, beta=1.0, w=None, pm=None, plv=None):
    """One elbo(x) from (pm, plv) - None: the initial posterior: (terms, {name: d / d param}, d elbo / d sigma by autograd, by the closed
    form, the cancellation ratio)"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    s = as_sigma(sigma, x.dtype, True)
    B, K = x.shape[0], a.slots
    if pm is None:
        pm = q['posterior.init_mean'][None, None].repeat(B, K, 1)
        plv = q['posterior.init_logvar'][None, None].repeat(B, K, 1)
    t = s_terms(x, w, pm, plv, eps, q, a, s, beta)
    names = list(q.keys())
    grads = torch.autograd.grad(t['elbo'], [q[n] for n in names] + [s], allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    cf = closed_form(x, w, t, s)
    return {k: t[k].detach() for k in ('elbo', 'kl', 'll')}, gd, grads[-1].detach(), cf[0], float(cf[1] / cf[2])


def pinned_scene(dtype=torch.float32):
    """The 0 / 0 scene of tests/test_gpu_boundary.py::test_mask_posterior_zero_over_zero_edge: (arch, params, x, eps)"""
    import numpy as np
    from iodine_amd import synth
    arch = O.tiny_arch(slots=3, iters=2)
    pn = synth.make_params(O.param_shapes(arch), seed=5, dec_gain=2.0, posterior_scale=0.05)
    pn['decoder.conv.bias'] = np.array([-6.0, -6.0, -6.0, 0.0], dtype=np.float32)
    params = {k: torch.from_numpy(v).to(dtype) for k, v in pn.items()}
    x = (torch.from_numpy(synth.make_images(2, arch.img_size, seed=3, kind='blobs')[0]) * 0.3).to(dtype)
    x[0] = 1.0
    eps = torch.from_numpy(synth.make_eps(arch.iters, 2, arch.slots, arch.dim_latent, seed=4)).to(dtype)
    return arch, params, x, eps
