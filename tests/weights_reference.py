"""Reference for per-pixel observation weights (``weights=``), composed from the oracle's public pieces.

A restatement of ``O._loop`` / ``O.train_forward`` / ``O.reconstruct`` / ``O.train_step_grads`` (oracle/iodine_oracle.py) with the weight as an
argument: ``t = O.elbo_terms(...)``, ``ll = (w * t['ll_px']).mean(0).sum()`` - iodine.py:213-220 with ``w`` in front of the pixel sum, not
normalised -, the inner ``torch.autograd.grad`` of ``B * (ll - kl)``, and ``O.input_encoding`` fed the RAW ``t`` (the likelihood-shaped
channels describe the scene, not the objective).  At ``w = 1`` it IS the oracle, op for op (test_pixel_weights_cpu pins that with
torch.equal).  ``wrong`` builds the compositions the CPU tests tell apart:

    'a'  weight in the reported LL (and the loss), not in the inner gradient
    'b'  weight in the inner gradient, not in the reported LL / loss
    'c'  weight also applied to k_ll / ll_px going into the encoding
    'd'  LL divided by mean(w)

``x`` may be a clip (B, E, 3, S, S), frame i in evaluation i - ``w`` is then (B, 1, S, S) for every frame or (B, E, 1, S, S) - and ``init`` an
initial (post_mean, post_logvar, h, c), as in clip_reference.  Parameters, images and noise come from objective_reference.inputs (seed 211)."""
import torch
import torch.nn.functional as F

from oracle import iodine_oracle as O

from objective_reference import SEED, inputs, weights as iter_weights           # noqa: F401  (re-exported: one set of inputs)

WSEED = 5
WRONG = ('a', 'b', 'c', 'd')


def pattern(B, S, dtype=torch.float64):
    """w = 0.25 + 1.25 rand(B, 1, S, S) (float64 draws, generator seed 5), then a zero rectangle of 6 x 5 pixels per image"""
    g = torch.Generator().manual_seed(WSEED)
    w = 0.25 + 1.25 * torch.rand(B, 1, S, S, generator=g, dtype=torch.float64)
    for i, (y0, x0) in enumerate(rectangles(B, S)):
        w[i, :, y0:y0 + 6, x0:x0 + 5] = 0.0
    return w.to(dtype)


def rectangles(B, S):
    """(y0, x0) of image i's zero rectangle w[i, :, y0:y0+6, x0:x0+5]"""
    return [((3 + 5 * i) % (S - 6), (2 + 7 * i) % (S - 5)) for i in range(B)]


def clip_pattern(B, E, S, dtype=torch.float64):
    """one weight image per frame, (B, E, 1, S, S): the pattern of B * E images"""
    return pattern(B * E, S, dtype).view(B, E, 1, S, S)


def _frame(x, i):
    return x if x.dim() == 4 else x[:, i]


def w_terms(x, w, pm, plv, eps, p, a, wrong=None):
    """O.elbo_terms plus the weighted terms: 'll' / 'elbo' = what the call reports, 'inner' = the ELBO the inner gradient differentiates,
    'll_img' = the per-image log-likelihood behind 'll'.  The oracle's own entries (k_ll, ll_px, ...) stay raw."""
    t = O.elbo_terms(x, pm, plv, eps, p, a)
    raw = t['ll']
    wl = w * t['ll_px']
    ll = wl.mean(0).sum()
    ll_img = wl.sum(dim=(1, 2, 3))
    if wrong == 'd':
        ll, ll_img = ll / w.mean(), ll_img / w.mean()
    t['inner'] = (raw if wrong == 'a' else ll) - t['kl']
    t['ll'] = raw if wrong == 'b' else ll
    t['ll_img'] = t['ll_px'].sum(dim=(1, 2, 3)) if wrong == 'b' else ll_img
    t['elbo'] = t['ll'] - t['kl']
    return t


def w_loop(x, w, eps, p, a, training, init=None, wrong=None):
    """O._loop under the weights.  Returns (pm, plv, hidden, elbos, kls, lls, lls_img)."""
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
    elbos, kls, lls, imgs = [], [], [], []
    for i in range(T):
        xi, wi = _frame(x, i), _frame(w, i)
        t = w_terms(xi, wi, pm, plv, eps[i], p, a, wrong)
        g_mean, g_mask, g_pm, g_plv = torch.autograd.grad(B * t['inner'], [t['mean'], t['mask'], pm, plv], retain_graph=training)
        elbos.append(t['elbo']); kls.append(t['kl']); lls.append(t['ll']); imgs.append(t['ll_img'])
        if wrong == 'c':
            t = dict(t, k_ll=wi[:, None] * t['k_ll'], ll_px=wi * t['ll_px'])
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
    return pm, plv, hidden, elbos, kls, lls, imgs


def train_forward(x, w, eps, p, a, init=None, wrong=None, iw=None):
    """O.train_forward under the weights: loss = -sum_i iw_i ELBO_i (iw: objective_reference.weights spec, default (i+1)/(T+1)); adds the
    state after T updates (attached to the graph)"""
    T = a.iters
    pm, plv, hidden, elbos, kls, lls, _ = w_loop(x, w, eps, p, a, True, init, wrong)
    t = w_terms(_frame(x, T), _frame(w, T), pm, plv, eps[T], p, a, wrong)
    elbos.append(t['elbo']); kls.append(t['kl']); lls.append(t['ll'])
    total = 0
    for wi, e in zip(iter_weights(iw, T), elbos):
        total = total + wi * e
    return dict(loss=-total, elbos=torch.stack(elbos), kls=torch.stack(kls), lls=torch.stack(lls), post_mean=pm, post_logvar=plv,
                final_mask=t['mask'], final_mean=t['mean'], hidden=hidden)


def train_step_grads(x, w, eps, p, a, init=None, wrong=None, iw=None):
    """O.train_step_grads under the weights: (detached outputs, {name: d loss / d parameter})"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    out = train_forward(x, w, eps, q, a, init, wrong, iw)
    names = list(q.keys())
    grads = torch.autograd.grad(out['loss'], [q[n] for n in names], allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    det = lambda v: tuple(u.detach() for u in v) if isinstance(v, tuple) else v.detach()
    return {k: det(v) for k, v in out.items()}, gd


def reconstruct(x, w, eps, p, a, init=None, wrong=None):
    """O.reconstruct under the weights; adds the state after T updates and the per-image log-likelihoods (T, B) of a trajectory"""
    q = {k: v.detach() for k, v in p.items()}
    pm, plv, hidden, elbos, kls, lls, imgs = w_loop(x, w, eps, q, a, False, init, wrong)
    with torch.no_grad():
        z = O.sample(pm, plv, eps[a.iters])
        mean, logits = O.decoder(z, q, a)
        mask = F.softmax(logits, dim=1)
        pred = torch.sum(mask * mean, dim=1)
    B, K = x.shape[0], a.slots
    return dict(pred=pred, mask=mask, mean=mean, z=z, post_mean=pm.detach(), post_logvar=plv.detach(),
                elbos=torch.stack([e.detach() for e in elbos]), kls=torch.stack([k.detach() for k in kls]),
                lls=torch.stack([l.detach() for l in lls]), lls_img=torch.stack([l.detach() for l in imgs]),
                state=(pm.detach(), plv.detach(), hidden[0].reshape(B, K, -1), hidden[1].reshape(B, K, -1)))


def elbo_grads(x, w, eps, p, a, pm=None, plv=None):
    """One elbo(x, weights=w) from the posterior (pm, plv) - None: the initial one - with autograd:
    (terms, d / d pm, d / d plv (None from the initial posterior), {name: d / d param})"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    B, K = x.shape[0], a.slots
    given = pm is not None
    if given:
        pm, plv = pm.detach().clone().requires_grad_(True), plv.detach().clone().requires_grad_(True)
    else:
        pm = q['posterior.init_mean'][None, None].repeat(B, K, 1)
        plv = q['posterior.init_logvar'][None, None].repeat(B, K, 1)
    t = w_terms(x, w, pm, plv, eps, q, a)
    names = list(q.keys())
    leaves = [q[n] for n in names] + ([pm, plv] if given else [])
    grads = torch.autograd.grad(t['elbo'], leaves, allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    return ({k: t[k].detach() for k in ('elbo', 'kl', 'll')}, grads[-2] if given else None, grads[-1] if given else None, gd)
