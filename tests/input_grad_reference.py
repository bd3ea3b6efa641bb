"""Reference for the gradient into the image and the pixel weights and for the per-pixel likelihood maps, composed from sigma_reference
(the oracle's loop with every knob of a call: sigma, beta, iteration weights, pixel weights, a clip, a carried state).

The image and the weights are leaves that autograd sees.  ``O.input_encoding`` detaches the refinement input (iodine.py:343) and the inner
``torch.autograd.grad`` has no ``create_graph``, so both reach the loss only through the likelihood of each ELBO evaluation.  ``closed_form``
is the identity the library implements (kernels_pixmap.hip), per evaluation e with LL_e = (1 / B) sum_b sum_p w_p sum_c ll_c(p):

    d LL_e / d x[b,c,p] = -(1 / B) sum_k g1_kc,     g1_kc = w_p r_kc (x_c - mu_kc) / sigma^2      (r: responsibilities)
    d LL_e / d w[b,p]   =  (1 / B) sum_c ll_c(p)                                                  (raw: not multiplied by w)

and d loss / d (x, w) = -sum_e a_e d LL_e / d (x, w) with the iteration weights a_e; frame e of a clip (a per-frame weight image alike)
meets evaluation e alone, a 4-D weight used for every frame gets the sum.  The maps are the oracle's own ``k_ll`` / ``ll_px``."""
import torch

import sigma_reference as R
from sigma_reference import inputs                                       # noqa: F401  (re-exported: one set of inputs)


def _frame(x, i):
    return x if x is None or x.dim() == 4 else x[:, i]


def closed_form(x, w, t, sigma):
    """(d LL / d x (B, 3, S, S), d LL / d w (B, 1, S, S)) of one evaluation from its terms ``t`` (sigma_reference.s_terms)"""
    with torch.no_grad():
        B = x.shape[0]
        s = float(sigma)
        a = torch.log(t['mask'] + 1e-12) + t['k_ll']
        r = torch.exp(a - torch.logsumexp(a, dim=1, keepdim=True))
        wt = torch.ones_like(x[:, :1]) if w is None else w.expand_as(x[:, :1])
        g1 = wt[:, None] * r * (x[:, None] - t['mean']) / s ** 2
        return -g1.sum(dim=1) / B, t['ll_px'].sum(dim=1, keepdim=True) / B


def train_step_grads(x, eps, p, a, sigma, beta=1.0, iw=None, w=None, init=None, aux=None):
    """One training step with x and w as leaves -> dict(out = detached outputs, grads = {name: d / d parameter}, gx / gw = d total / d x,
    d total / d w by autograd (gw None without weights), cx / cw = d loss / d x, d loss / d w by the closed form, w-shaped: what a module
    without weights= would hand a weight of ones).  aux: a function of the attached outputs added to the loss."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xl = x.detach().clone().requires_grad_(True)
    wl = None if w is None else w.detach().clone().requires_grad_(True)
    out = R.train_forward(xl, eps, q, a, R.as_sigma(sigma, x.dtype), beta, iw, wl, False, init)
    total = out['loss'] if aux is None else out['loss'] + aux(out)
    names = list(q.keys())
    leaves = [q[n] for n in names] + [xl] + ([wl] if wl is not None else [])
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    gx = grads[len(names)].detach()
    gw = grads[len(names) + 1].detach() if wl is not None else None
    cx = torch.zeros_like(x)
    cw = torch.zeros_like(w) if w is not None else torch.zeros_like(_frame(x, 0)[:, :1])
    for e, (ae, t) in enumerate(zip(out['iw'], out['terms'])):
        dx, dw = closed_form(_frame(x, e).detach(), _frame(w, e), {k: v.detach() for k, v in t.items()}, sigma)
        if x.dim() == 5:
            cx[:, e] -= ae * dx
        else:
            cx -= ae * dx
        if w is not None and w.dim() == 5:
            cw[:, e] -= ae * dw
        else:
            cw -= ae * dw
    keep = ('loss', 'elbos', 'kls', 'lls', 'post_mean', 'post_logvar')
    det = {k: out[k].detach() for k in keep}
    det['ll_px'] = out['terms'][-1]['ll_px'].detach()
    det['k_ll'] = out['terms'][-1]['k_ll'].detach()
    return dict(out=det, grads=gd, gx=gx, gw=gw, cx=cx, cw=cw)


def elbo_grads(x, eps, p, a, sigma, beta=1.0, w=None, pm=None, plv=None):
    """One elbo(x) from (pm, plv) - None: the initial posterior - with x and w as leaves: dict(terms, grads, gx, gw, cx, cw, ll_px, k_ll)"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xl = x.detach().clone().requires_grad_(True)
    wl = None if w is None else w.detach().clone().requires_grad_(True)
    B, K = x.shape[0], a.slots
    if pm is None:
        pm = q['posterior.init_mean'][None, None].repeat(B, K, 1)
        plv = q['posterior.init_logvar'][None, None].repeat(B, K, 1)
    t = R.s_terms(xl, wl, pm, plv, eps, q, a, R.as_sigma(sigma, x.dtype), beta)
    names = list(q.keys())
    leaves = [q[n] for n in names] + [xl] + ([wl] if wl is not None else [])
    grads = torch.autograd.grad(t['elbo'], leaves, allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    cx, cw = closed_form(x.detach(), w, {k: v.detach() for k, v in t.items()}, sigma)
    return dict(terms={k: t[k].detach() for k in ('elbo', 'kl', 'll')}, grads=gd, gx=grads[len(names)].detach(),
                gw=grads[len(names) + 1].detach() if wl is not None else None, cx=cx, cw=cw, ll_px=t['ll_px'].detach(), k_ll=t['k_ll'].detach())


def kernel_reference(x, w, dec, sigma):
    """The four outputs of the per-pixel kernels on a raw decoder output, float64: x (B, 3, P), w (B, P) or None, dec (B, K, P, 4) = rgb
    logits and mask logit -> (ll (B, 3, P), kll (B, K, 3, P), vx (B, 3, P) = -sum_k g1, vw (B, P) = sum_c ll_c); a launch writes coef x vx / vw"""
    import math
    mean = torch.sigmoid(dec[..., :3]).permute(0, 1, 3, 2)               # (B, K, 3, P)
    mask = torch.softmax(dec[..., 3], dim=1)[:, :, None]                 # (B, K, 1, P)
    d = x[:, None] - mean
    kll = -d ** 2 / (2 * sigma ** 2) - math.log(sigma) - 0.5 * math.log(2 * math.pi)
    a = torch.log(mask + 1e-12) + kll
    ll = torch.logsumexp(a, dim=1)
    r = torch.exp(a - ll[:, None])
    wt = torch.ones_like(x[:, :1]) if w is None else w[:, None]
    vx = -(wt[:, None] * r * d / sigma ** 2).sum(dim=1)
    return ll, kll, vx, ll.sum(dim=1)
