"""Reference for multi-sample evaluation (``IODINE.predictive``), composed from the oracle's public pieces.

``predictive(x, w, pm, plv, eps, p, a)`` runs ``O.elbo_terms`` once per sample (``O.sample`` + decoder + mixture likelihood, iodine.py:161-241)
in the dtype of its inputs - float64 in the tests - and reduces the samples the textbook way: ``torch.mean`` / population ``torch.var`` of the
rendered image and of the masks, the count of arg-max wins per slot (lowest index on a tie), the per-image weighted log-likelihood
``ll[s, b] = sum_{c,p} w_p ll_px`` and the bounds built from it.

``bounds(ll, z, eps, pm, plv)`` is the host arithmetic on its own, written with the full Gaussian densities rather than the simplified sum the
module uses: log_w = ll + log N(z; 0, 1) - log N(z; mu, exp(logvar)), iwae = logsumexp_s(log_w) - log S, elbo_mc = mean_s log_w,
elbo = mean_s ll - KL(q || N(0, 1)) with ``O.kl_unit_gaussian``."""
import math

import torch

from oracle import iodine_oracle as O


def bounds(ll, z, eps, pm, plv):
    """ll (S, B), z / eps (S, B, K, L), pm / plv (B, K, L) -> dict(log_w (S, B), iwae, elbo_mc, elbo (B)), float64"""
    ll, z, eps, pm, plv = (t.double() for t in (ll, z, eps, pm, plv))
    S = ll.shape[0]
    c = 0.5 * math.log(2.0 * math.pi)
    log_p = (-0.5 * z ** 2 - c).sum((-2, -1))
    log_q = (-0.5 * eps ** 2 - 0.5 * plv[None] - c).sum((-2, -1))           # (z - mu)^2 / exp(logvar) = eps^2
    log_w = ll + log_p - log_q
    kl = O.kl_unit_gaussian(pm, plv).sum((-2, -1))
    return dict(log_w=log_w, iwae=torch.logsumexp(log_w, 0) - math.log(S), elbo_mc=log_w.mean(0), elbo=ll.mean(0) - kl)


def votes_of(masks):
    """masks (S, B, K, 1, H, W) -> (B, K, H, W) int64: samples in which slot k holds the pixel's largest mask, the lowest index on a tie"""
    S, B, K = masks.shape[:3]
    m = masks[:, :, :, 0]
    top = m.max(2, keepdim=True).values
    first = ((m == top).cumsum(2) == 1) & (m == top)
    return first.sum(0)


def predictive(x, w, pm, plv, eps, p, a):
    """x (B, 3, H, W) or None, w (B, 1, H, W) or None (= ones), pm / plv (B, K, L), eps (S, B, K, L), parameters p, arch a"""
    S, B = eps.shape[0], pm.shape[0]
    xs = x if x is not None else torch.zeros(B, 3, a.img_size, a.img_size, dtype=pm.dtype)
    zs, preds, masks, lls = [], [], [], []
    for s in range(S):
        t = O.elbo_terms(xs, pm, plv, eps[s], p, a)
        zs.append(t['z'])
        masks.append(t['mask'])
        preds.append((t['mask'] * t['mean']).sum(1))
        lp = t['ll_px'] if w is None else w * t['ll_px']
        lls.append(lp.sum((1, 2, 3)))
    z, pred, mask = torch.stack(zs), torch.stack(preds), torch.stack(masks)
    out = dict(z=z, pred=pred, mask=mask, pred_mean=pred.mean(0), pred_var=pred.var(0, unbiased=False), mask_mean=mask.mean(0),
               mask_var=mask.var(0, unbiased=False), votes=votes_of(mask))
    if x is not None:
        out['ll'] = torch.stack(lls)
        out.update(bounds(out['ll'], z, eps, pm, plv))
    return out
