"""Reference for ``model.likelihood = 'joint'`` (library option joint_likelihood): ONE K-component mixture per pixel over the whole RGB
vector, the IODINE paper's likelihood,

    LL_p = log sum_k (m_k + 1e-12) prod_c N(x_c; mu_kc, sigma) = logsumexp_k(log(m_k + 1e-12) + sum_c l_kc),

where the reference implementation (iodine.py:210-216) - and the library's default - has a mixture for each colour channel,
``sum_c logsumexp_k(log(m_k + 1e-12) + l_kc)``.  The reference has no joint form, so nothing here is a golden: the pinned oracle under a
three-line change of its ``elbo_terms`` IS the reference of this mode.

* ``evaluate(inp, dtype)``: pixel_reference.evaluate with the joint ``ll_px`` (B, 1, P) - the inputs, outputs, case table, error measures,
  margins and cap are pixel_reference's own, imported, not copied.  Gradients are autograd's; no closed form is used.
* ``joint_elbo_terms`` / ``joint_s_terms``: ``O.elbo_terms`` and ``sigma_reference.s_terms`` (the same evaluation with a tensor sigma,
  pixel weights and beta) with the joint ``ll_px`` (B, 1, S, S); ``patched()`` puts them in place, so that ``O._loop`` / ``train_forward`` /
  ``reconstruct`` / ``input_encoding`` and everything sigma_reference / input_grad_reference compose from them run the joint model
  unchanged (``input_encoding`` sums ``ll_px`` over dim 1, which holds for one plane; mask_posterior and the leave-one-out channel are
  built from ``k_ll`` and were joint over RGB all along).
* ``closed_form``: the identities the kernels implement (pixel_terms.h), in the kernel's order of operations, for tests/test_joint_cpu.py.

No GPU work here."""
import contextlib
import functools
import math
from unittest import mock

import torch
import torch.nn.functional as F

import pixel_reference as R
import sigma_reference
from oracle import iodine_oracle as O
from pixel_reference import CASES, GATE_CAP, MARGIN, case_inputs, errors, excluded, layernorm, make_inputs, plane_err, scalar_err   # noqa: F401

# the cases of the kernel-level GPU tests: a partial wave, one wave, K = 1 with weights, an unaligned block start, K = 16, a nine-block
# finalize, one pixel, saturated masks, far with weights and beta
GPU_CASES = ('near_k2_s5', 'near_k7_s8_kl448', 'near_k1_s9_w_kl3', 'near_k3_s23_w_beta', 'near_k16_s23_w_kl1024', 'near_k11_s65', 'raw_k3_s1',
             'far_k3_s23_sat_s03', 'far_k7_s33_w_s03_beta')


def joint_ll_px(mask, k_ll):
    """mask (B, K, 1, ...), k_ll (B, K, 3, ...) -> (B, 1, ...)"""
    return torch.logsumexp(torch.log(mask + 1e-12) + k_ll.sum(dim=2, keepdim=True), dim=1)


def evaluate(inp, dtype=torch.float64):
    """pixel_reference.evaluate for the joint form: the same inputs and outputs, ``ll_px`` (B, 1, P)"""
    c = lambda t: None if t is None else t.detach().to(dtype)
    x, w, pm, plv, lin = c(inp['x']), c(inp['w']), c(inp['pm']), c(inp['plv']), c(inp['lin'])
    B, K, P = inp['dec'].shape[:3]
    S = lin.numel()
    assert S * S == P
    sigma = torch.tensor(inp['sigma'], dtype=dtype, requires_grad=True)
    dec = c(inp['dec']).requires_grad_(True)
    mean = torch.sigmoid(dec[..., :3]).permute(0, 1, 3, 2)                # (B, K, 3, P)
    logits = dec[..., 3][:, :, None]                                      # (B, K, 1, P)
    mask = torch.softmax(logits, dim=1)
    k_ll = -(x[:, None] - mean) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - 0.5 * math.log(2 * math.pi)
    ll_px = joint_ll_px(mask, k_ll)                                       # (B, 1, P)
    ll_img = (ll_px if w is None else w[:, None] * ll_px).sum(dim=(1, 2))
    kl_img = (0.5 * (torch.exp(plv) + pm ** 2 - 1 - plv)).sum(dim=(1, 2))
    ll, kl = ll_img.mean(0), kl_img.mean(0)
    elbo = ll - inp['beta'] * kl
    g, g_mean, g_mask = torch.autograd.grad(B * elbo, [dec, mean, mask], retain_graph=True)
    sgrad, = torch.autograd.grad(ll, sigma)
    with torch.no_grad():
        use_ln = bool(inp['use_ln'])
        ls = k_ll.sum(dim=2, keepdim=True)                                # (B, K, 1, P)
        k_like = torch.exp(ls)
        mask_post = k_like / k_like.sum(dim=1, keepdim=True)
        like = torch.exp(ll_px.sum(dim=1, keepdim=True))[:, None].expand(B, K, 1, P).contiguous()
        mixture = (mask * k_like).sum(dim=1, keepdim=True)
        loo = (mixture - mask * k_like) / (1 - mask + 1e-5)
        n_gmean, *st_gmean = layernorm(g_mean, use_ln)
        n_gmask, *st_gmask = layernorm(g_mask, use_ln)
        n_like, *st_like = layernorm(like, use_ln)
        n_loo, *st_loo = layernorm(loo, use_ln)
        if K == 1:
            # the planes pixel_reference.evaluate states as constant for a single slot (mask = 1); d / d mask = 1 / (1 + 1e-12) here
            mask_post = torch.ones_like(mask_post)
            n_loo = torch.zeros_like(n_loo)
            if w is None and use_ln:
                n_gmask = torch.zeros_like(n_gmask)
        cx = lin.repeat(S)[None, None, None].expand(B, K, 1, P)
        cy = lin.repeat_interleave(S)[None, None, None].expand(B, K, 1, P)
        enc = torch.cat([x[:, None].expand(B, K, 3, P), mean, mask, logits, mask_post, n_gmean, n_gmask, n_like, n_loo, cx, cy], dim=2)
        lnstat = torch.stack([st_gmean[0], st_gmean[1], st_gmask[0], st_gmask[1], st_loo[0], st_loo[1], st_like[0], st_like[1]], dim=2)
        return dict(g=g.detach(), lnstat=lnstat, ll_img=ll_img.detach(), kl_img=kl_img, scal=torch.stack([elbo, kl, ll]).detach(),
                    sgrad=sgrad.reshape(1), enc=enc.permute(0, 1, 3, 2).contiguous(), mask_post_stable=torch.softmax(ls[:, :, 0], dim=1),
                    pred=(mask * mean).sum(dim=1).detach(), mask=mask[:, :, 0].detach(), mean=mean.detach(), logits=logits[:, :, 0].detach(),
                    g_mean=g_mean, g_mask=g_mask[:, :, 0], k_ll=k_ll.detach(), ll_px=ll_px.detach())


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(float64 joint reference, {stable: errors of the float32 joint evaluation on the CPU against it}): computed once, never modified"""
    inp = case_inputs(case)
    ref = evaluate(inp, torch.float64)
    lo = evaluate(inp, torch.float32)
    errs = {}
    for stable in (0, 1):
        got = dict(lo)
        if stable:
            got['enc'] = lo['enc'].clone()
            got['enc'][..., 8] = lo['mask_post_stable']
        errs[stable] = errors(got, ref, case, stable)
    return ref, errs


@functools.lru_cache(maxsize=None)
def cpu_floor():
    """{tensor: worst error of the float32 CPU evaluation of the JOINT reference over GPU_CASES (both forms of channel 8)}"""
    worst = {}
    for case in GPU_CASES:
        for e in case_reference(case)[1].values():
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


def gates(strict):
    """the project's margins over the floor of the joint reference, capped like pixel_reference.gates"""
    return {k: min(MARGIN[strict] * v, GATE_CAP) for k, v in cpu_floor().items()}


# ---- the closed forms of pixel_terms.h (JOINT), in its order of operations -----------------------------------------------------------------
def closed_form(x, w, mean, mask, sigma):
    """x (B, 3, P), w (B, P) or None, mean (B, K, 3, P), mask (B, K, 1, P), sigma a float -> dict(ll_px (B, 1, P), r (B, K, 1, P),
    g1 (B, K, 3, P) = d (sum_p w ll_px) / d mean, g2 (B, K, 1, P) = d / d mask, gx (B, 3, P) = d / d x, gw (B, P) = d / d w,
    sgrad_sigma (B,) = sigma x d / d sigma per image)"""
    lm = torch.log(mask + 1e-12)
    d = x[:, None] - mean
    l = -(d * d) * (1 / (2 * sigma * sigma)) + (-math.log(sigma) - 0.5 * math.log(2 * math.pi))
    s = (l[:, :, 0:1] + l[:, :, 1:2]) + l[:, :, 2:3]                      # lsum's order
    a = lm + s
    amax = a.amax(dim=1, keepdim=True)
    e = torch.exp(a - amax)
    den = e.sum(dim=1, keepdim=True)
    ll_px = (amax + torch.log(den))[:, 0]
    wt = torch.ones_like(x[:, :1]) if w is None else w[:, None]
    r = e * (wt[:, None] / den)                                           # w x responsibility
    g1 = r * d * (1 / (sigma * sigma))
    g2 = r / (mask + 1e-12)
    return dict(ll_px=ll_px, r=r, g1=g1, g2=g2, gx=-g1.sum(dim=1), gw=ll_px[:, 0],
                sgrad_sigma=(g1 * d).sum(dim=(1, 2, 3)) - 3 * wt.sum(dim=(1, 2)))


# ---- the oracle under the joint form ---------------------------------------------------------------------------------------------------------
def joint_elbo_terms(x, post_mean, post_logvar, eps, p, a):
    """O.elbo_terms with one mixture per pixel: ll_px (B, 1, S, S)"""
    z = O.sample(post_mean, post_logvar, eps)
    mean, logits = O.decoder(z, p, a)
    mask = F.softmax(logits, dim=1)
    kl = O.kl_unit_gaussian(post_mean, post_logvar).mean(0).sum()
    k_ll = O.gaussian_log_likelihood(x[:, None], mean, a.sigma)
    ll_px = joint_ll_px(mask, k_ll)
    ll = ll_px.mean(0).sum()
    return dict(z=z, mean=mean, logits=logits, mask=mask, k_ll=k_ll, ll_px=ll_px, kl=kl, ll=ll, elbo=ll - kl)


def joint_s_terms(x, w, pm, plv, eps, p, a, sigma, beta=1.0):
    """sigma_reference.s_terms (a tensor sigma, pixel weights, beta) with one mixture per pixel"""
    z = O.sample(pm, plv, eps)
    mean, logits = O.decoder(z, p, a)
    mask = F.softmax(logits, dim=1)
    kl = O.kl_unit_gaussian(pm, plv).mean(0).sum()
    k_ll = -(x[:, None] - mean) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - 0.5 * math.log(2 * math.pi)
    ll_px = joint_ll_px(mask, k_ll)
    ll = (ll_px if w is None else w * ll_px).mean(0).sum()
    return dict(z=z, mean=mean, logits=logits, mask=mask, k_ll=k_ll, ll_px=ll_px, kl=kl, ll=ll, elbo=ll - beta * kl)


@contextlib.contextmanager
def patched():
    """the oracle - and sigma_reference's restatement of it with the knobs of a call - as the joint model.  The closed forms that
    sigma_reference / input_grad_reference report beside autograd (``dll``, ``cx``, ``cw``) stay per-channel: under the patch use autograd's."""
    with mock.patch.object(O, 'elbo_terms', joint_elbo_terms), mock.patch.object(sigma_reference, 's_terms', joint_s_terms):
        yield
