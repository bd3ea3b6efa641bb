"""Ground truth for per-frame auxiliary losses (``forward(x, attach_frames=...)``), composed from the oracle's public pieces.

``forward`` is the loop of ``train_state_reference.forward`` that also returns, per ELBO evaluation, what the reference leaves on its module
after that ``elbo()`` call, still attached (iodine.py:171-187): ``z, mean, mask, mask_logits`` and the ``post_mean, post_logvar`` the
evaluation sampled from.  The detach points are the reference's: lambda_{i+1} = detach(lambda_i) + delta_i, refinement inputs detached.
The auxiliary functional is fixed: aux = sum over (evaluation i, tensor name) of <W[(i, name)], t_i[name]> with W standard normal, seeded by
(i, name) - a single-frame or single-kind case uses the same cotangents as the all-frames case.  Gradients are those of
g_loss * loss + aux via ``torch.autograd.grad(allow_unused=True)``.  Everything runs in the dtype asked for; ground truth is float64."""
import numpy as np
import torch

from oracle import iodine_oracle as O

TENSORS = ('z', 'mean', 'mask', 'mask_logits', 'post_mean', 'post_logvar')


def shapes(arch, B):
    K, L, S = arch.slots, arch.dim_latent, arch.img_size
    return dict(z=(B, K, L), mean=(B, K, 3, S, S), mask=(B, K, 1, S, S), mask_logits=(B, K, 1, S, S), post_mean=(B, K, L), post_logvar=(B, K, L))


def weights(arch, B, seed, evals, names=TENSORS):
    """{(i, name): W (float64)}; W[(i, name)] depends on (seed, i, name) only"""
    shp = shapes(arch, B)
    return {(i, n): torch.from_numpy(np.random.default_rng((seed * 64 + i) * 16 + TENSORS.index(n)).standard_normal(shp[n]))
            for i in evals for n in names}


def default_w(T):
    return tuple((i + 1) / (T + 1) for i in range(T + 1))


def forward(x, eps, p, a, w=None, init=None, pixel_w=None):
    """x: images (B, 3, S, S) or a clip (B, E, 3, S, S), evaluation i against frame i; eps (E, B, K, L); w: E loss weights (None: the
    default (i + 1) / E); init: None or (post_mean, post_logvar (B, K, L), h, c (B, K, H)) used as given; pixel_w: None or per-pixel
    observation weights (B, 1, S, S).  Returns dict(loss, elbos [E], evals [E] of {the six tensors, attached}, state)."""
    E = eps.shape[0]
    B, K = x.shape[0], a.slots
    w = default_w(E - 1) if w is None else w
    frame = (lambda i: x) if x.dim() == 4 else (lambda i: x[:, i])
    if init is None:
        pm = p['posterior.init_mean'][None, None].repeat(B, K, 1)
        plv = p['posterior.init_logvar'][None, None].repeat(B, K, 1)
        hidden = None
    else:
        pm, plv = init[0], init[1]
        hidden = (init[2].reshape(B * K, -1), init[3].reshape(B * K, -1))
    if not pm.requires_grad:
        pm = pm.detach().clone().requires_grad_(True)
        plv = plv.detach().clone().requires_grad_(True)

    def terms(i):
        t = O.elbo_terms(frame(i), pm, plv, eps[i], p, a)
        if pixel_w is not None:
            t['elbo'] = (pixel_w * t['ll_px']).mean(0).sum() - t['kl']
        return t

    elbos, evals = [], []
    for i in range(E):
        t = terms(i)
        elbos.append(t['elbo'])
        evals.append(dict(z=t['z'], mean=t['mean'], mask=t['mask'], mask_logits=t['logits'], post_mean=pm, post_logvar=plv))
        if i == E - 1:
            break
        g_mean, g_mask, g_pm, g_plv = torch.autograd.grad(B * t['elbo'], [t['mean'], t['mask'], pm, plv], retain_graph=True)
        enc, latent = O.input_encoding(frame(i), t, pm, plv, g_mean, g_mask, g_pm, g_plv, a)
        d_mean, d_logvar, hidden = O.refine(enc, latent, hidden, p, a)
        pm = pm.detach() + d_mean
        plv = plv.detach() + d_logvar
    total = 0
    for wi, e in zip(w, elbos):
        total = total + wi * e
    return dict(loss=-total, elbos=elbos, evals=evals, state=(pm, plv, hidden[0].reshape(B, K, -1), hidden[1].reshape(B, K, -1)))


def aux(evals, W):
    return sum((W[k].to(evals[k[0]][k[1]].dtype) * evals[k[0]][k[1]]).sum() for k in W)


def grads(x, eps, params, a, W, g_loss=0.0, w=None, init=None, pixel_w=None, dtype=torch.float64):
    """d (g_loss * loss + aux) / d params: ({name: tensor, or None where autograd finds no path}, the four gradients of ``init`` (None
    without one; zeros where no path), the forward's output)"""
    q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    leaves = None if init is None else tuple(t.detach().to(dtype).clone().requires_grad_(True) for t in init)
    out = forward(x.to(dtype), eps.to(dtype), q, a, w, leaves, None if pixel_w is None else pixel_w.to(dtype))
    total = g_loss * out['loss'] + aux(out['evals'], W)
    names = list(q)
    g = torch.autograd.grad(total, [q[n] for n in names] + list(leaves or ()), allow_unused=True)
    gs = None if leaves is None else tuple(torch.zeros_like(l) if t is None else t for l, t in zip(leaves, g[len(names):]))
    return dict(zip(names, g[:len(names)])), gs, out


def hip_aux(m, W):
    """the same functional on ``model.frames`` (float32 on the module's device)"""
    fr = m.frames
    return sum((W[(i, n)].to(device=fr[n].device, dtype=torch.float32) * fr[n][fr['index'].index(i)]).sum() for i, n in W)
