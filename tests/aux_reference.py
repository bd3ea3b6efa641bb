"""Ground truth for auxiliary losses on the training forward's final state, composed from the oracle's public pieces in float64.

``O.train_forward`` returns the graph-attached ``post_mean`` / ``post_logvar`` / ``final_mask`` / ``final_mean`` but not ``z`` and the mask
logits of the final evaluation, so the forward is restated here from ``O._loop`` + ``O.elbo_terms`` exactly as ``O.train_forward`` composes
them (a clip: ``clip_reference.clip_loop``, frame i in evaluation i).  The auxiliary functional is fixed: aux = sum_t <W_t, t> over the chosen
tensors, W_t standard normal, so the cotangent on tensor t is W_t."""
import numpy as np
import torch

from clip_reference import clip_loop
from oracle import iodine_oracle as O

TENSORS = ('z', 'mean', 'mask', 'mask_logits', 'post_mean', 'post_logvar')


def shapes(arch, B):
    K, L, S = arch.slots, arch.dim_latent, arch.img_size
    return dict(z=(B, K, L), mean=(B, K, 3, S, S), mask=(B, K, 1, S, S), mask_logits=(B, K, 1, S, S), post_mean=(B, K, L), post_logvar=(B, K, L))


def aux_weights(arch, B, seed, names=TENSORS):
    """{name: W (float64)} for the tensors in ``names``; every tensor's W depends on (seed, its position in TENSORS) only, so a single-tensor
    case uses the same cotangent as the all-six case."""
    shp = shapes(arch, B)
    return {n: torch.from_numpy(np.random.default_rng(seed * 16 + TENSORS.index(n)).standard_normal(shp[n])) for n in names}


def oracle_forward(x, eps, params, arch):
    """float64 forward: (leaf parameters, loss, {the six tensors of the final evaluation, attached to the graph})"""
    q = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    x, eps = x.double(), eps.double()
    T = arch.iters
    if x.dim() == 5:
        pm, plv, _, elbos, _, _ = clip_loop(x, eps, q, arch, True)
        t = O.elbo_terms(x[:, T], pm, plv, eps[T], q, arch)
    else:
        pm, plv, elbos, _, _ = O._loop(x, eps, q, arch, True)
        t = O.elbo_terms(x, pm, plv, eps[T], q, arch)
    elbos = elbos + [t['elbo']]
    loss = -sum((i + 1) / (T + 1) * e for i, e in enumerate(elbos))
    return q, loss, dict(z=t['z'], mean=t['mean'], mask=t['mask'], mask_logits=t['logits'], post_mean=pm, post_logvar=plv)


def oracle_grads(x, eps, params, arch, W, g_loss=0.0):
    """d (g_loss * loss + sum_t <W_t, t>) / d params in float64: {name: tensor, or None where autograd finds no path}"""
    q, loss, ts = oracle_forward(x, eps, params, arch)
    total = g_loss * loss + sum((W[n] * ts[n]).sum() for n in W)
    names = list(q.keys())
    grads = torch.autograd.grad(total, [q[n] for n in names], allow_unused=True)
    return dict(zip(names, grads))


def hip_tensors(m):
    return dict(z=m.z, mean=m.mean, mask=m.mask, mask_logits=m.mask_logits, post_mean=m.posterior.mean, post_logvar=m.posterior.logvar)


def hip_aux(m, W):
    """the same functional on the module's attached tensors (float32 on the module's device)"""
    ts = hip_tensors(m)
    return sum((W[n].to(device=ts[n].device, dtype=torch.float32) * ts[n]).sum() for n in W)
