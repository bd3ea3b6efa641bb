"""Reference for training from a carried state (truncated and exact BPTT over a clip), composed from the oracle's public pieces.

``forward`` is ``clip_reference.clip_loop`` + the final evaluation of ``O.train_forward`` with three differences: the initial state
(post_mean, post_logvar, h, c) is used AS GIVEN - leaves that require grad receive a gradient, the attached final state of an earlier
chunk keeps the graph across the boundary, detached tensors truncate it; the loss weights are explicit; and the final (lambda_T, h_T,
c_T) come back attached.  The number of iterations is the number of frames minus one, so one function serves the chunks (T = 2) and the
long forward (T = 4).  ``O.refine`` returns the LSTM state as (h1, c1), torch order, and the state tuples here use that order too.

Everything runs in the dtype of its inputs; the gradient references are taken in float64."""
import dataclasses

import torch

import clip_reference as R
from oracle import iodine_oracle as O

SEED = R.SEED       # parameters 131, scene 132, noise 133: the inputs of tests/clip_reference.py
T = 2               # iterations per chunk; the clip has 2 T + 1 = 5 frames
W_CHUNK = (0.2, 0.3, 0.5)                   # loss weights of a chunk's T + 1 evaluations (w_0 != 0: lambda_0 receives a gradient)
W_LATER = (0.0,) + W_CHUNK[1:]              # chunks after the first: the boundary evaluation was scored by the chunk before
W_LONG = W_CHUNK + W_CHUNK[1:]              # the same objective as ONE forward over the 5 frames


def arch(K=3, **kw):
    return dataclasses.replace(O.tiny_arch(slots=K, iters=T), **kw)


def inputs(a, B, dtype=torch.float32):
    """(params, clip (B, 5, 3, S, S), eps (5, B, K, L)) of the moving clip"""
    p = {k: v.to(dtype) for k, v in R.params(a, SEED).items()}
    x, _ = R.scene(a, B, SEED + 1)
    return p, R.moving_clip(x, 2 * T + 1).to(dtype), R.noise(a, B, SEED + 2, T=2 * T).to(dtype)


def weighted_loss(elbos, w):
    assert len(elbos) == len(w)
    total = 0
    for wi, e in zip(w, elbos):
        total = total + wi * e
    return -total


def forward(frames, eps, p, a, w, init=None):
    """frames (B, E, 3, S, S), eps (E, B, K, L), w: E weights; E - 1 refinement iterations and the final evaluation.
    init: None = Gaussian.init_unit + zero LSTM state, or (post_mean, post_logvar (B, K, L), h, c (B, K, H)) used as given.
    Returns dict(loss, elbos [E], state = (post_mean, post_logvar, h, c) after the last update, attached)."""
    B, E = frames.shape[0], frames.shape[1]
    K = a.slots
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
    elbos = []
    for i in range(E - 1):
        x = frames[:, i]
        t = O.elbo_terms(x, pm, plv, eps[i], p, a)
        g_mean, g_mask, g_pm, g_plv = torch.autograd.grad(B * t['elbo'], [t['mean'], t['mask'], pm, plv], retain_graph=True)
        elbos.append(t['elbo'])
        enc, latent = O.input_encoding(x, t, pm, plv, g_mean, g_mask, g_pm, g_plv, a)
        d_mean, d_logvar, hidden = O.refine(enc, latent, hidden, p, a)
        pm = pm.detach() + d_mean
        plv = plv.detach() + d_logvar
    elbos.append(O.elbo_terms(frames[:, E - 1], pm, plv, eps[E - 1], p, a)['elbo'])
    return dict(loss=weighted_loss(elbos, w), elbos=elbos,
                state=(pm, plv, hidden[0].reshape(B, K, -1), hidden[1].reshape(B, K, -1)))


def leaf_params(p, dtype=torch.float64):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}


def param_grads(total, q):
    """{name: d total / d q[name]}, zeros where autograd finds no path"""
    names = list(q)
    grads = torch.autograd.grad(total, [q[n] for n in names], allow_unused=True)
    return {n: (torch.zeros_like(q[n]) if g is None else g) for n, g in zip(names, grads)}


def long_grads(frames, eps, p, a, w=W_LONG):
    """the gradient of ONE forward over all frames: (out, {name: grad}) in float64"""
    q = leaf_params(p)
    out = forward(frames.double(), eps.double(), q, a, w)
    return out, param_grads(out['loss'], q)


def chunked_grads(frames, eps, p, a, exact, w0=W_CHUNK, w1=W_LATER):
    """two chunks of T iterations over the 2 T + 1 frames, float64: (out1, out2, {name: grad of loss1 + loss2}).  exact: chunk 2 starts
    from chunk 1's attached state (the long forward's graph); otherwise from its detached values (truncated BPTT)."""
    q = leaf_params(p)
    f, e = frames.double(), eps.double()
    o1 = forward(f[:, :T + 1], e[:T + 1], q, a, w0)
    init = o1['state'] if exact else tuple(t.detach() for t in o1['state'])
    o2 = forward(f[:, T:], e[T:], q, a, w1, init)
    return o1, o2, param_grads(o1['loss'] + o2['loss'], q)


def state_after_first_chunk(frames, eps, p, a, dtype=torch.float64):
    """detached (post_mean, post_logvar, h, c) that chunk 1 leaves - the entry state of chunk 2"""
    q = leaf_params(p, dtype)                   # (attached: the loop differentiates every evaluation with respect to its lambda)
    o1 = forward(frames[:, :T + 1].to(dtype), eps[:T + 1].to(dtype), q, a, W_CHUNK)
    return tuple(t.detach() for t in o1['state'])


def second_chunk_grads(frames, eps, p, a, state, w, g_loss=1.0, W_h=None, W_c=None):
    """float64 gradient of g_loss * loss + <W_h, h_T> + <W_c, c_T> of chunk 2 run from ``state`` as leaves:
    ({name: parameter grad}, (d / d post_mean, d / d post_logvar, d / d h, d / d c), out)"""
    q = leaf_params(p)
    leaves = tuple(t.detach().double().clone().requires_grad_(True) for t in state)
    out = forward(frames[:, T:].double(), eps[T:].double(), q, a, w, leaves)
    total = g_loss * out['loss']
    if W_h is not None:
        total = total + (W_h.double() * out['state'][2]).sum() + (W_c.double() * out['state'][3]).sum()
    names = list(q)
    grads = torch.autograd.grad(total, [q[n] for n in names] + list(leaves), allow_unused=True)
    gp = {n: (torch.zeros_like(q[n]) if g is None else g) for n, g in zip(names, grads)}
    gs = tuple(torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads[len(names):]))
    return gp, gs, out
