"""Reference for video input and resumable refinement, composed from the oracle's public pieces.

A restatement of ``O._loop`` (oracle/iodine_oracle.py) in which iteration i reads frame i: ``O.elbo_terms(frames[:, i], ...)``,
``torch.autograd.grad``, ``O.input_encoding(frames[:, i], ...)``, ``O.refine(..., hidden, ...)`` - with an optional initial
(post_mean, post_logvar, hidden) and a record of every iteration's decode.  With identical frames it IS the oracle's loop, op for op
(test_clip_frames_cpu pins that with torch.equal).  ``score`` / ``encode`` map the iteration to the frame that the ELBO resp. the
refinement input reads: the identity for the model; other maps build the wrong compositions the CPU tests tell apart."""
import torch
import torch.nn.functional as F

from iodine_amd import synth
from oracle import iodine_oracle as O

SEED = 131          # parameters; the scene is SEED + 1, the noise SEED + 2.  test_clip_frames_cpu shows that with these seeds the
                    # moving clip tells the correct composition from the wrong ones; the GPU tests use the same inputs


def moving_clip(x, E):
    """(B, 3, S, S) -> (B, E, 3, S, S): frame i = the scene rolled by (i, 2 i) pixels (rows, columns)"""
    return torch.stack([torch.roll(x, shifts=(i, 2 * i), dims=(-2, -1)) for i in range(E)], dim=1).contiguous()


def static_clip(x, E):
    return x[:, None].expand(x.shape[0], E, *x.shape[1:]).contiguous()


def scene(arch, B, seed):
    imgs, gt = synth.make_images(B, arch.img_size, seed=seed, kind='blobs')
    return torch.from_numpy(imgs), gt


def params(arch, seed):
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    return {k: torch.from_numpy(v) for k, v in pn.items()}


def noise(arch, B, seed, T=None, K=None):
    return torch.from_numpy(synth.make_eps(arch.iters if T is None else T, B, arch.slots if K is None else K, arch.dim_latent, seed=seed))


def _ident(i):
    return i


def clip_loop(frames, eps, p, a, training, init=None, score=_ident, encode=_ident, traj=None):
    """O._loop with frame ``score(i)`` in the ELBO of iteration i and frame ``encode(i)`` in its refinement input.
    init: (post_mean, post_logvar (B, K, L), h, c (B, K, H)) or None = Gaussian.init_unit + zero LSTM state.
    traj: list that receives, per iteration, the decode the ELBO made and its per-image terms.
    Returns (pm, plv, hidden, elbos, kls, lls)."""
    B = frames.shape[0]
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
    elbos, kls, lls = [], [], []
    for i in range(T):
        x = frames[:, score(i)]
        t = O.elbo_terms(x, pm, plv, eps[i], p, a)
        g_mean, g_mask, g_pm, g_plv = torch.autograd.grad(
            B * t['elbo'], [t['mean'], t['mask'], pm, plv], retain_graph=training)
        elbos.append(t['elbo']); kls.append(t['kl']); lls.append(t['ll'])
        if traj is not None:
            traj.append(dict(mean=t['mean'].detach(), mask=t['mask'].detach(), pred=(t['mask'] * t['mean']).sum(1).detach(),
                             kl=O.kl_unit_gaussian(pm, plv).sum((1, 2)).detach(), ll=t['ll_px'].sum((1, 2, 3)).detach()))
        xe = frames[:, encode(i)]
        if encode(i) != score(i):           # the likelihood channels of the encoding belong to the frame that is encoded
            with torch.no_grad():
                k_ll = O.gaussian_log_likelihood(xe[:, None], t['mean'], a.sigma)
                t = dict(t, k_ll=k_ll, ll_px=torch.logsumexp(torch.log(t['mask'] + 1e-12) + k_ll, dim=1))
        enc, latent = O.input_encoding(xe, t, pm, plv, g_mean, g_mask, g_pm, g_plv, a)
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


def clip_reconstruct(frames, eps, p, a, init=None, score=_ident, encode=_ident):
    """O.reconstruct over a clip (B, T, 3, S, S); adds the trajectory (T+1 decodes, (T, B) kl / ll) and the state after T updates."""
    q = {k: v.detach() for k, v in p.items()}
    tr = []
    pm, plv, hidden, elbos, kls, lls = clip_loop(frames, eps, q, a, False, init, score, encode, tr)
    with torch.no_grad():
        z = O.sample(pm, plv, eps[a.iters])
        mean, logits = O.decoder(z, q, a)
        mask = F.softmax(logits, dim=1)
        pred = torch.sum(mask * mean, dim=1)
    B, K = frames.shape[0], a.slots
    stack = lambda k: torch.stack([t[k] for t in tr])
    return dict(pred=pred, mask=mask, mean=mean, z=z, post_mean=pm.detach(), post_logvar=plv.detach(),
                elbos=torch.stack([e.detach() for e in elbos]), kls=torch.stack([k.detach() for k in kls]),
                lls=torch.stack([l.detach() for l in lls]),
                traj=dict(pred=torch.cat([stack('pred'), pred[None]]), mask=torch.cat([stack('mask'), mask[None]]),
                          mean=torch.cat([stack('mean'), mean[None]]), kl=stack('kl'), ll=stack('ll')),
                last_mask=tr[-1]['mask'], last_mean=tr[-1]['mean'],
                state=(pm.detach(), plv.detach(), hidden[0].reshape(B, K, -1), hidden[1].reshape(B, K, -1)))


def clip_train_forward(frames, eps, p, a):
    """O.train_forward over a clip (B, T+1, 3, S, S): ELBO_i against frame i, loss = -sum_i (i+1)/(T+1) ELBO_i."""
    pm, plv, _, elbos, kls, lls = clip_loop(frames, eps, p, a, True)
    t = O.elbo_terms(frames[:, a.iters], pm, plv, eps[a.iters], p, a)
    elbos.append(t['elbo']); kls.append(t['kl']); lls.append(t['ll'])
    n = len(elbos)
    total = 0
    for i, e in enumerate(elbos):
        total = total + (i + 1) / n * e
    return dict(loss=-total, elbos=torch.stack(elbos), kls=torch.stack(kls), lls=torch.stack(lls), post_mean=pm, post_logvar=plv,
                final_mask=t['mask'], final_mean=t['mean'])


def clip_train_step_grads(frames, eps, p, a):
    """O.train_step_grads over a clip: autograd through the composed forward."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    out = clip_train_forward(frames, eps, q, a)
    names = list(q.keys())
    grads = torch.autograd.grad(out['loss'], [q[n] for n in names], allow_unused=True)
    gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, gd
