"""The four ``torch.autograd.Function`` nodes behind ``IODINE.forward`` / ``decode`` / ``elbo`` and their helpers.  The nodes hold no
arithmetic: ``forward`` and ``backward`` are library calls made through the module's ``_train_*`` / ``_decode_*`` / ``_elbo_*`` methods."""
import torch

from . import _args
from ._chunked import CAT0, cut, merge, split


# A ``model.sigma`` that requires grad is the LAST input of the autograd nodes below, behind the module's parameters (otherwise they take the
# inputs they always took).  Sigma reaches the loss only through the direct likelihood term of each ELBO evaluation - the refinement inputs
# are detached (iodine.py:343) - so its gradient is one scalar that the forward returns next to its other outputs when asked
# (``sigma_grad=True``; iodine_last_sigma_grad): S = sum_e w_e dLL_e/dsigma of a training forward, dLL/dsigma of an elbo.  Auxiliary
# cotangents (attach_state, attach_frames, a carried state) add nothing to it.
def _split_sigma(module, params):
    """in ``forward``: (the module's parameters, the trailing sigma input or None)"""
    n = len(module._ordered_params())
    return params[:n], (params[n] if len(params) > n else None)


def _sigma_keep(ctx, sigma, s):
    """in ``forward``: keep S (None when sigma is not an input) for ``_sigma_tail``"""
    ctx.sigma_s = s if sigma is not None else None
    ctx.sigma_shape = sigma.shape if sigma is not None else None


def _sigma_tail(ctx, g, sign):
    """in ``backward``: the gradient of the trailing sigma input - sign * g * S -, or nothing when sigma was not an input"""
    if ctx.sigma_s is None:
        return ()
    if g is None:
        return (None,)
    return ((sign * g.to(torch.float32) * ctx.sigma_s).reshape(ctx.sigma_shape),)


# The image and a floating-point ``weights=`` tensor that require grad are inputs 1 and 3 of the nodes below AS THE CALLER GAVE THEM (otherwise
# the nodes take the checked, detached forms they always took).  Like sigma they reach the loss only through the direct likelihood term of each
# ELBO evaluation - the refinement inputs are detached (iodine.py:343) -: the forward runs with option input_grad, reads
# G = sum_e a_e dLL_e/d(x, w) back once (iodine_last_input_grad) and ``backward`` returns -g_loss * G (training) / +g * G (elbo), cast to
# the caller's dtype and shape.  Auxiliary cotangents (attach_state, attach_frames, a carried state) add nothing to it.
def _ig_inputs(ctx, module, x, w, what='forward'):
    """in ``forward``: (x, w) in the library's form and the bits of option input_grad this call needs (1 image, 2 weights)"""
    need = ctx.needs_input_grad
    bits = (1 if need[1] else 0) | (2 if w is not None and need[3] else 0)
    ctx.ig, ctx.ig_meta = None, None
    if bits:
        ctx.ig_meta = (x.dtype, x.shape, None if w is None else (w.dtype, w.shape, w.device))
        x = x.detach().to(torch.float32).contiguous()
        if bits & 2:
            w = _args.check_weights(w, x, module.img_size, what)
    return x, w, bits


def _ig_keep(ctx, module, bits):
    """in ``forward``, after the library call(s): keep G = (d / d x, d / d w) for ``_ig_grads``"""
    ctx.ig = module._last_ig if bits else None


def _ig_grads(ctx, g, sign):
    """in ``backward``: the gradients of inputs 1 (x) and 3 (w) - sign * g * G -, None where they were not asked for"""
    if ctx.ig is None or g is None:
        return None, None
    sc = sign * g.to(torch.float32)
    (xd, xs, wm), (Gx, Gw) = ctx.ig_meta, ctx.ig
    gx = None if Gx is None else (sc * Gx).reshape(xs).to(xd)
    gw = None if Gw is None else (sc * Gw).reshape(wm[1]).to(device=wm[2], dtype=wm[0])
    return gx, gw


_FRAME_KEYS = ('z', 'mean', 'mask', 'mask_logits', 'post_mean', 'post_logvar')     # the order of the library's six pointers
_ALL, _FROM_STATE = ('',), ('refine.', 'decoder.')    # ``live`` of _flat_views: every parameter / those of a forward from a state


class _TrainStep(torch.autograd.Function):
    """``loss = model(x)`` / ``loss.backward()`` through iodine_train_forward_frames / iodine_train_backward_frames, the node of every
    un-chunked ``forward``.  Outputs: the loss and the ELBO terms; with ``attach`` (``attach_state=True``) also what the forward's final
    ``elbo()`` leaves on the reference's module - z, mean, mask, mask_logits, posterior.mean / .logvar and the LSTM state ``lstm_hidden``,
    there still attached to the graph (iodine.py:37,137,144,171-187,642-651); with ``index`` (``attach_frames``, a tuple of evaluations)
    also what those evaluations decoded - z, mean, mask, mask_logits and the lambda they sampled from, each (F, B, K, ...).  So one
    ``backward()`` of any combination of them is ONE library call.  The four state tensors (``state=``; None: a forward from the initial
    posterior) receive the gradient the chunk hands back when they require grad."""

    @staticmethod
    def forward(ctx, module, x, eps, w, attach, index, s_pm, s_plv, s_h, s_c, *params):
        ctx.set_materialize_grads(False)                   # an output the loss does not use arrives as None -> a NULL pointer
        state = None if s_pm is None else (s_pm, s_plv, s_h, s_c)
        params, sigma = _split_sigma(module, params)
        x, w, ig = _ig_inputs(ctx, module, x, w)
        loss, elbo_iter, frames, sg = module._train_forward(x, eps, state, weights=w, frames=index, sigma_grad=sigma is not None, input_grad=ig)
        _sigma_keep(ctx, sigma, sg)
        _ig_keep(ctx, module, ig)
        ctx.module, ctx.from_state = module, state is not None
        ctx.serial = module._session.call_serial                   # identity of the saved forward (the library keeps exactly one)
        ctx.BK, ctx.attach, ctx.index = (x.shape[0], module.K), attach, index
        ctx.mark_non_differentiable(elbo_iter)
        if not attach:
            return (loss, elbo_iter, *frames)
        module._fetch_last_elbo(x, elbo_iter[-1])      # (grad mode is off in here: the logger entries stay detached)
        module._fetch_posterior(x.shape[0])
        h, c = module._fetch_pair('iodine_last_train_state', x.shape[0], module.K, int(module._cfg.ref_mlp_units))
        H = h.shape[-1]
        return (loss, elbo_iter, module.z, module.mean, module.mask, module.mask_logits, module.posterior.mean, module.posterior.logvar,
                h.view(-1, H), c.view(-1, H), *frames)

    @staticmethod
    def backward(ctx, g_loss, _g_elbo, *gs):
        n = 8 if ctx.attach else 0
        g_z, g_mean, g_mask, g_logits, g_pm, g_plv, g_h, g_c = gs[:n] or (None,) * 8
        cot, gf = (g_mean, g_mask, g_logits, g_z, g_pm, g_plv, g_h, g_c), gs[n:] or (None,) * 6
        if g_loss is None and all(g is None for g in cot + gf):
            return (None,) * len(ctx.needs_input_grad)
        want = tuple(ctx.from_state and ctx.needs_input_grad[6 + j] for j in range(4))
        flat, gstate = ctx.module._train_backward(g_loss, ctx.serial, cot, want, ctx.BK, ctx.index, gf)
        # (the initial posterior is not part of a forward from a state: unused parameters)
        grads = _flat_views(ctx.module, flat, _FROM_STATE if ctx.from_state else _ALL)
        gx, gw = _ig_grads(ctx, g_loss, -1.0)
        return (None, gx, None, gw, None, None, *gstate, *grads, *_sigma_tail(ctx, g_loss, -1.0))




class _ChunkedTrainStep(torch.autograd.Function):
    """The same for a batch larger than one device call takes (``IODINE.max_batch``): the images are independent and the loss is
    a batch mean, so the batch runs as chunks, each chunk's forward AND backward at once (the library keeps one saved forward),
    the parameter gradients accumulated with the chunk's share of the batch; ``loss.backward()`` then only scales them."""

    @staticmethod
    def forward(ctx, module, x, eps, w, state, keep_state, *params):
        params, sigma = _split_sigma(module, params)
        x, w, ig = _ig_inputs(ctx, module, x, w)
        loss, elbo_iter, flat, sg = module._train_chunked(x, eps, state, keep_state, w, sigma_grad=sigma is not None, input_grad=ig)
        _sigma_keep(ctx, sigma, sg)                         # (S: every chunk's share of the batch, added up by _train_chunked)
        _ig_keep(ctx, module, ig)                           # (G: every chunk's scaled by its share, concatenated along the batch)
        ctx.module, ctx.flat, ctx.from_state = module, flat, state is not None
        ctx.mark_non_differentiable(elbo_iter)
        return loss, elbo_iter

    @staticmethod
    def backward(ctx, grad_loss, _grad_elbo):
        # (from a detached state the initial posterior is not part of the forward: None, like unused parameters elsewhere)
        views = _flat_views(ctx.module, ctx.flat * grad_loss.to(ctx.flat.dtype), _FROM_STATE if ctx.from_state else _ALL)
        gx, gw = _ig_grads(ctx, grad_loss, -1.0)
        return (None, gx, None, gw, None, None, *views, *_sigma_tail(ctx, grad_loss, -1.0))


def _flat_views(module, flat, live):
    """Per-parameter gradients for autograd: views of the one flat buffer for the parameters named by ``live`` (name prefixes), None for
    the rest - the reference's autograd leaves .grad of a parameter the differentiated call never used at None too."""
    views, off = [], 0
    for n, p in module.named_parameters():
        views.append(flat[off:off + p.numel()].view_as(p) if flat is not None and n.startswith(live) else None)
        off += p.numel()
    return views


class _DecodeGrad(torch.autograd.Function):
    """``pred, mask, mean = model.decode(z)`` with autograd into ``z`` and the decoder weights (iodine.py:59-71) through
    iodine_decode (option save_for_backward) / iodine_decode_backward.  A batch above ``IODINE.max_batch`` is decoded in chunks and
    each chunk is decoded AGAIN in the backward, its backward right behind it (the library keeps one saved pass)."""

    @staticmethod
    def forward(ctx, module, z, *params):
        ctx.set_materialize_grads(False)                   # an output the loss does not use arrives as None -> a NULL pointer
        K = int(z.shape[1])
        T = module._session.shape[1]                       # the iteration count plays no part in a decode: the handle's
        ctx.module, ctx.K, ctx.T, ctx.z_dtype = module, K, T, z.dtype
        ctx.chunks = split(z.shape[0], module.max_batch(K=K, T=T))
        zc = z.detach().to(torch.float32).contiguous()
        if len(ctx.chunks) == 1:
            out = module._decode_call(zc, K, T, save=True)
            ctx.serial = module._session.call_serial               # identity of the saved pass
        else:
            out = merge([module._decode_call(zc[s:e], K, T, save=False) for s, e, _ in ctx.chunks], (CAT0,) * 3)
            ctx.z, ctx.versions = zc, module._session.param_versions
        return out

    @staticmethod
    def backward(ctx, g_pred, g_mask, g_mean):
        m = ctx.module
        want_z, want_p = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        if g_pred is None and g_mask is None and g_mean is None:
            return (None,) * len(ctx.needs_input_grad)
        if len(ctx.chunks) == 1:
            dz, flat = m._decode_backward(ctx.serial, ctx.K, (g_pred, g_mask, g_mean), want_z, want_p, None)
        else:
            m._bind(ctx.z.device).sync_params()
            if m._session.param_versions != ctx.versions:
                raise RuntimeError('IODINE: backward of a stale decode - the parameters changed since the chunked decode ran (its chunks '
                                   'are decoded again in the backward; call backward() before the optimizer step)')
            dzs, flat = [], None
            for s, e, _ in ctx.chunks:
                m._decode_call(ctx.z[s:e], ctx.K, ctx.T, save=True)
                gs = tuple(cut(g, s, e) for g in (g_pred, g_mask, g_mean))
                dzc, flat = m._decode_backward(m._session.call_serial, ctx.K, gs, want_z, want_p, flat)
                dzs.append(dzc)
            dz = torch.cat(dzs, 0) if want_z else None
        flat = m._session.own(flat)
        return (None, None if dz is None else dz.to(ctx.z_dtype), *_flat_views(m, flat, ('decoder.',)))


class _ElboGrad(torch.autograd.Function):
    """``elbo = model.elbo(x)`` with autograd into ``model.posterior.mean / logvar`` (or, from the initial posterior, into
    ``posterior.init_mean / init_logvar``) and the decoder weights (iodine.py:161-241) through iodine_elbo (option save_for_backward) /
    iodine_elbo_backward.  The ELBO is a batch mean of independent images: a batch above ``IODINE.max_batch`` runs as chunks, each
    chunk's forward and backward at once with its share of the batch, and ``backward`` only scales - like _ChunkedTrainStep."""

    @staticmethod
    def forward(ctx, module, x, eps, w, pm, plv, *params):
        ctx.set_materialize_grads(False)
        ctx.module, ctx.init = module, pm is None
        params, sigma = _split_sigma(module, params)
        x, w, ig = _ig_inputs(ctx, module, x, w, 'weighted_elbo')
        ctx.n = len(params)
        want_p = any(p.requires_grad for p in params)
        want_post = pm is not None and (pm.requires_grad or plv.requires_grad)
        if x.shape[0] <= module.max_batch():
            r = module._elbo_call(x, eps, pm, plv, save=True, weights=w, sigma_grad=sigma is not None, input_grad=ig)
            elbo, sg = r if sigma is not None else (r, None)
            ctx.serial, ctx.pre, ctx.BK = module._session.call_serial, None, (x.shape[0], module.K)
        else:
            elbo, ctx.pre, sg = module._elbo_chunked_grad(x, eps, pm, plv, want_post, want_p, w, sigma_grad=sigma is not None, input_grad=ig)
        _sigma_keep(ctx, sigma, sg)
        _ig_keep(ctx, module, ig)
        return elbo

    @staticmethod
    def backward(ctx, g):
        m = ctx.module
        n_in = len(ctx.needs_input_grad)
        if g is None:
            return (None,) * n_in
        live = ('decoder.', 'posterior.') if ctx.init else ('decoder.',)
        if ctx.pre is not None:                            # chunked: everything was computed with the forward
            gs = g.to(torch.float32)
            gpm, gplv, flat = (None if t is None else t * gs for t in ctx.pre)
        else:
            want_post = (not ctx.init) and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5])
            gpm, gplv, flat = m._elbo_backward(ctx.serial, ctx.BK, g, want_post, any(ctx.needs_input_grad[6:6 + ctx.n]))
            flat = m._session.own(flat)
        gx, gw = _ig_grads(ctx, g, 1.0)
        return (None, gx, None, gw, gpm if ctx.needs_input_grad[4] else None, gplv if ctx.needs_input_grad[5] else None,
                *_flat_views(m, flat, live), *_sigma_tail(ctx, g, 1.0))
