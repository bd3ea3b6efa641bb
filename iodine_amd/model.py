"""``IODINE(ARCH)``: the reference's module surface over libiodine_hip.so.

Mirrors ``lib/modeling/iodine.py`` of zhixuan-lin/IODINE for the callers of the hot path:
``loss = model(x)`` (lib/engine/train.py:60), ``model.reconstruct(image)``
(lib/eval/ari_eval.py:22), ``encode`` / ``decode`` (iodine.py:59-112), the
``named_parameters()`` / ``state_dict()`` names (lib/solver/build.py:10-14,
lib/utils/checkpoint.py:43,68), ``model.sigma`` (train.py:97) and the ``logger`` side
channel keys (iodine.py:156-157,226-239).  All arithmetic runs in hand-written gfx950
kernels behind the C ABI of include/iodine_hip.h; PyTorch only owns the tensors, the
stream and the autograd hook-up.  There is no CPU or eager fallback: tensors must live on
a ROCm device and the shared library must be built.

Like the reference, ``model.K`` and ``model.n_iters`` are plain attributes read when a call starts (iodine.py:81-83,123-126): set
them to run the same weights at another slot count (1..16) or iteration count - the paper's generalisation setting, e.g. CLEVR6
weights trained at K = 7, T = 5 evaluated at K = 11 - and ``decode(z)`` takes K from ``z`` (iodine.py:430).  The library handle
follows through ``iodine_set_run_shape``; ``loss.backward()`` differentiates the forward at the shape it ran with.

The objective is read the same way: ``model.sigma`` (the reference reads ``self.sigma`` on every ``elbo()`` call, iodine.py:210),
``model.beta`` - the weight of the KL term, as if iodine.py:223 read ``elbo = log_likelihood - self.beta * kl`` - and
``model.iter_weights`` - the per-iteration loss weights of iodine.py:152-153: None / 'linspace' = (i+1)/(T+1), 'uniform', 'last' or a
sequence of T + 1 numbers.  They are checked on the host when a call starts and reach the handle through ``iodine_set_objective``;
``loss.backward()`` differentiates the forward with the objective it ran with.

Video input and resumable refinement (the paper's tracking use of the T-step loop; the reference closes ``encode`` / ``forward`` over
one ``x``, iodine.py:73-105,115-158): ``x`` may be a clip ``(B, E, 3, S, S)`` with one frame per ELBO evaluation of the call (E = T for
``encode`` / ``reconstruct``, T + 1 for ``forward``); ``reconstruct(x, trajectory=True)`` leaves the decode of every iteration in
``model.trajectory``; ``reconstruct(x, objects=True)`` leaves the per-slot object table, the segmentation map and the per-slot KL in
``model.objects`` (``iodine_amd.objects``); ``model.refinement_state()`` / ``state=`` carry (lambda, h, c) from one call into the next, so a long clip runs
in chunks of ``n_iters`` frames.  Training carries the state the same way: ``forward(x, state=..., keep_state=True)`` continues a clip
from the state the last chunk left - detached tensors give truncated back-propagation through time, tensors that require grad receive the
gradient of the chunk (``iodine_train_backward_seq``), and ``attach_state=True`` leaves ``model.lstm_hidden`` attached to the graph like
the reference, so that ``iodine_amd.engine.clip_backward`` computes the exact gradient of a long clip chunk by chunk.
``forward(x, attach_frames=...)`` leaves chosen ELBO evaluations of the call attached in ``model.frames`` - a loss on every frame of a
clip in one ``(loss + aux).backward()`` (``iodine_train_forward_frames`` / ``iodine_train_backward_frames``).

Per-pixel observation weights: ``forward`` / ``encode`` / ``reconstruct`` take ``weights=`` (the single-pass ELBO: ``weighted_elbo(x, weights)``; ``elbo`` keeps
the reference's signature), a tensor ``(B, 1, S, S)`` or
``(B, S, S)`` of numbers >= 0 (bool / uint8 / any float dtype; with a clip also ``(B, E, 1, S, S)`` / ``(B, E, S, S)``, one weight image per
frame - a 4-D weight is used for every frame), for padded or invalid regions, inpainting ("explain what I observed, show ``pred``
everywhere"), region-of-interest training, down-weighting a background:

    LL = mean_b sum_p w_p sum_c logsumexp_k(log(m_k + 1e-12) + l_kc),    ELBO = LL - beta * KL     (not normalised by sum(w) or mean(w))

    weighted      the reported LL / ELBO / loss (``elbo_terms[:, 0]`` and ``[:, 2]``, the logger's ``likelihood``, ``trajectory['ll']``);
                  the closed-form inner gradients d(B ELBO)/d mean and /d mask and everything downstream of them, as autograd gives for
                  the weighted objective: ``grad_post``, the layer-normed gradient channels of the refinement input, every outer gradient
    not weighted  the refinement-input channels that describe the scene (``mask_posterior``, ``likelihood``,
                  ``leave_one_out_likelihood``), the image channels, the KL

A weight tensor that requires grad receives ``d loss / d w``; otherwise weights are data.  Their values are the caller's contract (finite, >= 0,
not checked on the device); zeros are allowed, an all-zero image included.  They hold for the one call they are passed to (``iodine_set_pixel_weights``
is one-shot); ``weights=None`` and weights of all ones compute the same bits.

Gradients into the image and the weights: an ``x`` that requires grad (grad mode on) is a differentiable input of ``forward`` / ``elbo`` /
``weighted_elbo``, like in the reference, whose refinement input is detached (iodine.py:343) - ``d loss / d x`` is the direct likelihood
term of each ELBO evaluation, ``-sum_e a_e dLL_e/dx`` with ``dLL/dx[b,c,p] = -(1/B) sum_k w_p r_kc (x_c - mu_kc) / sigma^2``; frame e of a clip
gets its own evaluation's term.  A floating-point ``weights=`` tensor that requires grad gets ``dLL/dw[b,p] = (1/B) sum_c log_likelihood[b,c,p]``
(raw, not multiplied by w), in whichever accepted shape it was passed; a 4-D weight used for every frame of a clip gets the sum over the
frames.  The reference has no weights; that they are differentiable is ours.  ``encode`` / ``reconstruct`` outputs stay detached (through
them ``x`` has a zero gradient in the reference too).  Without either, no launch and no copy is added.

Likelihood maps: with ``model.likelihood_maps = True`` every call that evaluates an ELBO (``elbo``, ``weighted_elbo``, ``forward``,
``encode``, ``reconstruct``) leaves ``model.log_likelihood`` (B, 3, S, S) and ``model.K_log_likelihood`` (B, K, 3, S, S) of its last
evaluation, the two attributes of iodine.py:210-216 - an anomaly map, a per-slot "who explains this pixel" view, a way to choose
``weights=``.  Three deliberate differences from the reference: the maps are detached (the reference's are part of its graph), they are
raw under ``weights=`` (the weighted LL is ``sum_p w_p sum_c log_likelihood``), and they come from a kernel of their own, so their sum
over channels and pixels matches the reported LL to float32 rounding, not bitwise.  ``False`` (default): both are None, no launch runs.

Multi-sample evaluation: ``model.predictive(x, samples=S)`` draws S latents from one posterior (default: the one the last ``reconstruct`` /
``encode`` / ``forward`` left) and returns a ``Predictive`` - per-pixel mean and variance of the rendered image and of the masks, per-slot vote
counts with their arg-max and agreement, and with an image the per-sample log-likelihoods, the importance-weighted bound, the Monte-Carlo ELBO and
the closed-form-KL ELBO per image (``iodine_predictive``: the samples share one decoder pass per chunk and one per-pixel kernel keeps the running
moments; nothing per sample is written).  Not in the reference, which scores and renders one draw (iodine.py:103, 171).

Extensions over the reference: every entry point takes an optional ``eps`` tensor of shape
(T+1, B, K, L) replacing the ``torch.randn_like`` draws of ``Gaussian.sample``
(iodine.py:632) in call order, so that results can be compared with the CPU oracle.  Without
``eps`` the draws come from the library's own counter-based generator (Philox4x32-10,
``iodine_randn``; seed with ``model.manual_seed``) - no ATen COMPUTE kernel runs on the product path (what a kernel trace
still shows from ATen are autograd's own fills: ``loss.backward()`` seeds the scalar loss gradient with ``ones_like`` and
``zero_grad`` / the flat gradient buffer are fills - a handful of 5-us launches per training step, none of them arithmetic of the model).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib


class Logger:
    """Same role as lib/utils/vis_logger.py:30-50: a dict of the latest values."""

    def __init__(self):
        self.things = dict()

    def __getitem__(self, key):
        return self.things[key]

    def __contains__(self, key):
        return key in self.things

    def update(self, **kw):
        self.things.update(kw)


logger = Logger()


def _arch_get(arch, name, default=None):
    return getattr(arch, name, default)


class _MultiLayerConv(nn.Module):
    """Parameter container with the reference's names (iodine.py:570-584); never called."""

    def __init__(self, dim_in, dim_out, n_layers, kernel_size, stride=1):
        super().__init__()
        self.layers = nn.ModuleList()
        for _ in range(n_layers):
            self.layers.append(nn.Conv2d(dim_in, dim_out, kernel_size, stride=stride, padding=kernel_size // 2))
            dim_in = dim_out


class _MLP(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(dim_in, dim_out)])       # iodine.py:553-557


class _Refine(nn.Module):
    def __init__(self, dim_in, dim_conv, dim_hidden, dim_out, n_layers, kernel_size, stride):
        super().__init__()                                              # iodine.py:450-464
        self.mlc = _MultiLayerConv(dim_in, dim_conv, n_layers, kernel_size, stride)
        self.mlp = _MLP(dim_conv, dim_hidden)
        self.lstm = nn.LSTMCell(dim_hidden + 4 * dim_out, dim_hidden)
        self.mean_update = nn.Linear(dim_hidden, dim_out)
        self.logvar_update = nn.Linear(dim_hidden, dim_out)


class _Decoder(nn.Module):
    def __init__(self, dim_in, dim_hidden, n_layers, kernel_size):
        super().__init__()                                              # iodine.py:416-423
        self.mlc = _MultiLayerConv(dim_in + 2, dim_hidden, n_layers, kernel_size)
        self.conv = nn.Conv2d(dim_hidden, 4, kernel_size, stride=1, padding=kernel_size // 2)


class _Posterior(nn.Module):
    def __init__(self, dim_latent):
        super().__init__()                                              # iodine.py:596-604
        self.init_mean = nn.Parameter(torch.zeros(dim_latent))
        self.init_logvar = nn.Parameter(torch.zeros(dim_latent))
        self.mean = None
        self.logvar = None


@dataclasses.dataclass
class SceneEdit:
    """What ``IODINE.edit`` returns: the renderings of E single-slot edits of one decoded scene.  ``pred (E, 3, S, S)``; ``mask (E, K, 1, S,
    S)`` and ``mean (E, 3, S, S)`` - the sigmoid rgb of the slot-image put into the edited slot, of a removal that of the removed slot -
    where asked for, else None; ``base`` = ``(pred, mask, mean)`` of the unedited ``decode(z)`` or None.  Detached tensors."""
    pred: torch.Tensor
    mask: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None
    base: Optional[tuple] = None


@dataclasses.dataclass
class Predictive:
    """What ``IODINE.predictive`` returns: read-outs over ``samples`` draws from one posterior.  ``z (S, B, K, L)``; ``pred_mean`` /
    ``pred_var (B, 3, S, S)`` and ``mask_mean`` / ``mask_var (B, K, 1, S, S)`` - mean and population variance (M2 / S, exactly 0 for one
    sample) of the per-sample ``decode(z[s])``; ``votes (B, K, S, S)`` int32 - samples in which slot k wins the pixel; ``segmentation (B, S,
    S)`` uint8 - the arg-max of the votes (lowest index on a tie) - and ``agreement (B, S, S)`` - its share of the samples.  With an image
    also ``ll (S, B)`` - the (weighted) log-likelihood of each sample and image -, ``log_w (S, B)`` float64 = log p(x|z) + log p(z) - log q(z),
    ``iwae (B)`` = logsumexp_s(log_w) - log S, ``elbo_mc (B)`` = mean_s log_w, ``elbo (B)`` = mean_s ll - KL(q || N(0, 1)) in closed form;
    else None.  Detached tensors."""
    z: torch.Tensor
    pred_mean: torch.Tensor
    pred_var: torch.Tensor
    mask_mean: torch.Tensor
    mask_var: torch.Tensor
    votes: torch.Tensor
    segmentation: torch.Tensor
    agreement: torch.Tensor
    samples: int
    ll: Optional[torch.Tensor] = None
    log_w: Optional[torch.Tensor] = None
    iwae: Optional[torch.Tensor] = None
    elbo_mc: Optional[torch.Tensor] = None
    elbo: Optional[torch.Tensor] = None


def sample_bounds(ll, z, eps, post_mean, post_logvar):
    """The float64 host arithmetic behind ``Predictive``: per-sample log-likelihoods ``ll (S, B)``, the samples ``z`` and their noise ``eps
    (S, B, K, L)`` and the posterior (B, K, L) -> (log_w (S, B), iwae, elbo_mc, elbo (B)).  With z = mu + exp(logvar / 2) eps the
    densities are log p(z) - log q(z) = sum_{k,l} (-z^2 / 2 + eps^2 / 2 + logvar / 2) (the 2 pi terms cancel); the importance-weighted bound
    is taken around the maximum: max_s log_w + log mean_s exp(log_w - max), i.e. logsumexp_s(log_w) - log S, exactly log_w[0] for one sample."""
    S = ll.shape[0]
    z, eps, lv, mu = z.double(), eps.double(), post_logvar.double(), post_mean.double()
    log_w = ll.double() + (-0.5 * z * z + 0.5 * eps * eps + 0.5 * lv.unsqueeze(0)).sum((-2, -1))
    top = log_w.max(0).values
    iwae = top + torch.log(torch.exp(log_w - top).sum(0) / S)
    elbo_mc = log_w.sum(0) / S
    kl = 0.5 * (lv.exp() + mu * mu - 1.0 - lv).sum((-2, -1))
    return log_w, iwae, elbo_mc, ll.double().sum(0) / S - kl


@dataclasses.dataclass
class _RefineState:
    """(lambda_T, h, c) after the last encode / reconstruct, for ``IODINE.refinement_state``.  ``h`` / ``c`` are None while they
    are still in the library's workspace, which holds them until model call ``serial`` is followed by another; a chunked call that
    was not asked to keep its state leaves ``serial`` None too: its chunks' LSTM states are gone."""
    post_mean: torch.Tensor
    post_logvar: torch.Tensor
    h: Optional[torch.Tensor] = None
    c: Optional[torch.Tensor] = None
    serial: Optional[int] = None


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
            w = module._check_weights(w, x, what)
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
        ctx.serial = module._call_serial                   # identity of the saved forward (the library keeps exactly one)
        ctx.BK, ctx.attach, ctx.index = (x.shape[0], module.K), attach, index
        ctx.mark_non_differentiable(elbo_iter)
        if not attach:
            return (loss, elbo_iter, *frames)
        module._fetch_last_elbo(module._handle, x, elbo_iter[-1])      # (grad mode is off in here: the logger entries stay detached)
        module._fetch_posterior(module._handle, x.shape[0], x.device)
        h, c = module._fetch_train_state(x.shape[0], x.device)
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


_WRAPPER_OPTIONS = ('batch_cap',)      # max images per library call (IODINE.max_batch); the rest go to iodine_set_option


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
        T = module._shape[1] if module._shape is not None else int(module._cfg.iters)
        ctx.module, ctx.K, ctx.T, ctx.z_dtype = module, K, T, z.dtype
        ctx.chunks = module._chunks(z.shape[0], module.max_batch(K=K, T=T))
        zc = z.detach().to(torch.float32).contiguous()
        if len(ctx.chunks) == 1:
            out = module._decode_call(zc, K, T, save=True)
            ctx.serial = module._call_serial               # identity of the saved pass
        else:
            outs = [module._decode_call(zc[s:e], K, T, save=False) for s, e in ctx.chunks]
            out = tuple(torch.cat([o[j] for o in outs], 0) for j in range(3))
            ctx.z, ctx.versions = zc, module._param_versions
        return out

    @staticmethod
    def backward(ctx, g_pred, g_mask, g_mean):
        m = ctx.module
        want_z, want_p = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        if g_pred is None and g_mask is None and g_mean is None:
            return (None,) * len(ctx.needs_input_grad)
        if len(ctx.chunks) == 1:
            dz, flat = m._decode_backward(ctx.serial, ctx.K, (g_pred, g_mask, g_mean), want_z, want_p, None)
            flat = m._own(flat)
        else:
            m._sync_params(ctx.z.device)
            if m._param_versions != ctx.versions:
                raise RuntimeError('IODINE: backward of a stale decode - the parameters changed since the chunked decode ran (its chunks '
                                   'are decoded again in the backward; call backward() before the optimizer step)')
            dzs, flat = [], None
            for s, e in ctx.chunks:
                m._decode_call(ctx.z[s:e], ctx.K, ctx.T, save=True)
                gs = tuple(None if g is None else g[s:e] for g in (g_pred, g_mask, g_mean))
                dzc, flat = m._decode_backward(m._call_serial, ctx.K, gs, want_z, want_p, flat)
                dzs.append(dzc)
            dz = torch.cat(dzs, 0) if want_z else None
            flat = m._own(flat)
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
            ctx.serial, ctx.pre, ctx.BK = module._call_serial, None, (x.shape[0], module.K)
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
            flat = m._own(flat)
        gx, gw = _ig_grads(ctx, g, 1.0)
        return (None, gx, None, gw, gpm if ctx.needs_input_grad[4] else None, gplv if ctx.needs_input_grad[5] else None,
                *_flat_views(m, flat, live), *_sigma_tail(ctx, g, 1.0))


class IODINE(nn.Module):
    def __init__(self, ARCH):
        super().__init__()
        # same attribute reads as iodine.py:8-21
        self.dim_latent = ARCH.DIM_LATENT
        self.n_iters = ARCH.ITERS
        self.K = ARCH.SLOTS
        self.encodings = list(ARCH.ENCODING)
        self.img_channels = ARCH.IMG_CHANNELS
        self.img_size = ARCH.IMG_SIZE
        self.sigma = ARCH.SIGMA         # likelihood scale, read when a call starts (iodine.py:210)
        self.beta = 1.0                 # weight of the KL term: ELBO = LL - beta * KL; elbo_terms[:, 1] and the logger's kl stay the raw KL
        self.iter_weights = None        # loss weights of the T + 1 ELBO evaluations of forward: None / 'linspace', 'uniform', 'last', a sequence
        self.stable_encoding = False    # True: the mask_posterior channel of the refinement input as a max-subtracted softmax over the slots
                                        # (option stable_encoding) - finite where the reference's exp(s_k) / sum_j exp(s_j) is 0 / 0
        self.use_layernorm = ARCH.LAYERNORM
        self.use_stop_gradient = _arch_get(ARCH, 'STOP_GRADIENT', False)

        input_size, lambda_size = self.get_input_size()
        ref, dec = ARCH.REF, ARCH.DEC
        self.refine = _Refine(input_size, ref.CONV_CHAN, ref.MLP_UNITS, ARCH.DIM_LATENT, ref.CONV_LAYERS,
                              ref.KERNEL_SIZE, _arch_get(ref, 'STRIDE', 2))
        self.decoder = _Decoder(ARCH.DIM_LATENT, dec.CONV_CHAN, dec.CONV_LAYERS, dec.KERNEL_SIZE)
        self.posterior = _Posterior(self.dim_latent)

        self._cfg = _lib.Config(
            dim_latent=ARCH.DIM_LATENT, iters=ARCH.ITERS, slots=ARCH.SLOTS, img_size=ARCH.IMG_SIZE,
            img_channels=ARCH.IMG_CHANNELS, sigma=float(ARCH.SIGMA), layernorm=int(bool(ARCH.LAYERNORM)),
            stop_gradient=int(bool(self.use_stop_gradient)), encoding=_lib.encoding_bits(self.encodings),
            ref_conv_chan=ref.CONV_CHAN, ref_conv_layers=ref.CONV_LAYERS, ref_mlp_units=ref.MLP_UNITS,
            ref_kernel_size=ref.KERNEL_SIZE, ref_stride=_arch_get(ref, 'STRIDE', 2),
            dec_conv_chan=dec.CONV_CHAN, dec_conv_layers=dec.CONV_LAYERS, dec_kernel_size=dec.KERNEL_SIZE)

        # per-call state the reference keeps on self (iodine.py:36-52)
        self.lstm_hidden = None
        self.frames = None              # forward(x, attach_frames=...): the chosen ELBO evaluations (see forward)
        self.z = None
        self.mean = None
        self.mask_logits = None
        self.mask = None
        self.elbo_terms = None          # (n_elbo_calls, 3) = {ELBO, KL, LL} of the last call
        self.trajectory = None          # reconstruct(x, trajectory=True): dict of per-iteration outputs, else None
        self.objects = None             # reconstruct(x, objects=True): dict(table, segmentation, kl) of the returned decode, else None
        self.likelihood_maps = False    # True: every call that evaluates an ELBO also leaves the two per-pixel maps below (iodine.py:210-216)
        self.log_likelihood = None      # (B, 3, S, S)    logsumexp_k(log(mask + 1e-12) + K_log_likelihood) of the last ELBO evaluation
        self.K_log_likelihood = None    # (B, K, 3, S, S) gaussian_log_likelihood(x[:, None], mean, sigma); both float32, detached, raw

        self._handle = None
        self._handle_device = None
        self._param_versions = None
        self._workspace = None
        self._ws_key = None
        self._shape = None              # (slots, iters) the handle runs at (iodine_set_run_shape); follows self.K / self.n_iters
        self._frames = 0                # frames per call the handle expects (iodine_set_frames; 0 = one image)
        self._objective = None          # (sigma, beta, weights) the handle holds (iodine_set_objective); None: the constructor's
        self._modes = {}                # options stable_encoding / sigma_grad as the handle holds them (_ensure_objective)
        self._ig = 0                    # option input_grad as the handle holds it (_ensure_input_grad)
        self._last_ig = None            # (d / d x, d / d w) the last differentiable call accumulated, for its autograd node
        self._state = None              # _RefineState of the last encode / reconstruct: see refinement_state
        self._options: Dict[str, float] = {}
        self._seed = 0                  # Philox key of the library's normal generator (manual_seed)
        self._draws = 0                 # Philox stream id: one per eps draw
        self._call_serial = 0           # bumped by every compute call; a backward must match the forward that saved state
        self._graph_stream = None
        self._graph_bufs: Dict[tuple, torch.Tensor] = {}

    # ---- bookkeeping identical to the reference -------------------------------------------------
    def get_input_size(self):
        """iodine.py:345-374."""
        size, latent = 0, 0
        e, c = self.encodings, self.img_channels
        if 'grad_post' in e: latent += 2 * self.dim_latent
        if 'posterior' in e: latent += 2 * self.dim_latent
        for name, n in (('image', c), ('means', c), ('mask', 1), ('mask_logits', 1), ('mask_posterior', 1),
                        ('grad_means', c), ('grad_mask', 1), ('likelihood', 1), ('leave_one_out_likelihood', 1),
                        ('coordinate', 2)):
            if name in e:
                size += n
        return size, latent

    # ---- library plumbing ---------------------------------------------------------------------
    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().iodine_destroy(self._handle)
        except Exception:
            pass

    def _ordered_params(self):
        return [p for _, p in self.named_parameters()]

    def _ensure_handle(self, device: torch.device):
        if device.type != 'cuda':
            raise RuntimeError('iodine_amd.IODINE runs only on a ROCm device (gfx950); got tensors on '
                               f'{device}. There is no CPU fallback - move the module and inputs with .to("cuda").')
        L = _lib.lib()
        if self._handle is not None and self._handle_device != device:
            L.iodine_destroy(self._handle)
            self._handle, self._param_versions, self._workspace, self._ws_key, self._shape = None, None, None, None, None
        if self._handle is None:
            with torch.cuda.device(device):
                h = C.c_void_p()
                _lib.check(L.iodine_create(C.byref(self._cfg), C.byref(h)), None, 'iodine_create')
            self._handle, self._handle_device = h, device
            self._shape = (int(self._cfg.slots), int(self._cfg.iters))
            self._frames = 0
            self._objective = (float(self._cfg.sigma), 1.0, ())
            for k, v in self._options.items():
                if k in _WRAPPER_OPTIONS:
                    continue
                _lib.check(L.iodine_set_option(h, k.encode(), v), h)
            self._modes = {k: bool(self._options.get(k)) for k in ('stable_encoding', 'sigma_grad')}
            self._ig = int(self._options.get('input_grad', 0))
            names = []
            for i in range(L.iodine_num_params(h)):
                nm, nd, dims = C.c_char_p(), C.c_int(), (C.c_longlong * 4)()
                _lib.check(L.iodine_param_info(h, i, C.byref(nm), C.byref(nd), dims), h)
                names.append((nm.value.decode(), tuple(dims[:nd.value])))
            mine = [(n, tuple(p.shape)) for n, p in self.named_parameters()]
            if names != mine:
                raise RuntimeError(f'parameter table mismatch between module and library:\n{names}\n{mine}')
        return self._handle

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _launch(self, device, fn):
        """Run ``fn()`` (library calls on the current stream) with ``device`` current.  With option ``graph`` the calls go to
        a private non-default stream (the legacy null stream cannot be captured), ordered after / before the caller's."""
        with torch.cuda.device(device):
            if not self._options.get('graph'):
                return fn()
            if self._graph_stream is None or self._graph_stream.device != device:
                self._graph_stream = torch.cuda.Stream(device=device)
            cur = torch.cuda.current_stream()
            self._graph_stream.wait_stream(cur)
            with torch.cuda.stream(self._graph_stream):
                out = fn()
            cur.wait_stream(self._graph_stream)
            return out

    # With option ``graph`` the library keys its hipGraphs on the full argument tuple, device addresses included.  Tensors the
    # caching allocator hands out per call (inputs made contiguous, noise, outputs, the flat gradient buffer) would change that
    # key from step to step - every call an eager run or a re-capture instead of a replay.  So in graph mode the library only
    # ever sees persistent staging buffers owned by the module: inputs are copied in, outputs are cloned out.  Host-side scalars are baked
    # into captured nodes, so the key also holds the objective (sigma, beta, the weight table): a schedule that changes ``model.beta`` every
    # step sees each key once and simply runs eagerly, a repeated objective is captured and replayed.
    def _graph_on(self):
        return bool(self._options.get('graph'))

    def _gbuf(self, name, shape, device):
        key = (name, tuple(shape), str(device))
        t = self._graph_bufs.get(key)
        if t is None:
            t = self._graph_bufs[key] = torch.empty(tuple(shape), device=device, dtype=torch.float32)
        return t

    def _stage(self, name, t):
        """``t`` as the library should see it: itself, or (graph mode) its copy in the persistent buffer ``name``."""
        if t is None or not self._graph_on():
            return t
        buf = self._gbuf(name, t.shape, t.device)
        if buf.data_ptr() != t.data_ptr():
            buf.copy_(t)
        return buf

    def _out(self, name, shape, device):
        if self._graph_on():
            return self._gbuf(name, shape, device)
        return torch.empty(tuple(shape), device=device, dtype=torch.float32)

    def _own(self, t):
        """What the caller gets: the tensor itself, or (graph mode) a copy that the next call will not overwrite."""
        return t.clone() if (t is not None and self._graph_on()) else t

    def manual_seed(self, seed: int):
        """Seed of the library's generator for the ``eps=None`` draws (Philox4x32-10; give every rank its own seed)."""
        self._seed, self._draws = int(seed) & (2 ** 64 - 1), 0
        return self

    def mark_params_dirty(self):
        """Force a re-pack of the weights on the next call.  Needed only after writes that bypass autograd's version counter
        (``p.data.copy_(...)``, ``dist.broadcast(p.data, 0)``); optimizers, ``load_state_dict`` and ``.to()`` are seen."""
        self._param_versions = None

    def _sync_params(self, device):
        h = self._ensure_handle(device)
        params = self._ordered_params()
        for p in params:
            if p.device != device or p.dtype != torch.float32:
                raise RuntimeError('all parameters must be float32 on the same ROCm device as the input')
        versions = tuple((p.data_ptr(), p._version) for p in params)
        if versions != self._param_versions:
            keep = [p.detach().contiguous() for p in params]
            arr = (C.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
            _lib.check(_lib.lib().iodine_set_params(h, self._stream(), arr, len(keep)), h, 'iodine_set_params')
            self._param_versions = versions
        return h

    # ``model.K`` / ``model.n_iters`` are read when a call starts, as the reference reads them on every call (Gaussian.init_unit(B,
    # self.K), get_input_encoding's repeat over K, the loops of encode / forward: iodine.py:81-83,123-126,279,312).  No parameter
    # depends on either, so one set of weights runs at any (K, T); the library handle follows through iodine_set_run_shape.
    def _run_shape(self, K=None, T=None):
        """(K, T) of the call that is starting: ``self.K`` / ``self.n_iters`` unless given, checked on the host before any device work."""
        K = self.K if K is None else K
        T = self.n_iters if T is None else T
        if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= 16:
            raise ValueError(f'IODINE: the slot count (model.K) must be an integer in 1..16 - the per-pixel kernels keep every slot of '
                             f'a pixel in registers, instantiated for K <= 16; got {K!r}')
        if isinstance(T, bool) or int(T) != T or int(T) < 1:
            raise ValueError(f'IODINE: the iteration count (model.n_iters) must be an integer >= 1; got {T!r}')
        return int(K), int(T)

    # ``model.sigma`` / ``model.beta`` / ``model.iter_weights``: read when a call starts, like K / n_iters, and checked on the host before
    # any device work.  The handle follows through ONE iodine_set_objective call whenever any of the three differs from what it holds.
    def _read_objective(self, T):
        """(sigma, beta, weights) of the call that is starting at ``T`` iterations; weights: () = the default (i+1)/(T+1), else T + 1
        floats.  ValueError for anything the library would refuse.  Every entry point reads all three "at call time", so explicit
        ``iter_weights`` of the training length make encode / reconstruct / elbo at ANOTHER ``n_iters`` raise the length error although
        inference never uses the weights, and a named weighting sends its table for the T of an inference call too - set
        ``iter_weights = None`` (or a name) around evaluation at another iteration count."""
        import math
        import numbers

        def number(v, name, rule, ok):
            # a Python or numpy real number, or a tensor / array with one element - what a schedule usually produces
            if torch.is_tensor(v) and v.numel() == 1 and not v.is_complex():
                v = v.detach().item()
            elif not isinstance(v, numbers.Real) and getattr(v, 'size', None) == 1 and hasattr(v, 'item'):
                v = v.item()
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise ValueError(f'IODINE: model.{name} must be a finite number {rule}, given as a real number or a one-element '
                                 f'tensor; got {v!r} of type {type(v).__name__}')
            if not math.isfinite(v) or not ok(v):
                raise ValueError(f'IODINE: model.{name} must be a finite number {rule}; got {v!r}')
            return float(v)
        sigma = number(self.sigma, 'sigma', '> 0 (the likelihood scale)', lambda v: v > 0)
        beta = number(self.beta, 'beta', '>= 0 (the weight of the KL term)', lambda v: v >= 0)
        w = self.iter_weights
        if w is None or (isinstance(w, str) and w == 'linspace'):
            return sigma, beta, ()
        if isinstance(w, str):
            if w == 'uniform':
                return sigma, beta, (1.0 / (T + 1),) * (T + 1)
            if w == 'last':
                return sigma, beta, (0.0,) * T + (1.0,)
            raise ValueError(f"IODINE: model.iter_weights must be None, 'linspace', 'uniform', 'last' or a sequence of T + 1 numbers; "
                             f'got {w!r}')
        if torch.is_tensor(w):
            w = w.detach().reshape(-1).tolist()
        try:
            w = tuple(w)
        except TypeError:
            raise ValueError(f"IODINE: model.iter_weights must be None, 'linspace', 'uniform', 'last' or a sequence of T + 1 numbers; "
                             f'got {w!r}') from None
        if len(w) != T + 1:
            raise ValueError(f'IODINE: model.iter_weights has {len(w)} entries, but a call at n_iters = {T} makes {T + 1} ELBO '
                             f'evaluations and takes {T + 1} weights (or one of the names, which follow n_iters)')
        w = tuple(number(v, 'iter_weights[%d]' % i, '>= 0' , lambda v: v >= 0) for i, v in enumerate(w))
        if not any(C.c_float(v).value > 0 for v in w):
            raise ValueError(f'IODINE: model.iter_weights are all zero (as float32) - no evaluation would carry any loss; got {w!r}')
        return sigma, beta, w

    def _ensure_objective(self, h, obj, device, sigma_grad=False):
        """The objective of the call that is starting, ``model.stable_encoding`` and whether the call differentiates sigma (option
        sigma_grad; ``set_option('sigma_grad', 1)`` keeps it on for every call) on the handle - each sent only when it differs."""
        for key, want in (('stable_encoding', bool(self.stable_encoding)), ('sigma_grad', bool(sigma_grad or self._options.get('sigma_grad')))):
            if self._modes.get(key, False) != want:
                _lib.check(_lib.lib().iodine_set_option(h, key.encode(), float(want)), h, 'iodine_set_option')
                self._modes[key] = want
        if obj == self._objective:
            return
        sigma, beta, w = obj
        arr = (C.c_double * len(w))(*w) if w else None
        with torch.cuda.device(device):                     # (a new weight table is a small device allocation of the handle)
            _lib.check(_lib.lib().iodine_set_objective(h, sigma, beta, arr, len(w)), h, 'iodine_set_objective')
        self._objective = obj

    def _ensure_input_grad(self, h, bits):
        """Option input_grad (bit 1: image, bit 2: pixel weights) of the call that is starting, sent only when it differs;
        ``set_option('input_grad', bits)`` keeps bits on for every call.  Before ``_ensure_workspace``: the two accumulators are part of
        the workspace plan while a bit is set, so a change asks the library for the size again."""
        want = int(bits) | int(self._options.get('input_grad', 0))
        if want != self._ig:
            _lib.check(_lib.lib().iodine_set_option(h, b'input_grad', float(want)), h, 'iodine_set_option')
            self._ig, self._ws_key = want, None

    def _fetch_input_grad(self, h, dev, x, w, bits):
        """After a library call that ran with input_grad ``bits``: (G_x shaped like x, G_w shaped like w - ``_check_weights`` form), None
        where the bit is off - fresh tensors (iodine_last_input_grad)."""
        gx = torch.empty(x.shape, device=dev, dtype=torch.float32) if bits & 1 else None
        if not bits & 2:
            gw = None
        elif w is not None:
            gw = torch.empty(w.shape, device=dev, dtype=torch.float32)
        else:
            gw = torch.empty((x.shape[0], self.img_size, self.img_size), device=dev, dtype=torch.float32)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_last_input_grad(h, self._stream(), _lib.ptr(gx), _lib.ptr(gw)), h,
                                             'iodine_last_input_grad'))
        return gx, gw

    def _grad_inputs(self, x, weights, xc, wc):
        """What the autograd node of a call takes as image and weights: the caller's own tensors where they require grad (grad mode on) -
        the node converts them and returns their gradient -, else the checked, detached forms ``xc`` / ``wc``."""
        on = torch.is_grad_enabled()
        xi = x if on and x.requires_grad else xc
        wi = weights if on and wc is not None and weights.requires_grad else wc
        return xi, wi

    # ``model.sigma`` as a tensor that requires grad (a leaf, or e.g. ``log_sigma.exp()``): the value handed to the library is still a host
    # number - one ``.item()`` per call, and a sigma that changes every step runs eagerly in graph mode, like a beta schedule - and the
    # call also computes d LL / d sigma (option sigma_grad), which ``backward()`` turns into ``sigma.grad``.
    def _sigma_input(self):
        """() or (model.sigma,): the extra autograd input of a call that must differentiate sigma (grad mode on)"""
        s = self.sigma
        live = torch.is_tensor(s) and s.requires_grad and s.numel() == 1 and torch.is_grad_enabled()
        return (s,) if live else ()

    def _fetch_sigma_grad(self, h, dev, n, weights=None):
        """After a library call that ran with sigma_grad: sum_e w_e dLL_e/dsigma over its n evaluations (weights: the iteration weights it
        ran with, () = the default; None: n = 1, the value itself) as a device scalar."""
        out = self._out('t.dll', (n,), dev)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_last_sigma_grad(h, self._stream(), _lib.ptr(out), n), h,
                                             'iodine_last_sigma_grad'))
        if weights is None:
            return out[0].clone()
        wv = torch.tensor(list(weights) or [(i + 1) / n for i in range(n)], dtype=torch.float32, device=dev)
        return (wv * out).sum()

    def _ensure_workspace(self, h, B, mode, device, K, T, frames=None):
        """Run shape (K, T), frame count and a workspace planned for (B, mode, K, T, frames) on the handle.  ``frames``: 0 = one image
        per batch entry, E = a clip of E frames (iodine_set_frames); None = whatever the handle has (decode / elbo: no re-plan)."""
        if self._shape != (K, T):
            _lib.check(_lib.lib().iodine_set_run_shape(h, K, T), h, 'iodine_set_run_shape')
            self._shape = (K, T)
        if frames is not None and frames != self._frames:
            _lib.check(_lib.lib().iodine_set_frames(h, frames), h, 'iodine_set_frames')
            self._frames = frames
        key = (B, mode, K, T, self._frames, device)
        if self._ws_key == key:
            return
        need = _lib.lib().iodine_workspace_bytes(h, B, mode)
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
            self._workspace = None
            self._workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().iodine_set_workspace(h, C.c_void_p(self._workspace.data_ptr()),
                                                   self._workspace.numel()), h, 'iodine_set_workspace')
        self._ws_key = key

    def _check_x(self, x):
        if x.dim() != 4 or x.shape[1] != self.img_channels or x.shape[2] != self.img_size or x.shape[3] != self.img_size:
            raise RuntimeError(f'expected images of shape (B, {self.img_channels}, {self.img_size}, {self.img_size}), '
                               f'got {tuple(x.shape)}')
        return x.detach().to(torch.float32).contiguous()

    def _check_frames(self, x, E, what):
        """``x`` of a call that makes ``E`` ELBO evaluations -> (x, frames): images (B, C, S, S) -> frames 0; a clip (B, E, C, S, S),
        batch first, one frame per evaluation -> frames E.  Any other frame count is refused - never clamped or repeated."""
        if x.dim() != 5:
            return self._check_x(x), 0
        c, s = self.img_channels, self.img_size
        if tuple(x.shape[1:]) != (E, c, s, s):
            raise RuntimeError(f'{what} at n_iters = {self.n_iters} makes {E} ELBO evaluations: expected a clip of shape '
                               f'(B, {E}, {c}, {s}, {s}), one frame per evaluation, or images (B, {c}, {s}, {s}); got {tuple(x.shape)}')
        return x.detach().to(torch.float32).contiguous(), E

    def _check_weights(self, weights, x, what):
        """``weights=`` of a call on ``x`` (as given: images (B, C, S, S) or a clip (B, E, C, S, S)) -> None, or contiguous float32 on
        x's device: (B, S, S), or (B, E, S, S) for one weight image per frame.  Accepted: (B, 1, S, S) / (B, S, S), with a clip also
        (B, E, 1, S, S) / (B, E, S, S) - a 4-D (B, 1, S, S) weight goes to every frame.  Refused before any device work, like
        ``_check_frames``; the values (finite, >= 0) are the caller's contract.  Weights are data: detached."""
        if weights is None:
            return None
        if not torch.is_tensor(weights):
            raise RuntimeError(f'IODINE.{what}: weights must be a tensor of per-pixel weights (bool, uint8 or a float dtype), or None; got '
                               f'{type(weights).__name__}')
        if not (weights.dtype in (torch.bool, torch.uint8) or weights.is_floating_point()):
            raise RuntimeError(f'IODINE.{what}: weights must have dtype bool, uint8 or a float dtype; got {weights.dtype}')
        B, s = x.shape[0], self.img_size
        E = x.shape[1] if x.dim() == 5 else None
        got = tuple(weights.shape)
        per_frame = False
        if got in ((B, 1, s, s), (B, s, s)):
            pass
        elif E is not None and got in ((B, E, 1, s, s), (B, E, s, s)):
            per_frame = True
        else:
            if weights.dim() == 5 and E is None:
                raise RuntimeError(f'IODINE.{what}: weights of shape {got} hold one weight image per frame, but x {tuple(x.shape)} is a '
                                   f'batch of single images: expected weights ({B}, 1, {s}, {s}) or ({B}, {s}, {s})')
            clip = f', or ({B}, {E}, 1, {s}, {s}) / ({B}, {E}, {s}, {s}) - one weight image per frame' if E is not None else ''
            raise RuntimeError(f'IODINE.{what}: weights must have shape ({B}, 1, {s}, {s}) or ({B}, {s}, {s}){clip}, matching x '
                               f'{tuple(x.shape)}; got {got}')
        w = weights.detach().to(device=x.device, dtype=torch.float32)
        return w.reshape((B, E, s, s) if per_frame else (B, s, s)).contiguous()

    def _send_weights(self, h, w):
        """Hand ``w`` (``_check_weights``; None: nothing to do, the library's default is no weights) to the handle for the compute call
        that follows (iodine_set_pixel_weights: consumed and cleared by that call).  Graph mode: through the staging buffer 'w', like x."""
        if w is None:
            return None
        L = _lib.lib()
        if not hasattr(L, 'iodine_set_pixel_weights'):
            raise RuntimeError('IODINE: weights= needs iodine_set_pixel_weights, which this build of libiodine_hip.so does not have')
        ws = self._stage('w', w)
        _lib.check(L.iodine_set_pixel_weights(h, _lib.ptr(ws), 1 if ws.dim() == 4 else 0), h, 'iodine_set_pixel_weights')
        return ws

    def _check_state(self, state, B, K, device):
        """``state=`` of encode / reconstruct: (post_mean, post_logvar (B, K, L), h, c (B, K, MLP_UNITS)) as refinement_state returns it."""
        if state is None:
            return None
        L, H = self.dim_latent, int(self._cfg.ref_mlp_units)
        want = ((B, K, L), (B, K, L), (B, K, H), (B, K, H))
        if not isinstance(state, (tuple, list)) or len(state) != 4 or any(not torch.is_tensor(t) for t in state):
            raise RuntimeError('state must be the tuple (post_mean, post_logvar, h, c) that model.refinement_state() returns')
        got = tuple(tuple(t.shape) for t in state)
        if got != want:
            raise RuntimeError(f'state does not match this call: (B, K) = ({B}, {K}) needs tensors of shapes {want}, got {got}')
        return tuple(t.detach().to(device=device, dtype=torch.float32).contiguous() for t in state)

    def _check_train_state(self, state, B, K, device):
        """``state=`` of forward: the tuple of ``_check_state`` with h / c given as (B, K, MLP_UNITS) or as the reference's (B * K,
        MLP_UNITS) (``lstm_hidden``, iodine.py:37).  NOT detached: tensors that require grad stay connected to the caller's graph."""
        if state is None:
            return None
        L, H = self.dim_latent, int(self._cfg.ref_mlp_units)
        if not isinstance(state, (tuple, list)) or len(state) != 4 or any(not torch.is_tensor(t) for t in state):
            raise RuntimeError('state must be the tuple (post_mean, post_logvar, h, c) that model.refinement_state() returns')
        got = tuple(tuple(t.shape) for t in state)
        ok = got[0] == (B, K, L) and got[1] == (B, K, L) and all(g in ((B, K, H), (B * K, H)) for g in got[2:])
        if not ok:
            raise RuntimeError(f'state does not match this call: (B, K) = ({B}, {K}) needs post_mean, post_logvar of shape {(B, K, L)} and '
                               f'h, c of shape {(B, K, H)} (or {(B * K, H)}, as model.lstm_hidden); got {got}')
        shapes = ((B, K, L), (B, K, L), (B, K, H), (B, K, H))
        return tuple(t.to(device=device, dtype=torch.float32).reshape(shp).contiguous() for t, shp in zip(state, shapes))

    def _eps(self, eps, B, device):
        shape = (self.n_iters + 1, B, self.K, self.dim_latent)
        return self._normals(eps, shape, device)

    def _normals(self, eps, shape, device):
        if eps is None:
            out = self._out('eps', shape, device)
            self._launch(device, lambda: _lib.check(_lib.lib().iodine_randn(self._stream(), _lib.ptr(out), out.numel(),
                                                                          self._seed, self._draws), None, 'iodine_randn'))
            self._draws += 1
            return out
        if tuple(eps.shape) != shape:
            raise RuntimeError(f'eps must have shape {shape}, got {tuple(eps.shape)}')
        return self._stage('eps', eps.detach().to(device=device, dtype=torch.float32).contiguous())

    def debug_buffer(self, name: str, iteration: int = 0) -> torch.Tensor:
        """Copy of an internal workspace buffer of the last call (tests only)."""
        h = self._handle
        n = C.c_size_t()
        L = _lib.lib()
        _lib.check(L.iodine_debug_copy(h, self._stream(), name.encode(), iteration, None, 0, C.byref(n)), h)
        out = torch.empty(n.value, dtype=torch.float32, device=self._handle_device)
        _lib.check(L.iodine_debug_copy(h, self._stream(), name.encode(), iteration, C.c_void_p(out.data_ptr()),
                                       n.value, C.byref(n)), h)
        return out

    def set_option(self, key: str, value: float):
        """Debug/test options of the library (e.g. ``stop_after_iters``); applied to the live handle.  ``graph``: hipGraph replay of the
        fixed-shape launch sequences, one graph per distinct argument tuple - which includes ``model.sigma`` / ``beta`` / ``iter_weights``:
        an objective that changes every step (a beta warm-up) runs eagerly until it repeats.  ``conv_precision``: 0 = exact fp32 MFMA (the
        strict path), 1 = split fp16, three MFMAs per product, fp32-class (default), 2 = as 1 except that the weight-stationary decoder
        convs (3 x 3, 32 / 64 channels, power-of-two image sizes >= 16, ``conv_variant`` 6) form each product from ONE fp16 MFMA of operands
        rounded to nearest even at their cell / tensor scale: fp16-class forward and data gradient for faster evaluation (``reconstruct``,
        ``predictive``, ``edit``, ``decode``); every other kernel, and every shape that kernel does not run, computes what 1 computes.
        Training at 2 is differentiated consistently, its gradients are outside the 1e-3 budget.  tests/f16x1_reference.py defines the mode."""
        self._options[key] = float(value)
        if key in _WRAPPER_OPTIONS:                 # handled by this wrapper, unknown to the library
            return
        if key == 'stable_encoding':                # the same switch as the attribute, which every call reads
            self.stable_encoding = bool(value)
        if self._handle is not None:
            _lib.check(_lib.lib().iodine_set_option(self._handle, key.encode(), float(value)), self._handle)
            if key in self._modes:
                self._modes[key] = bool(value)
        if key in ('conv_precision', 'conv_variant', 'gen_conv_precision'):
            self._param_versions = None          # the library keeps only the selected path's weight packs: re-send the parameters
        if key == 'input_grad':
            self._ig = int(value)
        if key in ('wgrad_accum', 'input_grad'):
            self._ws_key = None                  # the workspace plan depends on it: ask the library again

    def profile_read(self, category: str, reset: bool = True):
        """(total_ms, launches) of one kernel category measured with HIP events (set_option('profile', 2); level 1 brackets the
        dominant ``conv_tile_*`` launches only)."""
        tot, cnt = C.c_double(), C.c_longlong()
        _lib.check(_lib.lib().iodine_profile_read(self._handle, category.encode(), C.byref(tot), C.byref(cnt),
                                                  int(reset)), self._handle)
        return tot.value, cnt.value

    # ---- inference: iodine.py:59-112 ------------------------------------------------------------
    def max_batch(self, training: bool = False, K: Optional[int] = None, T: Optional[int] = None) -> int:
        """Images one library call takes: the kernels index an activation tensor [B*K][pixels][channels] with 32-bit element
        offsets (check_ready in iodine_plan.cpp / train_forward_check in iodine_checks.cpp).  Larger batches are run in chunks of at most this many
        images by the methods below - images are independent.  The ``batch_cap`` option lowers it (tests).
        K / T: the shape of the call (default ``self.K`` / ``self.n_iters``)."""
        K, T = self._run_shape(K, T)
        P = self.img_size * self.img_size
        cd, cr = int(self._cfg.dec_conv_chan), int(self._cfg.ref_conv_chan)
        lim = ((1 << 31) - 1) // (K * P * max(cd, cr, 20))
        if training:
            lim = min(lim, ((1 << 31) - 1) // (K * T * P * 20), ((1 << 31) - 1) // (K * T * max(((self.img_size - 1) // max(int(self._cfg.ref_stride), 1) + 1) ** 2, 1) * cr))
        cap = int(self._options.get('batch_cap', 0))
        return max(1, min(lim, cap) if cap > 0 else lim)

    @staticmethod
    def _chunks(B, cap):
        """Balanced split of B images into ceil(B / cap) runs: [(start, stop), ...]."""
        n = -(-B // cap)
        base, extra = divmod(B, n)
        out, s = [], 0
        for i in range(n):
            e = s + base + (1 if i < extra else 0)
            out.append((s, e))
            s = e
        return out

    def _merge_chunk_state(self, parts, sizes, x):
        """Per-call state and logger entries of a chunked call, as one call over the whole batch would have left them: tensors
        over the batch concatenated, batch means (ELBO terms) weighted by the chunks' sizes, image-0 entries from chunk 0."""
        B = float(sum(sizes))
        cat = lambda key: torch.cat([p[key] for p in parts], 0)
        self.z, self.mean, self.mask, self.mask_logits = cat('z'), cat('mean'), cat('mask'), cat('mask_logits')
        maps = parts[0]['ll'] is not None
        self.log_likelihood, self.K_log_likelihood = (cat('ll'), cat('kll')) if maps else (None, None)
        self.elbo_terms = sum(p['elbo_terms'] * (n / B) for p, n in zip(parts, sizes))
        logger.update(**parts[0]['logger0'])
        if self.elbo_terms.shape[0] > 0:
            logger.update(kl=self.elbo_terms[-1, 1], likelihood=self.elbo_terms[-1, 2])

    def _chunk_state(self):
        keep = ('image', 'pred') + tuple(f'mask_{i}' for i in range(self.K)) + tuple(f'pred_{i}' for i in range(self.K))
        return dict(z=self.z, mean=self.mean, mask=self.mask, mask_logits=self.mask_logits, elbo_terms=self.elbo_terms,
                    ll=self.log_likelihood, kll=self.K_log_likelihood,
                    logger0={k: logger[k] for k in keep if k in logger})

    def _fetch_last_elbo(self, h, x, terms, count=None, frame=-1):
        """State the reference leaves on ``self`` after an ``elbo()`` call (iodine.py:171-187) and its logger entries
        (iodine.py:225-239): z, mean, mask, mask_logits of the whole batch and pred/image of image 0 (of a clip: its frame
        ``frame``, the one that call scored)."""
        dev, B = x.device, x.shape[0]
        K, L, S = self.K, self.dim_latent, self.img_size
        f = dict(device=dev, dtype=torch.float32)
        z, mean = torch.empty((B, K, L), **f), torch.empty((B, K, 3, S, S), **f)
        mask, logits, pred = torch.empty((B, K, 1, S, S), **f), torch.empty((B, K, 1, S, S), **f), torch.empty((B, 3, S, S), **f)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_last_elbo_outputs(
            h, self._stream(), B, _lib.ptr(z), _lib.ptr(mean), _lib.ptr(mask), _lib.ptr(logits), _lib.ptr(pred)),
            h, 'iodine_last_elbo_outputs'))
        self.z, self.mean, self.mask, self.mask_logits = z, mean, mask, logits
        self.log_likelihood = self.K_log_likelihood = None
        if self.likelihood_maps:                            # (one more per-pixel launch; off: none)
            ll, kll = torch.empty((B, 3, S, S), **f), torch.empty((B, K, 3, S, S), **f)
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_last_likelihood(h, self._stream(), B, _lib.ptr(ll), _lib.ptr(kll)),
                                                 h, 'iodine_last_likelihood'))
            self.log_likelihood, self.K_log_likelihood = ll, kll
        logger.update(image=x[0] if x.dim() == 4 else x[0, frame], pred=pred[0], kl=terms[1], likelihood=terms[2])
        logger.update(**{f'mask_{i}': mask[0, i, 0] for i in range(K)})
        logger.update(**{f'pred_{i}': mean[0, i] for i in range(K)})

    def _fetch_posterior(self, h, B, dev):
        """``self.posterior.mean / logvar`` = lambda_T, what ``Gaussian.update`` (iodine.py:636-645) leaves on the reference's
        module after ``forward``: a following ``model.elbo(x)`` samples from it."""
        pm = torch.empty((B, self.K, self.dim_latent), device=dev, dtype=torch.float32)
        plv = torch.empty_like(pm)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_last_posterior(h, self._stream(), B, _lib.ptr(pm), _lib.ptr(plv)),
                                             h, 'iodine_last_posterior'))
        self.posterior.mean, self.posterior.logvar = pm, plv

    @torch.no_grad()
    def _reconstruct(self, x, eps, want_images=True, state=None, trajectory=False, keep_state=False, weights=None):
        K, T = self._run_shape()
        obj = self._read_objective(T)
        x, frames = self._check_frames(x, T, 'encode / reconstruct')
        weights = self._check_weights(weights, x, 'encode / reconstruct')
        dev, B = x.device, x.shape[0]
        stop = int(self._options.get('stop_after_iters', -1))
        n_it = stop if 0 <= stop <= T else T
        if trajectory and n_it != T:
            raise RuntimeError('trajectory=True needs the whole call: its last entry is the final decode, which option stop_after_iters '
                               'skips (unset it with set_option("stop_after_iters", -1))')
        state = self._check_state(state, B, K, dev)
        self.trajectory, self._state, self.objects = None, None, None
        cap = self.max_batch()
        if B > cap:                                   # chunks of independent images; eps (T+1, B, K, L) is cut along B
            # the next chunk re-uses the workspace, so the LSTM state of a chunk is fetched (two small copies) only where the caller
            # uses the new arguments at all: a chunked call without them runs what it ran before
            keep_state = keep_state or state is not None or trajectory
            outs, parts, sizes, pms, plvs, trs, sts = [], [], [], [], [], [], []
            for s, e in self._chunks(B, cap):
                outs.append(self._reconstruct(x[s:e], None if eps is None else eps[:, s:e], want_images,
                                              None if state is None else tuple(t[s:e] for t in state), trajectory,
                                              weights=None if weights is None else weights[s:e]))
                parts.append(self._chunk_state()); sizes.append(e - s)
                pms.append(self.posterior.mean); plvs.append(self.posterior.logvar)
                trs.append(self.trajectory)
                if keep_state:
                    sts.append(self.refinement_state())
            self.posterior.mean, self.posterior.logvar = torch.cat(pms, 0), torch.cat(plvs, 0)
            self._merge_chunk_state(parts, sizes, x)
            if trajectory:                            # iteration first: the batch is axis 1
                self.trajectory = {k: torch.cat([t[k] for t in trs], 1) for k in trs[0]}
            self._state = _RefineState(self.posterior.mean, self.posterior.logvar)
            if keep_state:
                self._state.h, self._state.c = torch.cat([st[2] for st in sts], 0), torch.cat([st[3] for st in sts], 0)
            return tuple(None if outs[0][j] is None else torch.cat([o[j] for o in outs], 0) for j in range(4))
        h = self._sync_params(dev)
        self._ensure_workspace(h, B, 0, dev, K, T, frames)
        self._ensure_objective(h, obj, dev)
        eps = self._eps(eps, B, dev)
        xs = self._stage('x', x)
        L, S = self.dim_latent, self.img_size
        pred = self._out('r.pred', (B, 3, S, S), dev) if want_images else None
        mask = self._out('r.mask', (B, K, 1, S, S), dev) if want_images else None
        mean = self._out('r.mean', (B, K, 3, S, S), dev) if want_images else None
        z = self._out('r.z', (B, K, L), dev)
        pm, plv = self._out('r.pm', (B, K, L), dev), self._out('r.plv', (B, K, L), dev)
        elbo = self._out('r.elbo', (n_it, 3), dev)
        args = [_lib.ptr(t) for t in (xs, eps, pred, mask, mean, z, pm, plv, elbo)]
        self._call_serial += 1
        ws = self._send_weights(h, weights)                 # (ws: alive until the call is queued)
        if state is None and not trajectory:
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_reconstruct(h, self._stream(), B, *args), h, 'iodine_reconstruct'))
        else:
            # the initial state and the trajectory buffers go through persistent staging buffers in graph mode, like every other tensor
            state_in, state_ptrs, traj_out, traj_ptrs = None, None, None, None
            traj_names = ('pred', 'mask', 'mean', 'kl', 'll')
            if state is not None:
                state_in = [self._stage('s.' + n, t) for n, t in zip(('pm', 'plv', 'h', 'c'), state)]
                state_ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in state_in])
            if trajectory:
                shapes = ((T + 1, B, 3, S, S), (T + 1, B, K, 1, S, S), (T + 1, B, K, 3, S, S), (T, B), (T, B))
                traj_out = [self._out('tr.' + n, shp, dev) for n, shp in zip(traj_names, shapes)]
                traj_ptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in traj_out])
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_reconstruct_seq(
                h, self._stream(), B, *args, state_ptrs, traj_ptrs), h, 'iodine_reconstruct_seq'))
            if trajectory:
                self.trajectory = {n: self._own(t) for n, t in zip(traj_names, traj_out)}
        pred, mask, mean, z, pm, plv, elbo = (self._own(t) for t in (pred, mask, mean, z, pm, plv, elbo))
        self.posterior.mean, self.posterior.logvar, self.elbo_terms = pm, plv, elbo
        self._state = _RefineState(pm, plv, serial=self._call_serial)   # h, c stay in the workspace until asked for (refinement_state)
        if n_it > 0:
            self._fetch_last_elbo(h, x, elbo[-1], frame=n_it - 1)   # what the reference's last elbo() call left behind
        return pred, mask, mean, z

    def encode(self, x, eps=None, state=None, keep_state=False, weights=None):
        """z (B, K, L) after T refinement iterations.  iodine.py:73-105.  ``x``: images (B, 3, S, S) or a clip (B, T, 3, S, S) -
        iteration i then scores, differentiates and encodes frame i.  ``state`` / ``keep_state`` / ``weights``: see ``reconstruct``."""
        return self._reconstruct(x, eps, want_images=False, state=state, keep_state=keep_state, weights=weights)[3]

    def reconstruct(self, x, eps=None, trajectory=False, state=None, keep_state=False, weights=None, objects=False):
        """pred (B,3,S,S), mask (B,K,1,S,S), mean (B,K,3,S,S).  iodine.py:107-112.

        ``x``: images (B, 3, S, S), or a clip (B, T, 3, S, S), batch first: ELBO evaluation i uses frame ``x[:, i]`` for the
        likelihood, the inner gradients and the image-shaped encoding channels (the final sample + decode involves no image); any
        other frame count is a RuntimeError.  ``self.z / mean / mask / mask_logits`` and the logger entries are those of the last
        ELBO evaluation as before; the logger's ``image`` is ``x[0, T-1]``.

        ``trajectory=True`` leaves ``model.trajectory`` = dict(pred (T+1,B,3,S,S), mask (T+1,B,K,1,S,S), mean (T+1,B,K,3,S,S), kl (T,B),
        ll (T,B)), iteration first like ``eps`` and ``elbo_terms``: entry j < T is the decode ELBO evaluation j made (the sample from
        lambda_j, scored against frame j - with a clip the segmentation of frame j), entry T the final decode = the returned tuple;
        kl / ll are the per-image terms behind ``elbo_terms[:, 1:3]``.  Otherwise no extra launch runs and ``model.trajectory`` is None.

        ``state``: a tuple from ``model.refinement_state()`` for this (B, K) - the call starts from it instead of the initial posterior
        and a zero LSTM state and runs ``n_iters`` FURTHER iterations: T = 4 equals T = 2 followed by T = 2 from the state, bit for
        bit, given the matching slices of ``x`` and ``eps``.

        ``keep_state``: matters only where the batch exceeds ``max_batch()`` and runs in chunks.  Every chunk re-uses the workspace,
        so the LSTM state of a chunked call has to be copied out chunk by chunk; that is done when ``keep_state``, ``state`` or
        ``trajectory`` is given, and ``refinement_state()`` after a chunked call without any of them is refused.

        ``weights``: per-pixel observation weights >= 0 of this call, (B, 1, S, S) / (B, S, S), with a clip also (B, T, 1, S, S) /
        (B, T, S, S); see the module docstring for what is weighted.  The refinement then explains the weighted pixels only - a weight
        of 0 takes a pixel out of the objective - while ``pred`` / ``mask`` / ``mean`` are still rendered everywhere (inpainting).

        ``objects=True`` leaves ``model.objects`` = dict(table (B,K,14), segmentation (B,S,S) uint8, kl (B,K)): the per-slot table and
        argmax map of ``iodine_amd.objects.slot_table`` on the returned ``mask`` / ``mean`` (one more launch, after the call, so a chunked
        batch needs nothing special) and the per-slot KL of the final posterior against N(0, 1), ``0.5 sum_L(exp(lv) + m^2 - 1 - lv)`` -
        the usual "is this slot used" signal.  With ``trajectory=True`` as well, ``model.trajectory`` gains ``table (T+1,B,K,14)`` and
        ``segmentation (T+1,B,S,S)`` of every entry; entry T is ``model.objects``.  Every encode / reconstruct without it sets
        ``model.objects = None``, adds no launch and returns the same bits."""
        pred, mask, mean, _ = self._reconstruct(x, eps, state=state, trajectory=trajectory, keep_state=keep_state, weights=weights)
        if objects:
            self._read_objects(mask, mean, trajectory)
        return pred, mask, mean

    @torch.no_grad()
    def _read_objects(self, mask, mean, trajectory):
        """``model.objects`` (and the trajectory's tables) of a finished reconstruct: see there."""
        from .objects import slot_table
        pm, plv = self.posterior.mean.double(), self.posterior.logvar.double()    # (B, K, L): tiny; fp64 keeps exp(lv) - 1 - lv near lv = 0
        kl = (0.5 * (plv.exp() + pm * pm - 1.0 - plv).sum(-1)).float()
        if trajectory:                                # one launch over all T + 1 entries; the last is the returned decode
            table, seg = slot_table(self.trajectory['mask'], self.trajectory['mean'], segmentation=True)
            self.trajectory['table'], self.trajectory['segmentation'] = table, seg
            table, seg = table[-1], seg[-1]
        else:
            table, seg = slot_table(mask, mean, segmentation=True)
        self.objects = {'table': table, 'segmentation': seg, 'kl': kl}

    @torch.no_grad()
    def refinement_state(self):
        """Clones of (post_mean, post_logvar (B, K, L), h, c (B, K, MLP_UNITS)) after the last ``encode`` / ``reconstruct``: lambda_T
        and the LSTM state in torch order, as RefinementNetwork.forward returns it (iodine.py:503) - the ``state=`` of a continuing
        call.  The LSTM state of an un-chunked call stays in the library's workspace until asked for: the first call of this method
        must come before the next model call (forward / reconstruct / encode / decode / elbo re-use the workspace).  A state once
        fetched stays until the next ``encode`` / ``reconstruct`` replaces it or a training ``forward`` discards it.  After
        ``forward(..., keep_state=True)`` it returns (lambda_T, h_T, c_T) of that training forward, detached - the ``state=`` of the next
        chunk of a clip."""
        st = self._state
        if st is None:
            raise RuntimeError('IODINE.refinement_state: no encode / reconstruct has run since the module was made or trained (a training '
                               'forward keeps its final state only when called with keep_state=True)')
        if st.h is None:
            if st.serial is None:
                raise RuntimeError('IODINE.refinement_state: the last encode / reconstruct ran in chunks (batch > max_batch()), which '
                                   're-use the workspace - pass keep_state=True to that call to have each chunk\'s LSTM state copied out')
            if st.serial != self._call_serial:
                raise RuntimeError('IODINE.refinement_state: another model call has re-used the workspace since the encode / reconstruct '
                                   'whose state is asked for - call refinement_state() right after it')
            h, dev = self._handle, self._handle_device
            B, K = st.post_mean.shape[:2]
            st.h = torch.empty((B, K, int(self._cfg.ref_mlp_units)), device=dev, dtype=torch.float32)
            st.c = torch.empty_like(st.h)
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_last_refine_state(h, self._stream(), B, _lib.ptr(st.h), _lib.ptr(st.c)),
                                                 h, 'iodine_last_refine_state'))
        return tuple(t.clone() for t in (st.post_mean, st.post_logvar, st.h, st.c))

    def decode(self, z, differentiable=None):
        """iodine.py:59-71: z (B, K', L) -> pred (B,3,S,S), mask (B,K',1,S,S), mean (B,K',3,S,S).  Like the reference (iodine.py:430)
        the slot count comes from z itself - a single slot's latent decodes alone - and ``self.K`` is left as it is.

        ``differentiable``: None (default) - the outputs carry an autograd graph into ``z`` and the ``decoder.*`` parameters iff grad
        mode is on and ``z`` requires grad, as the reference's plain autograd code would; True - also when only the parameters do
        (decoder-only fine-tuning); False - never.  The outputs are the same bits either way.  The library keeps the state of ONE
        differentiable call: run ``backward()`` before the next model call (the error of a stale backward says so)."""
        if z.dim() != 3 or z.shape[2] != self.dim_latent or not 1 <= z.shape[1] <= 16:
            raise ValueError(f'IODINE.decode: z must have shape (B, K, {self.dim_latent}) with 1 <= K <= 16 (the per-pixel kernels are '
                             f'instantiated for K <= 16); got {tuple(z.shape)}')
        if differentiable is None:
            differentiable = z.requires_grad
        if differentiable and torch.is_grad_enabled():
            return _DecodeGrad.apply(self, z, *self._ordered_params())
        return self._decode_nograd(z)

    @torch.no_grad()
    def _decode_nograd(self, z):
        K = int(z.shape[1])
        # the iteration count plays no part in a decode: keep the handle's (no workspace re-plan for it)
        T = self._shape[1] if self._shape is not None else int(self._cfg.iters)
        z = z.detach().to(torch.float32).contiguous()
        B = z.shape[0]
        cap = self.max_batch(K=K, T=T)
        if B > cap:
            outs = [self._decode_nograd(z[s:e]) for s, e in self._chunks(B, cap)]
            return tuple(torch.cat([o[j] for o in outs], 0) for j in range(3))
        return self._decode_call(z, K, T, save=False)

    def _saving(self, h, on):
        """Option save_for_backward of the library for the call that follows (workspace mode 2; see include/iodine_hip.h)."""
        _lib.check(_lib.lib().iodine_set_option(h, b'save_for_backward', 1.0 if on else 0.0), h, 'iodine_set_option')

    def _decode_call(self, z, K, T, save):
        """One iodine_decode of at most ``max_batch`` slots-images; ``save``: kept for iodine_decode_backward."""
        dev, B = z.device, z.shape[0]
        h = self._sync_params(dev)
        self._ensure_workspace(h, B, 2 if save else 0, dev, K, T)
        S = self.img_size
        z = self._stage('d.z', z)
        pred, mask, mean = self._out('r.pred', (B, 3, S, S), dev), self._out('r.mask', (B, K, 1, S, S), dev), self._out('r.mean', (B, K, 3, S, S), dev)
        self._call_serial += 1
        if save:
            self._saving(h, True)
        try:
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_decode(h, self._stream(), B, _lib.ptr(z), _lib.ptr(pred),
                                                                          _lib.ptr(mask), _lib.ptr(mean)), h, 'iodine_decode'))
        finally:
            if save:
                self._saving(h, False)
        return self._own(pred), self._own(mask), self._own(mean)

    @staticmethod
    def _int_list(v, name, E=None):
        """An int sequence or integer tensor of edits -> list of Python ints (host values: the library checks them before any launch)."""
        if torch.is_tensor(v):
            if v.dim() != 1 or v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
                raise ValueError(f'IODINE.edit: {name} must be a 1-D integer tensor or a sequence of ints; got {v.dtype} of shape {tuple(v.shape)}')
            v = v.detach().cpu().tolist()
        else:
            try:
                v = list(v)
            except TypeError:
                raise ValueError(f'IODINE.edit: {name} must be a sequence of ints or a 1-D integer tensor; got {type(v).__name__}') from None
            if any(isinstance(i, bool) or int(i) != i for i in v):
                raise ValueError(f'IODINE.edit: {name} must hold integers; got {v!r}')
            v = [int(i) for i in v]
        if E is not None and len(v) != E:
            raise ValueError(f'IODINE.edit: {name} has {len(v)} entries, but there are {E} edits (one entry per edit)')
        return v

    @torch.no_grad()
    def edit(self, z, image, slot, z_new=None, remove=None, *, return_mask=False, return_mean=False, return_base=False):
        """E renderings of the scene ``decode(z)`` that each differ from it in ONE slot: edit e replaces slot ``slot[e]`` of image
        ``image[e]`` by the decode of ``z_new[e]``, or - where ``remove[e]`` - takes it out of the scene (the other K - 1 masks are
        re-normalised, the removed slot's mask is exactly 0).  The base is decoded once and every replacement decodes one slot-image, B K + E
        slot-image decodes where ``decode`` on the E edited scenes takes E K; a removal needs no decoder work at all.  A replace edit
        returns the bits ``decode`` returns for the edited ``z``.

        ``z`` (B, K, L) with 1 <= K <= 16, K taken from ``z`` as in ``decode``; ``image`` / ``slot``: int sequences or integer tensors of
        length E; ``z_new`` (E, L), row e for edit e (rows of removals are not read; None is allowed when every edit is a removal);
        ``remove``: E bools, default all False.  Returns a ``SceneEdit`` with ``pred (E, 3, S, S)`` and, on request, ``mask (E, K, 1, S, S)``,
        ``mean (E, 3, S, S)`` = the rgb of the slot-image put into the edited slot, ``base`` = ``decode(z)`` as (pred, mask, mean).

        NOT differentiable: the outputs are detached whatever ``z`` requires - gradients go through ``decode``.  One library call covers
        any E (it runs in chunks of ``max_batch()`` images' worth of slot-images without decoding the base again) and counts as a decode
        for the call order: a saved differentiable call is discarded, ``refinement_state()`` must be read before it."""
        L = self.dim_latent
        if not torch.is_tensor(z) or z.dim() != 3 or z.shape[2] != L or not 1 <= z.shape[1] <= 16 or z.shape[0] < 1:
            raise ValueError(f'IODINE.edit: z must have shape (B, K, {L}) with B >= 1 and 1 <= K <= 16 (the per-pixel kernels are '
                             f'instantiated for K <= 16); got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}')
        B, K = int(z.shape[0]), int(z.shape[1])
        image = self._int_list(image, 'image')
        E = len(image)
        if E < 1:
            raise ValueError('IODINE.edit: the edit list is empty (image has no entries)')
        slot = self._int_list(slot, 'slot', E)
        if remove is None:
            remove = [False] * E
        else:
            remove = [bool(r) for r in (remove.detach().cpu().tolist() if torch.is_tensor(remove) else list(remove))]
            if len(remove) != E:
                raise ValueError(f'IODINE.edit: remove has {len(remove)} entries, but there are {E} edits (one entry per edit)')
        for e in range(E):
            if not 0 <= image[e] < B:
                raise ValueError(f'IODINE.edit: edit {e}: image {image[e]} is outside 0..{B - 1} (z has shape {tuple(z.shape)})')
            if not 0 <= slot[e] < K:
                raise ValueError(f'IODINE.edit: edit {e}: slot {slot[e]} is outside 0..{K - 1} (z has shape {tuple(z.shape)})')
            if remove[e] and K == 1:
                raise ValueError(f'IODINE.edit: edit {e}: removes the only slot of image {image[e]} (z has K = 1: nothing would be left to render)')
        n_rep = E - sum(remove)
        if n_rep > 0 and (not torch.is_tensor(z_new) or tuple(z_new.shape) != (E, L)):
            raise ValueError(f'IODINE.edit: z_new must have shape ({E}, {L}), one row per edit (rows of removals are not read); got '
                             f'{tuple(z_new.shape) if torch.is_tensor(z_new) else type(z_new).__name__}')
        if n_rep > 0 and z_new.device != z.device:
            raise ValueError(f'IODINE.edit: z_new is on {z_new.device}, z on {z.device}')
        T = self._shape[1] if self._shape is not None else int(self._cfg.iters)      # plays no part, as in decode
        cap = self.max_batch(K=K, T=T)
        if B > cap:
            raise ValueError(f'IODINE.edit: z has {B} images, one call takes at most max_batch() = {cap} at K = {K}: edit the scenes in groups')
        dev = z.device
        z = z.detach().to(torch.float32).contiguous()
        zn = z_new.detach().to(torch.float32).contiguous() if n_rep > 0 else None
        W = min(cap, max(B, -(-n_rep // K)))
        h = self._sync_params(dev)
        if not hasattr(_lib.lib(), 'iodine_scene_edit'):
            raise RuntimeError('IODINE.edit: this build of libiodine_hip.so has no iodine_scene_edit')
        self._ensure_workspace(h, W, 0, dev, K, T)
        S = self.img_size
        f = dict(device=dev, dtype=torch.float32)
        pred = torch.empty((E, 3, S, S), **f)
        mask = torch.empty((E, K, 1, S, S), **f) if return_mask else None
        mean = torch.empty((E, 3, S, S), **f) if return_mean else None
        base = (torch.empty((B, 3, S, S), **f), torch.empty((B, K, 1, S, S), **f), torch.empty((B, K, 3, S, S), **f)) if return_base else (None,) * 3
        arr = lambda v: (C.c_int * E)(*v)
        self._call_serial += 1
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_scene_edit(
            h, self._stream(), B, _lib.ptr(z), E, arr(image), arr(slot), arr([int(r) for r in remove]), _lib.ptr(zn), W,
            _lib.ptr(pred), _lib.ptr(mask), _lib.ptr(mean), *[_lib.ptr(t) for t in base]), h, 'iodine_scene_edit'))
        return SceneEdit(pred, mask, mean, base if return_base else None)

    _PREDICTIVE_IMAGES = 256                    # images' worth of slot-images one chunk of ``predictive`` decodes at most (or one sample)

    @torch.no_grad()
    def predictive(self, x=None, samples=16, posterior=None, eps=None, weights=None):
        """Read-outs over ``samples`` draws z_s = mu + exp(logvar / 2) eps_s from ONE posterior: the per-pixel mean and variance of the
        rendered image and of every mask, how often each slot wins a pixel, and - with an image ``x (B, 3, S, S)`` - the per-image
        log-likelihood of every sample with the S-sample importance-weighted bound (IWAE), the Monte-Carlo ELBO and the closed-form-KL ELBO
        built from it.  Returns a ``Predictive``.  The S B K slot-images are decoded by the decoder's own kernels in chunks; one per-pixel
        kernel folds each chunk into the running moments, so no sample's planes are ever written, and every field is bit for bit
        independent of how the samples were cut into chunks (``batch_cap`` bounds the arena as it does for ``edit``).

        ``posterior``: ``(mean, logvar)`` of shape (B, K, L), 1 <= K <= 16 taken from it as in ``decode``; default
        ``model.posterior.mean / logvar`` - what the last ``reconstruct`` / ``encode`` / ``forward`` left (none: RuntimeError).  ``eps``:
        (S, B, K, L), or None for the library's generator, one draw per sample.  ``weights``: per-pixel observation weights of this call, as
        everywhere else; needs ``x``.  ``model.sigma`` is read as everywhere else, ``model.beta`` plays no part.  ``z[s]`` is what
        ``elbo(x, eps=eps[s])`` samples from that posterior, and each sample's image and masks are the bits ``decode(z[s])`` returns.

        NOT differentiable (gradients go through ``decode`` / ``elbo``).  A batch above ``max_batch()`` runs in groups of independent
        images.  The call counts as a decode for the call order: a saved differentiable call is discarded, ``refinement_state()`` still
        works after it; the logger and ``self.z / mean / mask`` are not touched."""
        import numbers
        L, Si = self.dim_latent, self.img_size
        if isinstance(samples, bool) or not isinstance(samples, numbers.Integral) or samples < 1:
            raise ValueError(f'IODINE.predictive: samples must be an integer >= 1; got {samples!r}')
        S = int(samples)
        if weights is not None and x is None:
            raise ValueError('IODINE.predictive: weights= weigh the likelihood of an image, but x is None')
        if posterior is None:
            posterior = (self.posterior.mean, self.posterior.logvar)
            if posterior[0] is None or posterior[1] is None:
                raise RuntimeError('IODINE.predictive: no posterior - pass posterior=(mean, logvar) or call reconstruct / encode / forward '
                                   'first (they leave model.posterior.mean / logvar)')
        if (not isinstance(posterior, (tuple, list)) or len(posterior) != 2 or any(not torch.is_tensor(t) for t in posterior)
                or posterior[0].dim() != 3 or posterior[0].shape != posterior[1].shape or posterior[0].shape[2] != L
                or not 1 <= posterior[0].shape[1] <= 16 or posterior[0].shape[0] < 1):
            got = tuple(tuple(t.shape) if torch.is_tensor(t) else type(t).__name__ for t in posterior) if isinstance(posterior, (tuple, list)) else type(posterior).__name__
            raise ValueError(f'IODINE.predictive: posterior must be (mean, logvar), both of shape (B, K, {L}) with B >= 1 and 1 <= K <= 16; got {got}')
        pm, plv = posterior
        B, K = int(pm.shape[0]), int(pm.shape[1])
        if eps is not None and (not torch.is_tensor(eps) or tuple(eps.shape) != (S, B, K, L)):
            raise RuntimeError(f'IODINE.predictive: eps must have shape {(S, B, K, L)} (samples, B, K, L); got '
                               f'{tuple(eps.shape) if torch.is_tensor(eps) else type(eps).__name__}')
        if x is not None:
            x = self._check_x(x)
            if x.shape[0] != B:
                raise ValueError(f'IODINE.predictive: x has {x.shape[0]} images, the posterior {B}')
            weights = self._check_weights(weights, x, 'predictive')
        T = self._shape[1] if self._shape is not None else int(self._cfg.iters)      # plays no part, as in decode
        sigma = self._read_objective(T)[0]
        dev = pm.device
        self._ensure_handle(dev)                            # (a CPU tensor is refused here, after the argument checks)
        if plv.device != dev or (x is not None and x.device != dev):
            raise ValueError('IODINE.predictive: the posterior and x must be on the same device')
        pm, plv = pm.detach().to(torch.float32).contiguous(), plv.detach().to(torch.float32).contiguous()
        cap = self.max_batch(K=K, T=T)
        if B > cap:                                         # groups of independent images; the noise is cut along its batch axis
            parts = [self.predictive(None if x is None else x[s:e], S, (pm[s:e], plv[s:e]), None if eps is None else eps[:, s:e],
                                     None if weights is None else weights[s:e]) for s, e in self._chunks(B, cap)]
            cat = lambda name, dim: None if getattr(parts[0], name) is None else torch.cat([getattr(q, name) for q in parts], dim)
            return Predictive(cat('z', 1), cat('pred_mean', 0), cat('pred_var', 0), cat('mask_mean', 0), cat('mask_var', 0), cat('votes', 0),
                              cat('segmentation', 0), cat('agreement', 0), S, cat('ll', 1), cat('log_w', 1), cat('iwae', 0), cat('elbo_mc', 0),
                              cat('elbo', 0))
        if not hasattr(_lib.lib(), 'iodine_predictive'):
            raise RuntimeError('IODINE.predictive: this build of libiodine_hip.so has no iodine_predictive')
        if eps is None:                                     # one draw id per sample
            eps = torch.empty((S, B, K, L), device=dev, dtype=torch.float32)
            for s in range(S):
                eps[s].copy_(self._normals(None, (B, K, L), dev))
        else:
            eps = eps.detach().to(device=dev, dtype=torch.float32).contiguous()
        W = min(cap, max(B, min(S * B, self._PREDICTIVE_IMAGES)))
        st = self._state                                    # the arena is re-planned for W images: an LSTM state still in it is fetched first
        if st is not None and st.h is None and st.serial is not None and st.serial == self._call_serial:
            self.refinement_state()
        h = self._sync_params(dev)
        self._ensure_workspace(h, W, 0, dev, K, T)
        self._ensure_objective(h, (sigma,) + tuple(self._objective[1:]), dev)     # sigma of this call; beta / iteration weights play no part
        f = dict(device=dev, dtype=torch.float32)
        z = torch.empty((S, B, K, L), **f)
        pmean, pm2 = torch.empty((B, 3, Si, Si), **f), torch.empty((B, 3, Si, Si), **f)
        mmean, mm2 = torch.empty((B, K, 1, Si, Si), **f), torch.empty((B, K, 1, Si, Si), **f)
        votes = torch.empty((B, K, Si, Si), device=dev, dtype=torch.int32)
        ll = torch.empty((S, B), **f) if x is not None else None
        self._call_serial += 1
        ws = self._send_weights(h, weights)                 # (ws: alive until the call is queued)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_predictive(
            h, self._stream(), B, S, _lib.ptr(pm), _lib.ptr(plv), _lib.ptr(eps), _lib.ptr(x), W, _lib.ptr(z), _lib.ptr(pmean), _lib.ptr(pm2),
            _lib.ptr(mmean), _lib.ptr(mm2), _lib.ptr(votes), _lib.ptr(ll)), h, 'iodine_predictive'))
        del ws
        # arg-max of the votes with the lowest index on a tie: the largest of votes * K + (K - 1 - k)
        key = votes.to(torch.int64) * K + torch.arange(K - 1, -1, -1, device=dev).view(1, K, 1, 1)
        top = key.max(1).values
        seg = (K - 1 - top % K).to(torch.uint8)
        agreement = (top // K).to(torch.float32) / S
        out = Predictive(z, pmean, pm2 / S, mmean, mm2 / S, votes, seg, agreement, S)
        if x is not None:
            out.ll = ll
            out.log_w, out.iwae, out.elbo_mc, out.elbo = sample_bounds(ll, z, eps, pm, plv)
        return out

    _STALE = ('IODINE: backward of a stale {0} - the library keeps the saved state of ONE differentiable call and another forward / '
              'reconstruct / decode / elbo call has re-used it since, or it was differentiated already (the reference would hold a second '
              'autograd graph; call backward() before the next model call)')

    def _decode_backward(self, serial, K, grads, want_z, want_p, flat):
        """iodine_decode_backward for the saved decode ``serial``: (dz or None, flat parameter gradients or None).  ``flat``: a buffer
        of earlier chunks to accumulate into."""
        if serial != self._call_serial:
            raise RuntimeError(self._STALE.format('decode'))
        h, dev = self._handle, self._handle_device
        B = next(g for g in grads if g is not None).shape[0]
        S, names = self.img_size, ('dg.pred', 'dg.mask', 'dg.mean')
        shapes = ((B, 3, S, S), (B, K, 1, S, S), (B, K, 3, S, S))
        gs = []
        for g, n, shp in zip(grads, names, shapes):
            if g is not None and tuple(g.shape) != shp:
                raise RuntimeError(f'IODINE.decode backward: gradient of shape {tuple(g.shape)}, expected {shp}')
            gs.append(None if g is None else self._stage(n, g.detach().to(device=dev, dtype=torch.float32).contiguous()))
        dz = self._out('dg.dz', (B, K, self.dim_latent), dev) if want_z else None
        acc = flat is not None
        if want_p and flat is None:
            flat = self._out('t.flat', (sum(p.numel() for p in self._ordered_params()),), dev)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_decode_backward(
            h, self._stream(), B, _lib.ptr(gs[0]), _lib.ptr(gs[1]), _lib.ptr(gs[2]), _lib.ptr(dz), _lib.ptr(flat) if want_p else None,
            1 if acc else 0), h, 'iodine_decode_backward'))
        self._call_serial += 1                      # the saved pass is consumed (no retain_graph)
        return self._own(dz), flat                  # (flat: the caller takes its copy - graph mode - after its last chunk)

    def elbo(self, x, eps=None, differentiable=None):
        """Single-pass ELBO (iodine.py:161-241), see ``_elbo_nograd`` for what it computes and leaves on ``self``.

        ``differentiable``: None (default) - the returned scalar carries an autograd graph iff grad mode is on and a caller-set
        ``model.posterior.mean`` / ``.logvar`` of this batch's shape requires grad; True - also without (gradients then go to the
        ``decoder.*`` parameters and, from the initial posterior, to ``posterior.init_mean / init_logvar``); False - never.
        ``elbo.backward()`` fills ``posterior.mean.grad / .logvar.grad`` and the parameter gradients as the reference's autograd does
        (iodine.py:90,137); the value is the same bits either way.  One differentiable call is kept: backward before the next call.
        With per-pixel observation weights: ``weighted_elbo``."""
        return self.weighted_elbo(x, None, eps, differentiable)

    def weighted_elbo(self, x, weights, eps=None, differentiable=None):
        """``elbo(x, eps, differentiable)`` under per-pixel observation weights (B, 1, S, S) / (B, S, S) of the log-likelihood (module
        docstring; None: no weights): value, ``elbo_terms`` and the gradients are those of the weighted ELBO.  ``elbo`` keeps the
        reference's signature, so the weights of a single-pass ELBO are an argument of this method."""
        pm, plv = self.posterior.mean, self.posterior.logvar
        shape = (x.shape[0], self.K, self.dim_latent) if x.dim() == 4 else None
        given = pm is not None and plv is not None and tuple(pm.shape) == shape and pm.device == x.device
        sg = self._sigma_input()
        in_grad = x.requires_grad or (torch.is_tensor(weights) and weights.requires_grad)
        if differentiable is None:
            differentiable = (given and (pm.requires_grad or plv.requires_grad)) or bool(sg) or in_grad
        if differentiable and torch.is_grad_enabled():
            xc = self._check_x(x)                           # (model.K / n_iters are checked by _elbo_call, before any device work)
            w = self._check_weights(weights, xc, 'weighted_elbo')
            xi, wi = self._grad_inputs(x, weights, xc, w)
            return _ElboGrad.apply(self, xi, eps, wi, pm if given else None, plv if given else None, *self._ordered_params(), *sg)
        return self._elbo_nograd(x, eps, weights)

    @torch.no_grad()
    def _elbo_nograd(self, x, eps=None, weights=None):
        """Single-pass ELBO (iodine.py:161-241): one sample from the current posterior (``self.posterior.mean / logvar`` as
        left by the last call for this batch size; otherwise the initial posterior of ``init_unit``, iodine.py:607-618),
        decode, mixture log-likelihood minus KL.  Sets ``self.z / mean / mask / mask_logits`` and the logger entries like the
        reference.  ``eps`` (B, K, L) replaces the ``torch.randn_like`` draw.  Returns the scalar ELBO (no autograd graph:
        the gradients the reference takes from it are what reconstruct / forward compute in closed form)."""
        K, T = self._run_shape()
        self._read_objective(T)
        x = self._check_x(x)
        weights = self._check_weights(weights, x, 'weighted_elbo')
        dev, B = x.device, x.shape[0]
        cap = self.max_batch()
        if B > cap:
            pm0, plv0 = self.posterior.mean, self.posterior.logvar
            whole = pm0 is not None and plv0 is not None and tuple(pm0.shape) == (B, self.K, self.dim_latent) and pm0.device == dev
            parts, sizes = [], []
            for s, e in self._chunks(B, cap):
                # the chunk's slice of the current posterior (or the initial posterior, as for a whole batch)
                self.posterior.mean, self.posterior.logvar = (pm0[s:e], plv0[s:e]) if whole else (None, None)
                self._elbo_nograd(x[s:e], None if eps is None else eps[s:e], None if weights is None else weights[s:e])
                parts.append(self._chunk_state()); sizes.append(e - s)
            self.posterior.mean, self.posterior.logvar = pm0, plv0
            self._merge_chunk_state(parts, sizes, x)
            return self.elbo_terms[0, 0]
        pm, plv = self.posterior.mean, self.posterior.logvar
        if pm is None or plv is None or tuple(pm.shape) != (B, K, self.dim_latent) or pm.device != dev:
            pm = plv = None
        return self._elbo_call(x, eps, pm, plv, save=False, weights=weights)

    def _elbo_call(self, x, eps, pm, plv, save, weights=None, sigma_grad=False, input_grad=0):
        """One iodine_elbo of at most ``max_batch`` images from the posterior (pm, plv) - None: the initial one; ``save``: kept for
        iodine_elbo_backward.  x as ``_check_x``, weights as ``_check_weights`` return them.  -> the ELBO; with ``sigma_grad`` (a saved call
        only) -> (ELBO, d LL / d sigma)."""
        K, T = self._run_shape()
        obj = self._read_objective(T)
        dev, B = x.device, x.shape[0]
        h = self._sync_params(dev)
        input_grad = input_grad if save else 0
        self._ensure_input_grad(h, input_grad)
        self._ensure_workspace(h, B, 2 if save else 0, dev, K, T)
        self._ensure_objective(h, obj, dev, save and sigma_grad)
        shape = (B, K, self.dim_latent)
        eps = self._normals(eps, shape, dev)
        if pm is not None:
            pm = self._stage('e.pm', pm.detach().to(torch.float32).contiguous())
            plv = self._stage('e.plv', plv.detach().to(torch.float32).contiguous())
        terms = self._out('e.terms', (3,), dev)
        xs = self._stage('x', x)
        self._call_serial += 1
        ws = self._send_weights(h, weights)
        if save:
            self._saving(h, True)
        try:
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_elbo(h, self._stream(), B, _lib.ptr(xs), _lib.ptr(pm), _lib.ptr(plv),
                                                                        _lib.ptr(eps), _lib.ptr(terms)), h, 'iodine_elbo'))
        finally:
            if save:
                self._saving(h, False)
        terms = self._own(terms)
        self.elbo_terms = terms.view(1, 3)
        sg = self._fetch_sigma_grad(h, dev, 1) if save and sigma_grad else None
        self._last_ig = self._fetch_input_grad(h, dev, x, weights, input_grad) if input_grad else None
        self._fetch_last_elbo(h, x, terms)
        elbo = terms[0].clone() if save else terms[0]
        return (elbo, sg) if sigma_grad else elbo

    def _elbo_backward(self, serial, BK, grad_out, want_post, want_p, flat=None):
        """iodine_elbo_backward for the saved elbo ``serial``: (d / d posterior.mean, d / d posterior.logvar, flat parameter gradients),
        each None when not asked for.  ``flat``: a buffer of earlier chunks to accumulate into."""
        if serial != self._call_serial:
            raise RuntimeError(self._STALE.format('elbo'))
        h, dev = self._handle, self._handle_device
        B, K = BK                                   # batch and slots of the saved call
        gl = self._stage('e.gl', grad_out.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous())
        gpm = self._out('e.gpm', (B, K, self.dim_latent), dev) if want_post else None
        gplv = self._out('e.gplv', (B, K, self.dim_latent), dev) if want_post else None
        acc = flat is not None
        if want_p and flat is None:
            flat = self._out('t.flat', (sum(p.numel() for p in self._ordered_params()),), dev)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_elbo_backward(
            h, self._stream(), _lib.ptr(gl), _lib.ptr(gpm), _lib.ptr(gplv), _lib.ptr(flat) if want_p else None, 1 if acc else 0),
            h, 'iodine_elbo_backward'))
        self._call_serial += 1                      # the saved pass is consumed (no retain_graph)
        return self._own(gpm), self._own(gplv), flat          # (flat: the caller takes its copy - graph mode - after its last chunk)

    def _elbo_chunked_grad(self, x, eps, pm, plv, want_post, want_p, weights=None, sigma_grad=False, input_grad=0):
        """Differentiable elbo of a batch above ``max_batch`` (see _ElboGrad): forward + backward of every chunk with its share of the
        batch mean.  Returns the ELBO, (d / d posterior.mean, d / d posterior.logvar, flat parameter gradients) for grad_output 1 and, with
        ``sigma_grad``, d LL / d sigma of the batch (else None)."""
        dev, B = x.device, x.shape[0]
        parts, sizes, gpms, gplvs, flat, sig, igs = [], [], [], [], None, None, []
        pm0, plv0 = self.posterior.mean, self.posterior.logvar
        for s, e in self._chunks(B, self.max_batch()):
            r = self._elbo_call(x[s:e].contiguous(), None if eps is None else eps[s:e], None if pm is None else pm[s:e],
                                None if plv is None else plv[s:e], save=True, weights=None if weights is None else weights[s:e].contiguous(),
                                sigma_grad=sigma_grad, input_grad=input_grad)
            sc = r[1] if sigma_grad else None
            parts.append(self._chunk_state()); sizes.append(e - s)
            w = torch.full((), (e - s) / float(B), device=dev, dtype=torch.float32)
            if input_grad:                                  # this chunk's share of the batch mean
                igs.append(tuple(None if t is None else t * w for t in self._last_ig))
            if sc is not None:                              # this chunk's share of the batch mean
                sig = sc * w if sig is None else sig + sc * w
            gpm, gplv, flat = self._elbo_backward(self._call_serial, (e - s, self.K), w, want_post, want_p, flat)
            if not want_p:
                flat = None
            gpms.append(gpm); gplvs.append(gplv)
        self.posterior.mean, self.posterior.logvar = pm0, plv0
        self._merge_chunk_state(parts, sizes, x)
        self._last_ig = tuple(None if igs[0][j] is None else torch.cat([g[j] for g in igs], 0) for j in range(2)) if input_grad else None
        pre = (torch.cat(gpms, 0) if want_post else None, torch.cat(gplvs, 0) if want_post else None,
               self._own(flat) if flat is not None else None)
        return self.elbo_terms[0, 0].clone(), pre, sig

    # ---- training: iodine.py:115-158 + lib/engine/train.py:60-63 -------------------------------------
    def _check_attach_frames(self, attach_frames, T):
        """``attach_frames`` of ``forward`` -> None (off) or the sorted tuple of evaluation indices.  Host only."""
        if attach_frames is None or attach_frames is False:
            return None
        if attach_frames is True:
            return tuple(range(T + 1))
        try:
            vals = list(attach_frames)
        except TypeError:
            raise ValueError(f'IODINE.forward: attach_frames must be None, a bool or an iterable of evaluation indices in 0..{T}; got '
                             f'{attach_frames!r}') from None
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= T:
                raise ValueError(f'IODINE.forward: attach_frames holds {v!r}; a forward of {T} iterations makes the ELBO evaluations 0..{T}')
        if len(set(vals)) != len(vals):
            raise ValueError(f'IODINE.forward: attach_frames names an evaluation twice: {vals!r}')
        return tuple(sorted(vals))

    def forward(self, x, eps=None, state=None, attach_state=False, keep_state=False, weights=None, attach_frames=None):
        """-sum_i w_i ELBO_i (w = ``model.iter_weights``, by default (i+1)/(T+1); ELBO_i = LL_i - ``model.beta`` KL_i at ``model.sigma``),
        differentiable wrt every parameter.  ``loss.backward()`` differentiates the forward as it
        ran, at the (K, T) it read - like the reference, whose autograd graph is fixed at forward time.  ``x``: images
        (B, 3, S, S) or a clip (B, T+1, 3, S, S), ELBO_i then against frame i (frame i of a clip that requires grad gets the gradient of evaluation i).

        ``state``: a tuple (post_mean, post_logvar, h, c) as ``refinement_state()`` returns it (h / c also as the reference's (B * K,
        MLP_UNITS) of ``lstm_hidden``): evaluation 0 samples from the given lambda and the LSTM starts from (h, c) instead of the initial
        posterior and zeros; the call still makes T + 1 evaluations.  T = 4 equals T = 2 followed by T = 2 from the state, evaluation by
        evaluation and bit for bit, given the matching slices of ``x`` and ``eps``; the boundary frame is evaluated by both calls, so the
        continuing call usually runs with ``iter_weights[0] = 0`` (``iodine_amd.engine.clip_backward`` does all of this).  Detached
        tensors give truncated back-propagation through time.  Tensors that require grad (under grad mode) receive their gradient from
        ``backward()``: d / d (h, c) through all T iterations, d / d lambda through evaluation 0 alone (lambda_1 = detach(lambda_0) +
        delta_0, iodine.py:642-643).  ``posterior.init_mean / init_logvar`` are not part of such a forward and get ``None`` from autograd.

        ``keep_state=True``: ``model.refinement_state()`` after the call returns detached clones of (lambda_T, h_T, c_T) - the ``state``
        of the next chunk (two small copies, made only then).  Without it a training forward leaves no state to fetch, as before.

        ``attach_state=True`` (with grad mode on; under ``torch.no_grad()`` it changes nothing): ``model.z``, ``model.mean``,
        ``model.mask``, ``model.mask_logits``, ``model.posterior.mean``, ``model.posterior.logvar`` - the state of the final ELBO
        evaluation (of a clip: frame T) - and ``model.lstm_hidden`` = (h, c) after the last update, shaped (B * K, MLP_UNITS), carry the
        autograd graph like in the reference (iodine.py:37,137,144,171-187,642-651), so auxiliary
        terms on them (a supervised mask loss, a probe on ``z``, a slot regulariser, the cotangents of a following chunk) train the decoder
        and, back through all T iterations, the refinement network: ``(loss + aux).backward()``.  The values are the same bits as without
        it; the logger entries stay detached.  The library keeps ONE saved forward and its backward consumes it: sum the terms first and
        call ``backward()`` once - a second one (``aux.backward()`` followed by ``loss.backward()``) raises the stale-forward error.

        ``attach_frames``: per-frame auxiliary losses.  ``True`` attaches all T + 1 ELBO evaluations, an iterable of ints in 0..T the
        chosen ones (sorted; a repeated or out-of-range index raises ``ValueError`` before any device work), ``None`` / ``False`` none.
        ``model.frames`` is then a dict: ``index`` (the attached evaluations) and ``z``, ``post_mean``, ``post_logvar`` (F, B, K, L),
        ``mean`` (F, B, K, 3, S, S), ``mask``, ``mask_logits`` (F, B, K, 1, S, S) - entry j is what evaluation ``index[j]`` decoded and
        the lambda it sampled from, attached to the graph like in the reference, whose every ``elbo()`` call of ``forward`` leaves them so
        (iodine.py:171-187): a mask loss per frame, a consistency term between z_i and z_{i+1}, a probe on a frame's posterior, all in
        one ``(loss + aux).backward()``.  Each attached evaluation with a term on mean / mask / mask_logits costs one decoder forward
        and backward in that ``backward()``; evaluation T costs what ``attach_state`` costs.  Under ``torch.no_grad()`` the same values
        come detached (a training-time trajectory).  Any ``forward`` without it sets ``model.frames = None``.

        A batch above ``max_batch(training=True)`` runs in chunks, each chunk's backward inside the forward: a detached ``state`` is sliced
        per chunk and ``keep_state`` gathers the chunks' states; ``attach_state``, ``attach_frames`` and a ``state`` that requires grad are
        refused there.

        ``weights``: per-pixel observation weights >= 0 of this call, (B, 1, S, S) / (B, S, S), with a clip also (B, T+1, 1, S, S) /
        (B, T+1, S, S): the loss and every gradient are those of the weighted ELBO (module docstring).  A floating-point weight tensor that
        requires grad receives d loss / d w, and an ``x`` that requires grad d loss / d x (module docstring); otherwise both are data."""
        K, T = self._run_shape()
        self._read_objective(T)                      # (refusals before any device work; _train_forward hands it to the handle)
        x_given, w_given = x, weights
        x, _ = self._check_frames(x, T + 1, 'forward' if state is None else 'forward from a state')
        weights = self._check_weights(weights, x, 'forward')
        xi, wi = self._grad_inputs(x_given, w_given, x, weights)   # (the nodes' inputs 1 and 3: the caller's tensors where they require grad)
        B = x.shape[0]
        state = self._check_train_state(state, B, K, x.device)
        index = self._check_attach_frames(attach_frames, T)
        self._state = None                          # the state of an earlier encode / reconstruct ends here (refinement_state)
        self.frames = None
        attach = bool(attach_state) and torch.is_grad_enabled()
        sg = self._sigma_input()
        state_grad = state is not None and torch.is_grad_enabled() and any(t.requires_grad for t in state)
        if B > self.max_batch(training=True):
            for on, what in ((attach, 'attach_state=True'), (state_grad, 'a state that requires grad'),
                             (index is not None, 'attach_frames')):
                if on:
                    raise RuntimeError(f'IODINE.forward({what}): a batch of {B} images exceeds max_batch(training=True) = '
                                       f'{self.max_batch(training=True)}; such a batch runs in chunks, each chunk\'s backward inside the forward, '
                                       'which leaves nothing for cotangents that arrive later to back-propagate through - use a smaller '
                                       'batch per call')
            if state is not None:
                state = tuple(t.detach() for t in state)
            loss, elbo_iter = _ChunkedTrainStep.apply(self, xi, eps, wi, state, bool(keep_state), *self._ordered_params(), *sg)
            self.elbo_terms = elbo_iter
            return loss
        eps = self._eps(eps, B, x.device)
        out = _TrainStep.apply(self, xi, eps, wi, attach, index, *(state or (None,) * 4), *self._ordered_params(), *sg)
        loss, self.elbo_terms = out[:2]
        if attach:
            self.z, self.mean, self.mask, self.mask_logits, self.posterior.mean, self.posterior.logvar, lh, lc = out[2:10]
            self.lstm_hidden = (lh, lc)
        if index is not None:
            self.frames = dict(index=index, **dict(zip(_FRAME_KEYS, out[-6:])))
        hc = self._train_tail(x, self.elbo_terms, attach, keep_state)
        if keep_state:
            self._state = _RefineState(self.posterior.mean.detach(), self.posterior.logvar.detach(), *hc)
        return loss

    @torch.no_grad()
    def _train_tail(self, x, terms, attach=False, keep_state=False, scalars=True):
        """What a training forward leaves behind its library call: the state and logger entries of its final elbo() (iodine.py:226-239; a
        clip: its last frame) and lambda_T unless the node attached them (``attach``), the logger scalars of iodine.py:156-157
        (``scalars``) and, returned with ``keep_state``, the LSTM state (h, c) (B, K, MLP_UNITS)."""
        h, dev, B = self._handle, x.device, x.shape[0]
        hc = None
        if not attach:
            self._fetch_last_elbo(h, x, terms[-1])
            self._fetch_posterior(h, B, dev)
        if keep_state:
            hc = tuple(t.detach().view(B, self.K, -1) for t in self.lstm_hidden) if attach else self._fetch_train_state(B, dev)
        if scalars:
            stats = torch.empty((2,), device=dev, dtype=torch.float32)
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_logger_scalars(h, self._stream(), _lib.ptr(stats)), h))
            logger.update(init_mean=stats[0], init_logvar=stats[1])
        return hc

    def _fetch_train_state(self, B, dev):
        """(h, c) (B, K, MLP_UNITS) after the last update of the training forward that just ran (iodine_last_train_state)."""
        hh = torch.empty((B, self.K, int(self._cfg.ref_mlp_units)), device=dev, dtype=torch.float32)
        cc = torch.empty_like(hh)
        h = self._handle
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_last_train_state(h, self._stream(), B, _lib.ptr(hh), _lib.ptr(cc)),
                                             h, 'iodine_last_train_state'))
        return hh, cc

    def _train_forward(self, x, eps, state=None, weights=None, frames=None, sigma_grad=False, input_grad=0):
        """iodine_train_forward_frames -> (loss, ELBO terms, frames, S).  ``state``: None or the initial (post_mean, post_logvar, h, c);
        ``frames``: None -> (), or a tuple of evaluation indices, possibly empty -> the six (F, B, K, ...) tensors of those evaluations in
        the order of ``_FRAME_KEYS``; S: with ``sigma_grad`` the device scalar sum_e w_e dLL_e/dsigma (the forward then runs with option
        sigma_grad), else None.  NULL / 0 for what is not asked for: the library then runs the plain forward, launch for launch."""
        dev, B = x.device, x.shape[0]
        K, T = self._run_shape()
        obj = self._read_objective(T)
        h = self._sync_params(dev)
        self._ensure_input_grad(h, input_grad)
        self._ensure_workspace(h, B, 1, dev, K, T, x.shape[1] if x.dim() == 5 else 0)
        self._ensure_objective(h, obj, dev, sigma_grad)
        loss = self._out('t.loss', (), dev)
        elbo_iter = self._out('t.elbo', (T + 1, 3), dev)
        xs, eps = self._stage('x', x), self._stage('eps', eps)
        self._call_serial += 1
        ws = self._send_weights(h, weights)                 # (ws: alive until the call is queued)
        outs, sptrs, optrs, idx, F = (), None, None, None, len(frames or ())
        if frames is not None:
            L, S = self.dim_latent, self.img_size
            shapes = ((F, B, K, L), (F, B, K, 3, S, S), (F, B, K, 1, S, S), (F, B, K, 1, S, S), (F, B, K, L), (F, B, K, L))
            outs = [self._out('tf.' + n, shp, dev) for n, shp in zip(_FRAME_KEYS, shapes)]
        if F:
            optrs, idx = (C.c_void_p * 6)(*[t.data_ptr() for t in outs]), (C.c_int * F)(*frames)
        if state is not None:
            # (graph mode: the state goes through persistent staging buffers like reconstruct's, so the graph key repeats)
            st = [self._stage('ts.' + n, t.detach()) for n, t in zip(('pm', 'plv', 'h', 'c'), state)]
            sptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in st])
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_train_forward_frames(
            h, self._stream(), B, _lib.ptr(xs), _lib.ptr(eps), sptrs, _lib.ptr(loss), _lib.ptr(elbo_iter), idx, F, optrs),
            h, 'iodine_train_forward_frames'))
        out = (self._own(loss), self._own(elbo_iter), tuple(self._own(t) for t in outs))
        # (what is read back once after the call, in stream order)
        self._last_ig = self._fetch_input_grad(h, dev, x, weights, input_grad) if input_grad else None
        return (*out, self._fetch_sigma_grad(h, dev, T + 1, obj[2]) if sigma_grad else None)

    def _train_chunked(self, x, eps, state=None, keep_state=False, weights=None, sigma_grad=False, input_grad=0):
        """Forward + backward of every chunk (see _ChunkedTrainStep): returns the batch loss, the (T+1, 3) ELBO terms of the whole
        batch, d loss / d parameters as one flat buffer in named_parameters() order and, with ``sigma_grad``, sum_e w_e dLL_e/dsigma of
        the batch (else None).  ``state``: a detached initial state, cut along the batch; ``keep_state``: every chunk's LSTM state is
        copied out for ``refinement_state``."""
        dev, B = x.device, x.shape[0]
        flat = self._out('t.flat', (sum(p.numel() for p in self._ordered_params()),), dev)
        loss, terms, parts, sizes, pms, plvs, hcs, sig, igs = None, None, [], [], [], [], [], None, []
        for c, (s, e) in enumerate(self._chunks(B, self.max_batch(training=True))):
            xc = x[s:e].contiguous()
            ec = self._eps(None if eps is None else eps[:, s:e], e - s, dev)
            lc, tc, _, sc = self._train_forward(xc, ec, None if state is None else tuple(t[s:e].contiguous() for t in state),
                                                None if weights is None else weights[s:e].contiguous(), sigma_grad=sigma_grad,
                                                input_grad=input_grad)
            h = self._handle
            w = torch.full((), (e - s) / float(B), device=dev, dtype=torch.float32)
            if input_grad:                              # this chunk's share of the batch mean
                igs.append(tuple(None if t is None else t * w for t in self._last_ig))
            ws = self._stage('t.gl', w)
            if sc is not None:                          # this chunk's share of the batch mean
                sig = sc * w if sig is None else sig + sc * w
            self._launch(dev, lambda: _lib.check(_lib.lib().iodine_train_backward_flat(h, self._stream(), _lib.ptr(ws), _lib.ptr(flat),
                                                                                       1 if c else 0), h, 'iodine_train_backward'))
            hc = self._train_tail(xc, tc, keep_state=keep_state, scalars=c == 0)
            pms.append(self.posterior.mean); plvs.append(self.posterior.logvar)
            if keep_state:
                hcs.append(hc)
            self.elbo_terms = tc
            parts.append(self._chunk_state()); sizes.append(e - s)
            self._call_serial += 1                  # this chunk's saved forward is consumed
            loss = lc * w if loss is None else loss + lc * w
        with torch.no_grad():
            self._merge_chunk_state(parts, sizes, x)
            self.posterior.mean, self.posterior.logvar = torch.cat(pms, 0), torch.cat(plvs, 0)
            if keep_state:
                self._state = _RefineState(self.posterior.mean, self.posterior.logvar, torch.cat([hc[0] for hc in hcs], 0),
                                           torch.cat([hc[1] for hc in hcs], 0))
        self._last_ig = tuple(None if igs[0][j] is None else torch.cat([g[j] for g in igs], 0) for j in range(2)) if input_grad else None
        return loss, self.elbo_terms, self._own(flat), sig

    def _train_backward(self, grad_loss, serial, cot, want, BK, index, gf):
        """iodine_train_backward_frames for the saved forward ``serial`` -> (d loss / d parameters as one flat buffer, the four state
        gradients or None each).  ``cot``: the cotangents (mean, mask, mask_logits, z, posterior.mean, posterior.logvar) on the final
        elbo() of an attached forward and (h, c) (B * K, H) on the LSTM state after the last update; ``gf``: the six cotangents
        (F, B, K, ...) on the evaluations ``index`` in the order of ``_FRAME_KEYS``; each a tensor or None, ``grad_loss`` too.  ``want``:
        which of d / d (post_mean, post_logvar, h, c) of the initial state to return.  NULL / 0 for what is not asked for: the library
        then runs the narrower backward - without any of it the plain one -, launch for launch."""
        if serial != self._call_serial:
            raise RuntimeError(self._STALE.format('forward'))
        h, dev = self._handle, self._handle_device
        flat = self._out('t.flat', (sum(p.numel() for p in self._ordered_params()),), dev)
        # (graph mode: the cotangents go through persistent staging buffers like every other tensor, so the graph key repeats)
        stage = lambda names, gs: [None if g is None else self._stage(n, g.detach().to(device=dev, dtype=torch.float32).contiguous())
                                   for n, g in zip(names, gs)]
        addr = lambda ts: [None if t is None else t.data_ptr() for t in ts]
        cs = stage(('t.gl', 'a.mean', 'a.mask', 'a.logits', 'a.z', 'a.pm', 'a.plv', 'a.h', 'a.c'), (grad_loss, *cot))
        fs = stage(['f.' + n for n in _FRAME_KEYS], gf)
        outs, gptrs, fptrs, idx, F = (None,) * 4, None, None, None, 0
        if any(want):
            (B, K), L, H = BK, self.dim_latent, int(self._cfg.ref_mlp_units)
            outs = [self._out('ts.g' + n, shp, dev) if w else None
                    for n, shp, w in zip(('pm', 'plv', 'h', 'c'), ((B, K, L), (B, K, L), (B, K, H), (B, K, H)), want)]
            gptrs = (C.c_void_p * 4)(*addr(outs))
        if any(t is not None for t in fs):
            F = len(index)
            fptrs, idx = (C.c_void_p * 6)(*addr(fs)), (C.c_int * F)(*index)
        self._launch(dev, lambda: _lib.check(_lib.lib().iodine_train_backward_frames(
            h, self._stream(), *[_lib.ptr(c) for c in cs], _lib.ptr(flat), 0, gptrs, idx, F, fptrs), h, 'iodine_train_backward_frames'))
        self._call_serial += 1                      # the saved forward is consumed (no retain_graph)
        # (graph mode: autograd may keep what we return as .grad; never the staging buffer)
        return self._own(flat), tuple(self._own(t) for t in outs)


def arch_namespace(dim_latent, iters, slots, img_size, ref, dec, sigma=0.10, layernorm=True,
                   encoding=_lib.ENC_ORDER, kernels=(3, 3), ref_stride=2):
    """Build an ``ARCH``-shaped namespace (the yacs node of lib/config/defaults.py:35-100) from plain
    values; ref = (CONV_CHAN, CONV_LAYERS, MLP_UNITS), dec = (CONV_CHAN, CONV_LAYERS), kernels = (REF, DEC) KERNEL_SIZE."""
    from types import SimpleNamespace as NS
    return NS(DIM_LATENT=dim_latent, ITERS=iters, SLOTS=slots, ENCODING=list(encoding), IMG_CHANNELS=3,
              IMG_SIZE=img_size, SIGMA=sigma, LAYERNORM=layernorm, STOP_GRADIENT=False,
              REF=NS(CONV_CHAN=ref[0], CONV_LAYERS=ref[1], MLP_UNITS=ref[2], KERNEL_SIZE=kernels[0], STRIDE=ref_stride),
              DEC=NS(CONV_CHAN=dec[0], CONV_LAYERS=dec[1], KERNEL_SIZE=kernels[1]))


def clevr6_arch(slots=7, iters=5):
    """configs/clevr6_prop.yaml:26-45."""
    return arch_namespace(64, iters, slots, 128, (64, 4, 256), (64, 4))


def dsprites_arch(slots=6, iters=5):
    """configs/dsprites_noclip.yaml:26-45."""
    return arch_namespace(16, iters, slots, 64, (32, 3, 128), (32, 5))
