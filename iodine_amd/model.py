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
follows before the call (``Session.prepare``); ``loss.backward()`` differentiates the forward at the shape it ran with.

The objective is read the same way: ``model.sigma`` (the reference reads ``self.sigma`` on every ``elbo()`` call, iodine.py:210),
``model.beta`` - the weight of the KL term, as if iodine.py:223 read ``elbo = log_likelihood - self.beta * kl`` - and
``model.iter_weights`` - the per-iteration loss weights of iodine.py:152-153: None / 'linspace' = (i+1)/(T+1), 'uniform', 'last' or a
sequence of T + 1 numbers.  They are checked on the host when a call starts and reach the handle before the call (``Session.prepare``);
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

Form of the likelihood: ``model.likelihood = 'per_channel'`` (default) is the reference's objective, a K-component mixture for each colour
channel, ``LL_p = sum_c log sum_k (m_k + 1e-12) N(x_c; mu_kc, sigma)``; ``'joint'`` is the IODINE paper's, one mixture per pixel over the
RGB vector, ``LL_p = log sum_k (m_k + 1e-12) prod_c N(x_c; mu_kc, sigma)`` (library option ``joint_likelihood``).  The attribute is read
when a call starts, like ``sigma``, and everything that reports or differentiates a likelihood follows it: ``forward``, ``encode``,
``reconstruct``, ``elbo``, ``weighted_elbo``, ``predictive``, ``elbo_terms``, the gradients into ``x``, ``weights=`` and a learnable
``sigma``.  In joint mode ``model.log_likelihood`` is (B, 1, S, S) and ``dLL/dx`` / ``dLL/dw`` hold one responsibility ``r_k`` per slot in
place of ``r_kc``; ``K_log_likelihood`` and the mask_posterior / leave-one-out channels of the refinement input (already joint over RGB in
the reference) are the same.  A ``backward()`` of a pass that ran in the other form is refused by the library.  The mode is not part of
``state_dict``.

Multi-sample evaluation: ``model.predictive(x, samples=S)`` draws S latents from one posterior (default: the one the last ``reconstruct`` /
``encode`` / ``forward`` left) and returns a ``Predictive`` - per-pixel mean and variance of the rendered image and of the masks, per-slot vote
counts with their arg-max and agreement, and with an image the per-sample log-likelihoods, the importance-weighted bound, the Monte-Carlo ELBO and
the closed-form-KL ELBO per image (``iodine_predictive``: the samples share one decoder pass per chunk and one per-pixel kernel keeps the running
moments; nothing per sample is written).  Not in the reference, which scores and renders one draw (iodine.py:103, 171).

Adaptive refinement: ``model.reconstruct_adaptive(x, tol=..., rtol=..., max_iters=..., budget=...)`` refines every image until its own ELBO
estimate stops improving, drops it from the batch between rounds of ``check_every`` iterations and returns an ``adaptive.Adaptive`` with the
per-image iteration counts - image b is bit for bit what ``reconstruct`` gives at ``n_iters = iters[b]``, at the cost of ``sum(iters)``
image-iterations (``iodine_reconstruct_adaptive``; the rule is defined by tests/adaptive_reference.py).  Not in the reference, which runs
``ARCH.ITERS`` iterations for every image (iodine.py:85).

Extensions over the reference: every entry point takes an optional ``eps`` tensor of shape
(T+1, B, K, L) replacing the ``torch.randn_like`` draws of ``Gaussian.sample``
(iodine.py:632) in call order, so that results can be compared with the CPU oracle.  Without
``eps`` the draws come from the library's own counter-based generator (Philox4x32-10,
``iodine_randn``; seed with ``model.manual_seed``) - no ATen COMPUTE kernel runs on the product path (what a kernel trace
still shows from ATen are autograd's own fills: ``loss.backward()`` seeds the scalar loss gradient with ``ones_like`` and
``zero_grad`` / the flat gradient buffer are fills - a handful of 5-us launches per training step, none of them arithmetic of the model).
"""
from __future__ import annotations

import dataclasses
import math
import numbers
from typing import Optional

import torch
from torch import nn

from . import _args, _lib
from ._autograd import _FRAME_KEYS, _ChunkedTrainStep, _DecodeGrad, _ElboGrad, _TrainStep
from ._chunked import CAT0, CAT1, FIRST, SHARE, SUM, cut, merge, scaled, split
from ._session import Session


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
    # how groups of independent images are put together (_chunked.merge): the batch is axis 1 behind the sample axis, else axis 0
    MERGE = dict(z=CAT1, pred_mean=CAT0, pred_var=CAT0, mask_mean=CAT0, mask_var=CAT0, votes=CAT0, segmentation=CAT0, agreement=CAT0,
                 samples=FIRST, ll=CAT1, log_w=CAT1, iwae=CAT0, elbo_mc=CAT0, elbo=CAT0)


@dataclasses.dataclass
class Restarts:
    """What ``IODINE.restarts`` returns: C refinement chains of the same B images, the best one per image, and how far the chains agree.
    ``pred (B, 3, S, S)``, ``mask (B, K, 1, S, S)``, ``mean (B, K, 3, S, S)``, ``z``, ``post_mean``, ``post_logvar (B, K, L)`` - those of chain
    ``best[b]``, rows ``best[b] B + b`` of the one ``reconstruct`` over the batch repeated chain-major; ``best (B)`` int64; ``ll (C, B)``
    float32 - the (weighted) log-likelihood of each chain's returned decode -, ``kl (C, B)`` float64 - KL(lambda_T || N(0, 1)) -, ``score (C,
    B)`` float64 = ll - beta kl; ``segmentation (C, B, S, S)`` uint8 - every chain's arg-max map.  With ``consensus=True`` also ``perm (C, B,
    K)`` int32 - slot i of chain c is slot ``perm[c, b, i]`` of the best chain's labelling (the identity for the best chain itself) -,
    ``overlap (C, B, K, K)`` int32 - the contingency table of every chain's map against the best chain's -, ``votes (B, K, S, S)`` int32,
    ``consensus (B, S, S)`` uint8, ``agreement (B, S, S)``, ``mask_mean (B, K, 1, S, S)``, ``match (C, B)`` - the share of pixels on which a
    chain, relabelled, agrees with the best - and ``stability (B)`` - the mean of ``match`` over the chains other than the best, 1 for one
    chain; else None.  ``decodes``: with ``keep_decodes=True`` the ``(pred (C, B, 3, S, S), mask (C, B, K, 1, S, S), mean (C, B, K, 3, S, S))``
    of every chain (views of the one call's outputs, for ``figures.restarts_sheet``), else None.  Detached tensors."""
    pred: torch.Tensor
    mask: torch.Tensor
    mean: torch.Tensor
    z: torch.Tensor
    post_mean: torch.Tensor
    post_logvar: torch.Tensor
    best: torch.Tensor
    score: torch.Tensor
    ll: torch.Tensor
    kl: torch.Tensor
    segmentation: torch.Tensor
    chains: int
    perm: Optional[torch.Tensor] = None
    overlap: Optional[torch.Tensor] = None
    votes: Optional[torch.Tensor] = None
    consensus: Optional[torch.Tensor] = None
    agreement: Optional[torch.Tensor] = None
    mask_mean: Optional[torch.Tensor] = None
    match: Optional[torch.Tensor] = None
    stability: Optional[torch.Tensor] = None
    decodes: Optional[tuple] = None

    def ari(self):
        """``(C, B)`` float64 on the host: the adjusted Rand index of every chain's map against the best chain's, from ``overlap`` through
        ``ari.compute_ari`` (1 for the best chain itself).  One copy to the host, made when called."""
        if self.overlap is None:
            raise RuntimeError('Restarts.ari: the overlap tables are part of the consensus step - call restarts(..., consensus=True)')
        from .ari import compute_ari
        t = self.overlap.cpu().numpy()
        return torch.tensor([[compute_ari(t[c, b]) for b in range(t.shape[1])] for c in range(t.shape[0])], dtype=torch.float64)


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
        self.likelihood = getattr(ARCH, 'LIKELIHOOD', 'per_channel')    # 'per_channel' (the reference: a K-component mixture for each colour
                                        # channel) or 'joint' (the paper: one mixture per pixel over the RGB vector, option joint_likelihood);
                                        # read when a call starts, by everything that reports or differentiates a likelihood
        self.use_layernorm = ARCH.LAYERNORM
        self.use_stop_gradient = getattr(ARCH, 'STOP_GRADIENT', False)

        input_size, lambda_size = self.get_input_size()
        ref, dec = ARCH.REF, ARCH.DEC
        self.refine = _Refine(input_size, ref.CONV_CHAN, ref.MLP_UNITS, ARCH.DIM_LATENT, ref.CONV_LAYERS,
                              ref.KERNEL_SIZE, getattr(ref, 'STRIDE', 2))
        self.decoder = _Decoder(ARCH.DIM_LATENT, dec.CONV_CHAN, dec.CONV_LAYERS, dec.KERNEL_SIZE)
        self.posterior = _Posterior(self.dim_latent)

        self._cfg = _lib.Config(
            dim_latent=ARCH.DIM_LATENT, iters=ARCH.ITERS, slots=ARCH.SLOTS, img_size=ARCH.IMG_SIZE,
            img_channels=ARCH.IMG_CHANNELS, sigma=float(ARCH.SIGMA), layernorm=int(bool(ARCH.LAYERNORM)),
            stop_gradient=int(bool(self.use_stop_gradient)), encoding=_lib.encoding_bits(self.encodings),
            ref_conv_chan=ref.CONV_CHAN, ref_conv_layers=ref.CONV_LAYERS, ref_mlp_units=ref.MLP_UNITS,
            ref_kernel_size=ref.KERNEL_SIZE, ref_stride=getattr(ref, 'STRIDE', 2),
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
        self.log_likelihood = None      # (B, 3, S, S)    logsumexp_k(log(mask + 1e-12) + K_log_likelihood) of the last ELBO evaluation;
                                        # likelihood 'joint': (B, 1, S, S), logsumexp_k(log(mask + 1e-12) + K_log_likelihood.sum(2))
        self.K_log_likelihood = None    # (B, K, 3, S, S) gaussian_log_likelihood(x[:, None], mean, sigma); both float32, detached, raw

        self._session = Session(self._cfg, self.named_parameters)      # the library handle and all that mirrors it (_session.py)
        self._last_ig = None            # (d / d x, d / d w) the last differentiable call accumulated, for its autograd node
        self._state = None              # _RefineState of the last encode / reconstruct: see refinement_state
        self._seed, self._draws = 0, 0  # Philox key (manual_seed) and stream id - one per eps draw - of the library's normal generator

    LIKELIHOODS = ('per_channel', 'joint')

    @property
    def likelihood(self):
        return self._likelihood

    @likelihood.setter
    def likelihood(self, value):
        if value not in self.LIKELIHOODS:
            raise ValueError(f"IODINE.likelihood must be 'per_channel' or 'joint', got {value!r}")
        self._likelihood = value

    def _joint(self):
        return self._likelihood == 'joint'

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
    def _ordered_params(self):
        return [p for _, p in self.named_parameters()]

    # the session's fields and methods under the names the module had for them: callers that reach in (tests, tools) keep working
    _handle, _workspace, _ws_key, _call_serial, _objective = (property(lambda self, n=n: getattr(self._session, n), lambda self, v, n=n: setattr(
        self._session, n, v)) for n in ('handle', 'workspace', 'ws_key', 'call_serial', 'objective'))
    _stream = lambda self: self._session.stream()
    _sync_params = lambda self, device: self._bind(device).sync_params()

    def _bind(self, device: torch.device) -> Session:
        """The session with its handle on ``device``; a module that moved gets a new session there."""
        if device.type != 'cuda':
            raise RuntimeError('iodine_amd.IODINE runs only on a ROCm device (gfx950); got tensors on '
                               f'{device}. There is no CPU fallback - move the module and inputs with .to("cuda").')
        if self._session.device not in (None, device):     # the module moved: a new session, with the options and the call count
            self._session.close()
            self._session = Session(self._cfg, self.named_parameters, self._session.options, self._session.call_serial)
        self._session.open(device)
        return self._session

    def manual_seed(self, seed: int):
        """Seed of the library's generator for the ``eps=None`` draws (Philox4x32-10; give every rank its own seed)."""
        self._seed, self._draws = int(seed) & (2 ** 64 - 1), 0
        return self

    def mark_params_dirty(self):
        """Force a re-pack of the weights on the next call.  Needed only after writes that bypass autograd's version counter
        (``p.data.copy_(...)``, ``dist.broadcast(p.data, 0)``); optimizers, ``load_state_dict`` and ``.to()`` are seen."""
        self._session.param_versions = None

    def _fetch_input_grad(self, x, w, bits):
        """After a library call that ran with input_grad ``bits``: (G_x shaped like x, G_w shaped like w - ``check_weights`` form), None
        where the bit is off - fresh tensors (iodine_last_input_grad)."""
        f = dict(device=x.device, dtype=torch.float32)
        gx = torch.empty(x.shape, **f) if bits & 1 else None
        gw = torch.empty(w.shape if w is not None else (x.shape[0], self.img_size, self.img_size), **f) if bits & 2 else None
        self._session.call('iodine_last_input_grad', gx, gw)
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

    def _fetch_sigma_grad(self, n, weights=None):
        """After a library call that ran with sigma_grad: sum_e w_e dLL_e/dsigma over its n evaluations (weights: the iteration weights it
        ran with, () = the default; None: n = 1, the value itself) as a device scalar."""
        s = self._session
        out = s.out('t.dll', (n,))
        s.call('iodine_last_sigma_grad', out, n)
        if weights is None:
            return out[0].clone()
        wv = torch.tensor(list(weights) or [(i + 1) / n for i in range(n)], dtype=torch.float32, device=s.device)
        return (wv * out).sum()

    def _eps(self, eps, B, device):
        return self._normals(eps, (self.n_iters + 1, B, self.K, self.dim_latent), device)

    def _normals(self, eps, shape, device):
        s = self._bind(device)
        if eps is None:
            out = s.out('eps', shape)
            _lib.call('iodine_randn', device, out, out.numel(), self._seed, self._draws)
            self._draws += 1
            return out
        if tuple(eps.shape) != shape:
            raise RuntimeError(f'eps must have shape {shape}, got {tuple(eps.shape)}')
        return s.stage('eps', eps.detach().to(device=device, dtype=torch.float32).contiguous())

    def debug_buffer(self, name: str, iteration: int = 0) -> torch.Tensor:
        """Copy of an internal workspace buffer of the last call (tests only)."""
        return self._session.debug_buffer(name, iteration)

    def set_option(self, key: str, value: float):
        """Debug/test options of the library (e.g. ``stop_after_iters``); applied to the live handle.  ``graph``: hipGraph replay of the
        fixed-shape launch sequences, one graph per distinct argument tuple - which includes ``model.sigma`` / ``beta`` / ``iter_weights``:
        an objective that changes every step (a beta warm-up) runs eagerly until it repeats.  ``conv_precision``: 0 = exact fp32 MFMA (the
        strict path), 1 = split fp16, three MFMAs per product, fp32-class (default), 2 = as 1 except that the weight-stationary decoder
        convs (3 x 3, 32 / 64 channels, power-of-two image sizes >= 16, ``conv_variant`` 6) form each product from ONE fp16 MFMA of operands
        rounded to nearest even at their cell / tensor scale: fp16-class forward and data gradient for faster evaluation (``reconstruct``,
        ``predictive``, ``edit``, ``decode``); every other kernel, and every shape that kernel does not run, computes what 1 computes.
        Training at 2 is differentiated consistently, its gradients are outside the 1e-3 budget.  tests/f16x1_reference.py defines the mode."""
        if key == 'stable_encoding':                # the same switch as the attribute, which every call reads
            self.stable_encoding = bool(value)
        if key == 'joint_likelihood':               # likewise: model.likelihood is what every call sends
            if value not in (0, 1):
                raise ValueError(f'IODINE.set_option: joint_likelihood must be 0 (per_channel) or 1 (joint), got {value!r}')
            self.likelihood = 'joint' if value else 'per_channel'
        self._session.set_option(key, value)

    def profile_read(self, category: str, reset: bool = True):
        """(total_ms, launches) of one kernel category measured with HIP events (set_option('profile', 2); level 1 brackets the
        dominant ``conv_tile_*`` launches only)."""
        return self._session.profile_read(category, reset)

    # ---- inference: iodine.py:59-112 ------------------------------------------------------------
    def max_batch(self, training: bool = False, K: Optional[int] = None, T: Optional[int] = None) -> int:
        """Images one library call takes: the kernels index an activation tensor [B*K][pixels][channels] with 32-bit element
        offsets (check_ready in iodine_plan.cpp / train_forward_check in iodine_checks.cpp).  Larger batches are run in chunks of at most this many
        images by the methods below - images are independent.  The ``batch_cap`` option lowers it (tests).
        K / T: the shape of the call (default ``self.K`` / ``self.n_iters``)."""
        K, T = _args.run_shape(self.K if K is None else K, self.n_iters if T is None else T)
        P = self.img_size * self.img_size
        cd, cr = int(self._cfg.dec_conv_chan), int(self._cfg.ref_conv_chan)
        lim = ((1 << 31) - 1) // (K * P * max(cd, cr, 20))
        if training:
            lim = min(lim, ((1 << 31) - 1) // (K * T * P * 20), ((1 << 31) - 1) // (K * T * max(((self.img_size - 1) // max(int(self._cfg.ref_stride), 1) + 1) ** 2, 1) * cr))
        cap = int(self._session.options.get('batch_cap', 0))
        return max(1, min(lim, cap) if cap > 0 else lim)

    @staticmethod
    def _chunks(B, cap):                        # balanced split of B images into ceil(B / cap) runs: [(start, stop), ...]
        return [(s, e) for s, e, _ in split(B, cap)]

    # what a chunk leaves on the module and how a chunked call puts it together (_chunked.merge): tensors over the batch concatenated,
    # batch means (ELBO terms) weighted by the chunks' shares, image-0 logger entries from chunk 0
    _STATE_RULES = dict(z=CAT0, mean=CAT0, mask=CAT0, mask_logits=CAT0, log_likelihood=CAT0, K_log_likelihood=CAT0, elbo_terms=SHARE,
                        logger0=FIRST)

    def _chunk_state(self):
        keep = ('image', 'pred') + tuple(f'mask_{i}' for i in range(self.K)) + tuple(f'pred_{i}' for i in range(self.K))
        return dict({k: getattr(self, k) for k in self._STATE_RULES if k != 'logger0'}, logger0={k: logger[k] for k in keep if k in logger},
                    pm=self.posterior.mean, plv=self.posterior.logvar)

    def _merge_chunk_state(self, parts, shares, posterior=True):
        """Per-call state and logger entries of a chunked call, as one call over the whole batch would have left them; ``posterior``:
        also ``posterior.mean / logvar`` (a call that refined them; an elbo restores the caller's instead)."""
        m = merge(parts, dict(self._STATE_RULES, **(dict(pm=CAT0, plv=CAT0) if posterior else {})), shares)
        logger.update(**m.pop('logger0'))
        if posterior:
            self.posterior.mean, self.posterior.logvar = m.pop('pm'), m.pop('plv')
        for k, v in m.items():
            setattr(self, k, v)
        if self.elbo_terms.shape[0] > 0:
            logger.update(kl=self.elbo_terms[-1, 1], likelihood=self.elbo_terms[-1, 2])

    def _fetch_last_elbo(self, x, terms, frame=-1):
        """State the reference leaves on ``self`` after an ``elbo()`` call (iodine.py:171-187) and its logger entries
        (iodine.py:225-239): z, mean, mask, mask_logits of the whole batch and pred/image of image 0 (of a clip: its frame
        ``frame``, the one that call scored)."""
        B, K, L, S = x.shape[0], self.K, self.dim_latent, self.img_size
        f = dict(device=x.device, dtype=torch.float32)
        z, mean = torch.empty((B, K, L), **f), torch.empty((B, K, 3, S, S), **f)
        mask, logits, pred = torch.empty((B, K, 1, S, S), **f), torch.empty((B, K, 1, S, S), **f), torch.empty((B, 3, S, S), **f)
        self._session.call('iodine_last_elbo_outputs', B, z, mean, mask, logits, pred)
        self.z, self.mean, self.mask, self.mask_logits = z, mean, mask, logits
        self.log_likelihood = self.K_log_likelihood = None
        if self.likelihood_maps:                            # (one more per-pixel launch; off: none)
            ll, kll = torch.empty((B, 1 if self._session.joint else 3, S, S), **f), torch.empty((B, K, 3, S, S), **f)
            self._session.call('iodine_last_likelihood', B, ll, kll)
            self.log_likelihood, self.K_log_likelihood = ll, kll
        logger.update(image=x[0] if x.dim() == 4 else x[0, frame], pred=pred[0], kl=terms[1], likelihood=terms[2])
        logger.update(**{f'mask_{i}': mask[0, i, 0] for i in range(K)})
        logger.update(**{f'pred_{i}': mean[0, i] for i in range(K)})

    def _fetch_pair(self, symbol, B, K, width):
        """Two fresh (B, K, width) tensors filled by ``symbol(B, ., .)``: lambda_T, or the LSTM state (h, c), of the last call."""
        a = torch.empty((B, K, width), device=self._session.device, dtype=torch.float32)
        b = torch.empty_like(a)
        self._session.call(symbol, B, a, b)
        return a, b

    def _fetch_posterior(self, B):
        """``self.posterior.mean / logvar`` = lambda_T, what ``Gaussian.update`` (iodine.py:636-645) leaves on the reference's
        module after ``forward``: a following ``model.elbo(x)`` samples from it."""
        self.posterior.mean, self.posterior.logvar = self._fetch_pair('iodine_last_posterior', B, self.K, self.dim_latent)

    @torch.no_grad()
    def _reconstruct(self, x, eps, want_images=True, state=None, trajectory=False, keep_state=False, weights=None):
        K, T = _args.run_shape(self.K, self.n_iters)
        obj = _args.read_objective(self.sigma, self.beta, self.iter_weights, T)
        x, frames = _args.check_frames(x, T, 'encode / reconstruct', self.img_channels, self.img_size, self.n_iters)
        weights = _args.check_weights(weights, x, self.img_size, 'encode / reconstruct')
        dev, B = x.device, x.shape[0]
        stop = int(self._session.options.get('stop_after_iters', -1))
        n_it = stop if 0 <= stop <= T else T
        if trajectory and n_it != T:
            raise RuntimeError('trajectory=True needs the whole call: its last entry is the final decode, which option stop_after_iters '
                               'skips (unset it with set_option("stop_after_iters", -1))')
        state = _args.check_state(state, B, K, self.dim_latent, int(self._cfg.ref_mlp_units), dev)
        self.trajectory, self._state, self.objects = None, None, None
        cap = self.max_batch()
        if B > cap:                                   # chunks of independent images; eps (T+1, B, K, L) is cut along B
            # the next chunk re-uses the workspace, so the LSTM state of a chunk is fetched (two small copies) only where the caller
            # uses the new arguments at all: a chunked call without them runs what it ran before
            keep_state = keep_state or state is not None or trajectory
            runs, outs, parts, trs, sts = split(B, cap), [], [], [], []
            for s, e, _ in runs:
                outs.append(self._reconstruct(x[s:e], cut(eps, s, e, 1), want_images, state and tuple(t[s:e] for t in state), trajectory,
                                              weights=cut(weights, s, e)))
                parts.append(self._chunk_state())
                trs.append(self.trajectory)
                if keep_state:
                    sts.append(self.refinement_state())
            self._merge_chunk_state(parts, [w for _, _, w in runs])
            if trajectory:                            # iteration first: the batch is axis 1
                self.trajectory = merge(trs, dict.fromkeys(trs[0], CAT1))
            self._state = _RefineState(self.posterior.mean, self.posterior.logvar)
            if keep_state:
                _, _, self._state.h, self._state.c = merge(sts, (FIRST, FIRST, CAT0, CAT0))
            return merge(outs, (CAT0,) * 4)
        ses = self._bind(dev)
        ses.prepare(dev, B, 0, K, T, frames, obj, stable_encoding=self.stable_encoding, joint_likelihood=self._joint())
        eps = self._eps(eps, B, dev)
        xs = ses.stage('x', x)
        L, S = self.dim_latent, self.img_size
        images = (('r.pred', (B, 3, S, S)), ('r.mask', (B, K, 1, S, S)), ('r.mean', (B, K, 3, S, S)))
        pred, mask, mean = (ses.out(n, shp) if want_images else None for n, shp in images)
        z, pm, plv = (ses.out(n, (B, K, L)) for n in ('r.z', 'r.pm', 'r.plv'))
        elbo = ses.out('r.elbo', (n_it, 3))
        args = (B, xs, eps, pred, mask, mean, z, pm, plv, elbo)
        ses.call_serial += 1
        ws = ses.send_weights(weights)                      # (ws: alive until the call is queued)
        if state is None and not trajectory:
            ses.call('iodine_reconstruct', *args)
        else:
            # the initial state and the trajectory buffers go through persistent staging buffers in graph mode, like every other tensor
            state_ptrs, traj_out, traj_ptrs = None, None, None
            traj_names = ('pred', 'mask', 'mean', 'kl', 'll')
            if state is not None:
                state_ptrs = _lib.ptrs([ses.stage('s.' + n, t) for n, t in zip(('pm', 'plv', 'h', 'c'), state)])
            if trajectory:
                shapes = ((T + 1, B, 3, S, S), (T + 1, B, K, 1, S, S), (T + 1, B, K, 3, S, S), (T, B), (T, B))
                traj_out = [ses.out('tr.' + n, shp) for n, shp in zip(traj_names, shapes)]
                traj_ptrs = _lib.ptrs(traj_out)
            ses.call('iodine_reconstruct_seq', *args, state_ptrs, traj_ptrs)
            if trajectory:
                self.trajectory = {n: ses.own(t) for n, t in zip(traj_names, traj_out)}
        pred, mask, mean, z, pm, plv, elbo = (ses.own(t) for t in (pred, mask, mean, z, pm, plv, elbo))
        self.posterior.mean, self.posterior.logvar, self.elbo_terms = pm, plv, elbo
        self._state = _RefineState(pm, plv, serial=ses.call_serial)     # h, c stay in the workspace until asked for (refinement_state)
        if n_it > 0:
            self._fetch_last_elbo(x, elbo[-1], frame=n_it - 1)      # what the reference's last elbo() call left behind
        return pred, mask, mean, z

    def encode(self, x, eps=None, state=None, keep_state=False, weights=None):
        """z (B, K, L) after T refinement iterations.  iodine.py:73-105.  ``x``: images (B, 3, S, S) or a clip (B, T, 3, S, S) -
        iteration i then scores, differentiates and encodes frame i.  ``state`` / ``keep_state`` / ``weights``: see ``reconstruct``."""
        return self._reconstruct(x, eps, want_images=False, state=state, keep_state=keep_state, weights=weights)[3]

    def reconstruct(self, x, eps=None, trajectory=False, state=None, keep_state=False, weights=None, objects=False, components=False):
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
        ``model.objects = None``, adds no launch and returns the same bits.

        ``components=True`` or a dict of ``connectivity`` / ``min_area`` / ``max_components`` / ``clean`` (needs ``objects=True``, else
        ValueError) adds ``model.objects['components']``: ``iodine_amd.objects.components`` of ``model.objects['segmentation']`` - the
        connected components of the map, one more call after the table's, so a chunked batch gives the same result; with
        ``trajectory=True`` also ``model.trajectory['components']`` over every entry.  Without it there is no such key and no launch."""
        want_components = components is not None and components is not False
        if want_components:                           # refused before any device work
            if not objects:
                raise ValueError("IODINE.reconstruct: components= reads model.objects['segmentation'] and needs objects=True")
            components = {} if components is True else dict(components)
            unknown = sorted(set(components) - {'connectivity', 'min_area', 'max_components', 'clean'})
            if unknown:
                raise ValueError(f'IODINE.reconstruct: components= takes connectivity, min_area, max_components and clean; got {unknown}')
        pred, mask, mean, _ = self._reconstruct(x, eps, state=state, trajectory=trajectory, keep_state=keep_state, weights=weights)
        if objects:
            self._read_objects(mask, mean, trajectory)
            if want_components:
                self._read_components(components, trajectory)
        return pred, mask, mean

    @torch.no_grad()
    def _read_components(self, options, trajectory):
        """``model.objects['components']`` (and the trajectory's) of a finished reconstruct(objects=True): see there."""
        from .objects import components
        K = int(self.objects['table'].shape[-2])      # the slots of the masks the map was taken from
        if trajectory:                                # one call over all T + 1 entries; the last is the returned decode
            comp = components(self.trajectory['segmentation'], K, **options)
            self.trajectory['components'] = comp
            comp = type(comp)(*(None if t is None else t[-1] for t in comp))
        else:
            comp = components(self.objects['segmentation'], K, **options)
        self.objects['components'] = comp

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
            if st.serial != self._session.call_serial:
                raise RuntimeError('IODINE.refinement_state: another model call has re-used the workspace since the encode / reconstruct '
                                   'whose state is asked for - call refinement_state() right after it')
            st.h, st.c = self._fetch_pair('iodine_last_refine_state', *st.post_mean.shape[:2], int(self._cfg.ref_mlp_units))
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
        T = self._session.shape[1]         # the iteration count plays no part in a decode: keep the handle's (no workspace re-plan for it)
        z = z.detach().to(torch.float32).contiguous()
        B = z.shape[0]
        cap = self.max_batch(K=K, T=T)
        if B > cap:
            return merge([self._decode_nograd(z[s:e]) for s, e, _ in split(B, cap)], (CAT0,) * 3)
        return self._decode_call(z, K, T, save=False)

    def _decode_call(self, z, K, T, save):
        """One iodine_decode of at most ``max_batch`` slots-images; ``save``: kept for iodine_decode_backward."""
        dev, B, S = z.device, z.shape[0], self.img_size
        ses = self._bind(dev)
        ses.prepare(dev, B, 2 if save else 0, K, T)
        z = ses.stage('d.z', z)
        pred, mask, mean = ses.out('r.pred', (B, 3, S, S)), ses.out('r.mask', (B, K, 1, S, S)), ses.out('r.mean', (B, K, 3, S, S))
        ses.call_serial += 1
        with ses.saving(save):
            ses.call('iodine_decode', B, z, pred, mask, mean)
        return ses.own(pred), ses.own(mask), ses.own(mean)

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
        image = _args.int_list(image, 'image')
        E = len(image)
        if E < 1:
            raise ValueError('IODINE.edit: the edit list is empty (image has no entries)')
        slot = _args.int_list(slot, 'slot', E)
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
        T = self._session.shape[1]                          # plays no part, as in decode
        cap = self.max_batch(K=K, T=T)
        if B > cap:
            raise ValueError(f'IODINE.edit: z has {B} images, one call takes at most max_batch() = {cap} at K = {K}: edit the scenes in groups')
        dev = z.device
        z = z.detach().to(torch.float32).contiguous()
        zn = z_new.detach().to(torch.float32).contiguous() if n_rep > 0 else None
        W = min(cap, max(B, -(-n_rep // K)))
        ses = self._bind(dev)
        ses.prepare(dev, W, 0, K, T)
        S = self.img_size
        f = dict(device=dev, dtype=torch.float32)
        pred = torch.empty((E, 3, S, S), **f)
        mask = torch.empty((E, K, 1, S, S), **f) if return_mask else None
        mean = torch.empty((E, 3, S, S), **f) if return_mean else None
        base = (torch.empty((B, 3, S, S), **f), torch.empty((B, K, 1, S, S), **f), torch.empty((B, K, 3, S, S), **f)) if return_base else (None,) * 3
        ses.call_serial += 1
        ses.call('iodine_scene_edit', B, z, E, _lib.ints(image), _lib.ints(slot), _lib.ints([int(r) for r in remove]), zn, W,
                 pred, mask, mean, *base)
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
            x = _args.check_x(x, self.img_channels, self.img_size)
            if x.shape[0] != B:
                raise ValueError(f'IODINE.predictive: x has {x.shape[0]} images, the posterior {B}')
            weights = _args.check_weights(weights, x, self.img_size, 'predictive')
        T = self._session.shape[1]                          # plays no part, as in decode
        sigma = _args.read_objective(self.sigma, self.beta, self.iter_weights, T)[0]
        dev = pm.device
        ses = self._bind(dev)                               # (a CPU tensor is refused here, after the argument checks)
        if plv.device != dev or (x is not None and x.device != dev):
            raise ValueError('IODINE.predictive: the posterior and x must be on the same device')
        pm, plv = pm.detach().to(torch.float32).contiguous(), plv.detach().to(torch.float32).contiguous()
        cap = self.max_batch(K=K, T=T)
        if B > cap:                                         # groups of independent images; the noise is cut along its batch axis
            parts = [self.predictive(cut(x, s, e), S, (pm[s:e], plv[s:e]), cut(eps, s, e, 1), cut(weights, s, e)) for s, e, _ in split(B, cap)]
            return Predictive(**merge([vars(q) for q in parts], Predictive.MERGE))
        if eps is None:                                     # one draw id per sample
            eps = torch.empty((S, B, K, L), device=dev, dtype=torch.float32)
            for s in range(S):
                eps[s].copy_(self._normals(None, (B, K, L), dev))
        else:
            eps = eps.detach().to(device=dev, dtype=torch.float32).contiguous()
        W = min(cap, max(B, min(S * B, self._PREDICTIVE_IMAGES)))
        st = self._state                                    # the arena is re-planned for W images: an LSTM state still in it is fetched first
        if st is not None and st.h is None and st.serial is not None and st.serial == ses.call_serial:
            self.refinement_state()
        # sigma of this call; beta / iteration weights play no part
        ses.prepare(dev, W, 0, K, T, objective=(sigma,) + tuple(ses.objective[1:]), stable_encoding=self.stable_encoding,
                    joint_likelihood=self._joint())
        f = dict(device=dev, dtype=torch.float32)
        z = torch.empty((S, B, K, L), **f)
        pmean, pm2 = torch.empty((B, 3, Si, Si), **f), torch.empty((B, 3, Si, Si), **f)
        mmean, mm2 = torch.empty((B, K, 1, Si, Si), **f), torch.empty((B, K, 1, Si, Si), **f)
        votes = torch.empty((B, K, Si, Si), device=dev, dtype=torch.int32)
        ll = torch.empty((S, B), **f) if x is not None else None
        ses.call_serial += 1
        ws = ses.send_weights(weights)                      # (ws: alive until the call is queued)
        ses.call('iodine_predictive', B, S, pm, plv, eps, x, W, z, pmean, pm2, mmean, mm2, votes, ll)
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

    MAX_CHAINS = 1024

    def _check_restarts(self, x, chains, eps, state, trajectory):
        """The host-only refusals of ``restarts`` -> (C, K, T); every one a ValueError, before any device work."""
        if isinstance(chains, bool) or not isinstance(chains, numbers.Integral) or not 1 <= chains <= self.MAX_CHAINS:
            raise ValueError(f'IODINE.restarts: chains must be an integer in 1..{self.MAX_CHAINS}; got {chains!r}')
        if state is not None or trajectory:
            raise ValueError('IODINE.restarts: state= and trajectory= are not supported - every chain starts from the initial posterior and '
                             'only the returned decode of a chain is scored')
        c, s = self.img_channels, self.img_size
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (c, s, s) or x.shape[0] < 1:
            clip = ' (a clip is not supported: the final decode of a clip has no frame of its own to be scored against)' if torch.is_tensor(x) and x.dim() == 5 else ''
            raise ValueError(f'IODINE.restarts: x must be images of shape (B, {c}, {s}, {s}){clip}; got '
                             f'{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
        K, T = _args.run_shape(self.K, self.n_iters)
        want = (int(chains), T + 1, int(x.shape[0]), K, self.dim_latent)
        if eps is not None and (not torch.is_tensor(eps) or tuple(eps.shape) != want):
            raise ValueError(f'IODINE.restarts: eps must have shape {want} (chains, T + 1, B, K, L); got '
                             f'{tuple(eps.shape) if torch.is_tensor(eps) else type(eps).__name__}')
        return int(chains), K, T

    @torch.no_grad()
    def restarts(self, x, chains=8, eps=None, weights=None, consensus=True, state=None, trajectory=False, keep_decodes=False):
        """``chains`` refinement chains per image from the same initial posterior with different noise, the best one per image, and how
        far the chains agree - inference is stochastic and multi-stable, and a single ``reconstruct`` shows one mode.  Returns a ``Restarts``.

        Run: ONE ``reconstruct`` over the batch repeated chain-major (row ``c B + b`` is chain c of image b; above ``max_batch()`` the
        usual chunks of independent images).  ``eps``: (C, T + 1, B, K, L), or None for one draw of that shape from the model's generator;
        chain c is the computation ``reconstruct(x, eps[c])`` runs.  ``weights``: the per-pixel observation weights of every chain and of
        the score, as everywhere else.
        Score: ``ll[c, b]`` = the (weighted) log-likelihood of the decode the chain RETURNS (``iodine_chain_score``, with ``model.sigma``
        and ``model.likelihood``; ``elbo_terms`` scores lambda_0 .. lambda_{T-1} only), ``kl[c, b]`` = KL(lambda_T || N(0, 1)) in closed form,
        ``score = ll - model.beta kl``; ``best[b] = argmax_c score``, the lowest chain on a tie, a NaN never wins, 0 if every score is NaN.
        Select: ``pred, mask, mean, z, post_mean, post_logvar`` of the best chain per image, gathered on the device without a
        synchronisation; ``model.posterior.mean / logvar`` are the chosen lambda_T, so ``predictive`` and ``elbo`` continue from the chosen
        mode; ``model.objects``, ``model.trajectory`` and the refinement state are None afterwards.  Every other per-call attribute
        (``model.z / mean / mask / mask_logits``, ``elbo_terms``, the likelihood maps, the logger) is that of the underlying C B call.
        Align and fold (``consensus=True``): the overlap of every chain's arg-max map with the best chain's (``overlap_table``, one launch),
        ``1 - slot_iou`` into ``matching.assign`` for ``perm``, and ``iodine_chain_consensus`` for votes, consensus, agreement, match and the
        mean relabelled mask.  ``keep_decodes=True`` also hands back every chain's decode (``Restarts.decodes``; no copy).

        NOT differentiable.  ``state=`` / ``trajectory=`` and a clip ``x`` are refused (ValueError), like every other bad argument, before
        any device work."""
        C, K, T = self._check_restarts(x, chains, eps, state, trajectory)
        sigma, beta, _ = _args.read_objective(self.sigma, self.beta, self.iter_weights, T)
        xc = _args.check_x(x, self.img_channels, self.img_size)
        w = _args.check_weights(weights, xc, self.img_size, 'restarts')
        dev, B, L, S = xc.device, int(xc.shape[0]), self.dim_latent, self.img_size
        self._bind(dev)                                     # (a CPU tensor is refused here, after the argument checks)
        from . import chains as _chains
        if eps is None:                                     # one draw for all chains; a copy: the generator's buffer is the session's
            eps = self._normals(None, (C, T + 1, B, K, L), dev).clone()
        eps = eps.detach().to(device=dev, dtype=torch.float32)
        pred, mask, mean, z = self._reconstruct(xc.repeat(C, 1, 1, 1), eps.permute(1, 0, 2, 3, 4).reshape(T + 1, C * B, K, L),
                                                weights=None if w is None else w.repeat(C, 1, 1))
        pm, plv = self.posterior.mean, self.posterior.logvar
        ll, seg = _chains.chain_score(xc, mask.view(C, B, K, 1, S, S), mean.view(C, B, K, 3, S, S), sigma, weights=w, joint=self._joint())
        pm64, plv64 = pm.double(), plv.double()             # (C B, K, L): tiny; fp64 keeps exp(lv) - 1 - lv near lv = 0, as _read_objects
        kl = (0.5 * (plv64.exp() + pm64 * pm64 - 1.0 - plv64).sum((-2, -1))).view(C, B)
        score = ll.double() - beta * kl
        key = torch.where(torch.isnan(score), torch.full_like(score, -float('inf')), score)
        best = ((key == key.max(0).values).cumsum(0) == 0).sum(0)           # the first chain that holds the maximum; 0 if all are NaN
        rows = best * B + torch.arange(B, device=dev)
        out = Restarts(*(t.index_select(0, rows) for t in (pred, mask, mean, z, pm, plv)), best, score, ll, kl, seg, C)
        self.posterior.mean, self.posterior.logvar = out.post_mean, out.post_logvar
        self.objects, self.trajectory, self._state = None, None, None
        if keep_decodes:
            out.decodes = (pred.view(C, B, 3, S, S), mask.view(C, B, K, 1, S, S), mean.view(C, B, K, 3, S, S))
        if consensus:
            from .matching import assign
            from .objects import overlap_table, slot_iou
            seg_best = seg.view(C * B, S, S).index_select(0, rows)
            out.overlap = overlap_table(seg, seg_best.unsqueeze(0).expand(C, B, S, S).contiguous(), K, K)
            perm = assign((1.0 - slot_iou(out.overlap)).float())[0]
            perm.view(C * B, K)[rows] = torch.arange(K, dtype=torch.int32, device=dev)     # the common labelling IS the best chain's
            out.perm = perm
            cons = _chains.chain_consensus(seg, perm, best.to(torch.int32), mask.view(C, B, K, 1, S, S))
            out.votes, out.consensus, out.agreement, out.match, out.mask_mean = cons
            m64 = cons.match.double()
            own = m64.gather(0, best.view(1, B))[0]
            out.stability = ((m64.sum(0) - own) / (C - 1)).float() if C > 1 else torch.ones(B, dtype=torch.float32, device=dev)
        return out

    def _check_adaptive(self, x, tol, rtol, max_iters, min_iters, check_every, budget, eps):
        """The host-only refusals of ``reconstruct_adaptive`` -> (ctl, K, budget as int32 on the host or None); every one a ValueError,
        before any device work."""
        from . import adaptive as _ad
        who = 'IODINE.reconstruct_adaptive'
        c, s = self.img_channels, self.img_size
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (c, s, s) or x.shape[0] < 1:
            clip = ' (a clip is not supported: its frames belong to fixed iterations)' if torch.is_tensor(x) and x.dim() == 5 else ''
            raise ValueError(f'{who}: x must be images of shape (B, {c}, {s}, {s}){clip}; got '
                             f'{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
        given_r = not isinstance(rtol, bool) and isinstance(rtol, (int, float)) and rtol > 0
        if tol is None and budget is None and not given_r:
            raise ValueError(f'{who}: give at least one of tol, rtol (> 0) or budget - without any the call is a fixed reconstruct')
        K, T = _args.run_shape(self.K, self.n_iters if max_iters is None else max_iters)
        # no tol: the relative rule alone (tol 0) where rtol is given, else only the budget stops an image early (tol -inf)
        ctl = _ad.controls(T, min_iters, check_every, (0.0 if given_r else -math.inf) if tol is None else tol, rtol, who)
        B = int(x.shape[0])
        if budget is not None:
            if (not torch.is_tensor(budget) or budget.is_floating_point() or budget.is_complex() or budget.dtype == torch.bool
                    or tuple(budget.shape) != (B,)):
                raise ValueError(f'{who}: budget must be an integer tensor of shape ({B},); got '
                                 f'{(budget.dtype, tuple(budget.shape)) if torch.is_tensor(budget) else type(budget).__name__}')
            budget = budget.detach().to(device='cpu', dtype=torch.int64)
            if int(budget.min()) < 1 or int(budget.max()) > T:
                raise ValueError(f'{who}: budget values must be in 1..max_iters = {T}; got {int(budget.min())}..{int(budget.max())}')
            budget = budget.to(torch.int32)
        want = (T + 1, B, K, self.dim_latent)
        if eps is not None and (not torch.is_tensor(eps) or tuple(eps.shape) != want):
            raise ValueError(f'{who}: eps must have shape {want} (max_iters + 1, B, K, L); got '
                             f'{tuple(eps.shape) if torch.is_tensor(eps) else type(eps).__name__}')
        return ctl, K, budget

    @torch.no_grad()
    def reconstruct_adaptive(self, x, tol=None, rtol=0.0, max_iters=None, min_iters=2, check_every=1, budget=None, eps=None, state=None,
                             weights=None):
        """``reconstruct`` with a per-image iteration count: every image is refined until ITS ELBO estimate stops improving, then leaves
        the batch - the later iterations run on the images still moving, so the cost follows ``sum(iters)``, not ``B max_iters``.  Returns
        an ``iodine_amd.adaptive.Adaptive``; ``Adaptive.iters`` is a diagnostic of its own ("iterations to converge" per image).

        The rule (tests/adaptive_reference.py defines it, in float64): with ``s_i = ll_i - model.beta kl_i`` of ELBO evaluation i of an
        image (the per-image terms ``trajectory['ll'] / ['kl']`` hold), after t in {check_every, 2 check_every, ..} < max_iters updates the
        image stops when ``t >= budget[b]``, or when ``t >= max(min_iters, 2)`` and ``s_{t-1} - s_{t-2} < tol + rtol |s_{t-2}|``; a NaN or
        an infinity that makes either side NaN keeps the image running; at ``max_iters`` (default ``model.n_iters``) everything stops.
        EVERY EVALUATION DRAWS FRESH NOISE: s is a one-sample estimate of the ELBO, so ``tol`` has to sit above that noise or images stop
        by chance (it may be negative: "stop once the estimate no longer rises by more than the noise"), and with ``check_every > 1`` only
        evaluations t - 1 and t - 2 are compared, not the gain of the whole round.  ``tol=-inf``: never stop early; ``+inf``: stop at the
        first permitted check.  ``tol=None``: 0 with an ``rtol > 0``, else the budget alone decides.  ``budget``: integer tensor (B,) with
        values in 1..max_iters, an iteration allowance per image (rounded up to a multiple of ``check_every``).

        For image b with t = iters[b]: ``pred, mask, mean, z, post_mean, post_logvar`` and the LSTM state are, bit for bit, what
        ``reconstruct`` + ``refinement_state()`` give with ``n_iters = t`` and the noise rows ``cat(eps[:t], eps[max_iters:])`` - the final
        sample of every image uses the LAST row of ``eps (max_iters + 1, B, K, L)`` -; ``ll[:t, b]`` / ``kl[:t, b]`` are that call's
        trajectory, the rows from t on NaN.  ``state`` / ``weights``: as ``reconstruct`` (``max_iters`` FURTHER iterations at most).
        Batches above ``max_batch()`` run in chunks and are merged (``active`` adds up over the chunks).

        Afterwards ``model.posterior`` holds the final posteriors and ``refinement_state()`` returns the full-batch (post_mean,
        post_logvar, h, c) of this call; ``elbo_terms``, ``trajectory`` and ``objects`` are None.  ``model.z / mean / mask / mask_logits``,
        the likelihood maps and the logger are LEFT AS THEY WERE: they describe "the last ELBO evaluation", and no single evaluation is
        the last for all images here.  NOT differentiable; never part of a hipGraph (with option ``graph`` the call runs eagerly - it
        reads two counts back after every round).  A clip ``x`` and every other bad argument is a ValueError before any device work."""
        from . import adaptive as _ad
        ctl, K, budget = self._check_adaptive(x, tol, rtol, max_iters, min_iters, check_every, budget, eps)
        M, R = int(ctl.max_iters), int(ctl.check_every)
        # (the handle runs at T = check_every; inference reads no iteration weights, so the default table is what it is given)
        obj = _args.read_objective(self.sigma, self.beta, None, R)
        xc = _args.check_x(x, self.img_channels, self.img_size)
        w = _args.check_weights(weights, xc, self.img_size, 'reconstruct_adaptive')
        dev, B, L, H = xc.device, int(xc.shape[0]), self.dim_latent, int(self._cfg.ref_mlp_units)
        self._bind(dev)                                     # (a CPU tensor is refused here, after the argument checks)
        state = _args.check_state(state, B, K, L, H, dev)
        if eps is None:
            eps = self._normals(None, (M + 1, B, K, L), dev).clone()
        eps = eps.detach().to(device=dev, dtype=torch.float32).contiguous()
        bud = None if budget is None else budget.to(dev)
        self.trajectory, self._state, self.objects, self.elbo_terms = None, None, None, None
        runs = split(B, self.max_batch(K=K, T=R))
        parts = []
        for s, e, _ in runs:                                # chunks of independent images; eps (max_iters + 1, B, K, L) is cut along B
            one = len(runs) == 1
            parts.append(self._adaptive_call(xc if one else xc[s:e].contiguous(), eps if one else cut(eps, s, e, 1).contiguous(),
                                             cut(w, s, e), state and tuple(t[s:e].contiguous() for t in state),
                                             None if bud is None else bud[s:e].contiguous(), ctl, K, obj))
        out = parts[0] if len(parts) == 1 else merge(parts, (CAT0,) * 9 + (CAT1, CAT1))
        pred, mask, mean, z, pm, plv, h, c, iters, ll, kl = out
        active = [sum(col) for col in zip(*(p.active for p in parts))]
        self.posterior.mean, self.posterior.logvar = pm, plv
        self._state = _RefineState(pm, plv, h, c)           # fetched: no workspace read is needed later
        return _ad.Adaptive(pred, mask, mean, z, pm, plv, iters, ll, kl, ll.double() - obj[1] * kl.double(), active)

    class _AdaptivePart(tuple):
        active = ()

    def _adaptive_call(self, x, eps, w, state, budget, ctl, K, obj):
        """One library call of ``reconstruct_adaptive`` (a whole batch, or a chunk of one) -> (pred, mask, mean, z, post_mean, post_logvar, h,
        c, iters, ll, kl) with ``.active``."""
        import ctypes as C
        dev, B, L, S, H = x.device, int(x.shape[0]), self.dim_latent, self.img_size, int(self._cfg.ref_mlp_units)
        M, R = int(ctl.max_iters), int(ctl.check_every)
        ses = self._bind(dev)
        ses.prepare(dev, B, 0, K, R, 0, obj, stable_encoding=self.stable_encoding, joint_likelihood=self._joint())
        f = dict(device=dev, dtype=torch.float32)
        pred, mask, mean = torch.empty((B, 3, S, S), **f), torch.empty((B, K, 1, S, S), **f), torch.empty((B, K, 3, S, S), **f)
        z, pm, plv = (torch.empty((B, K, L), **f) for _ in range(3))
        h, c = (torch.empty((B, K, H), **f) for _ in range(2))
        iters = torch.empty((B,), device=dev, dtype=torch.int32)
        ll, kl = (torch.empty((M, B), **f) for _ in range(2))
        active = (C.c_int * (-(-M // R)))()
        ses.call_serial += 1
        ws = ses.send_weights(w)                            # (ws: alive until the call is queued)
        ses.call('iodine_reconstruct_adaptive', B, x, eps, C.byref(ctl), budget, None if state is None else _lib.ptrs(list(state)),
                 pred, mask, mean, z, pm, plv, h, c, iters, ll, kl, active)
        del ws
        part = self._AdaptivePart((pred, mask, mean, z, pm, plv, h, c, iters, ll, kl))
        part.active = list(active)
        return part

    _STALE = ('IODINE: backward of a stale {0} -the library keeps the saved state of ONE differentiable call and another forward / '
              'reconstruct / decode / elbo call has re-used it since, or it was differentiated already (the reference would hold a second '
              'autograd graph; call backward() before the next model call)')

    def _decode_backward(self, serial, K, grads, want_z, want_p, flat):
        """iodine_decode_backward for the saved decode ``serial``: (dz or None, flat parameter gradients or None).  ``flat``: a buffer
        of earlier chunks to accumulate into."""
        ses = self._session
        if serial != ses.call_serial:
            raise RuntimeError(self._STALE.format('decode'))
        dev = ses.device
        B = next(g for g in grads if g is not None).shape[0]
        S, names = self.img_size, ('dg.pred', 'dg.mask', 'dg.mean')
        shapes = ((B, 3, S, S), (B, K, 1, S, S), (B, K, 3, S, S))
        gs = []
        for g, n, shp in zip(grads, names, shapes):
            if g is not None and tuple(g.shape) != shp:
                raise RuntimeError(f'IODINE.decode backward: gradient of shape {tuple(g.shape)}, expected {shp}')
            gs.append(None if g is None else ses.stage(n, g.detach().to(device=dev, dtype=torch.float32).contiguous()))
        dz = ses.out('dg.dz', (B, K, self.dim_latent)) if want_z else None
        acc = flat is not None
        if want_p and flat is None:
            flat = self._flat_out()
        ses.call('iodine_decode_backward', B, *gs, dz, flat if want_p else None, 1 if acc else 0)
        ses.call_serial += 1                        # the saved pass is consumed (no retain_graph)
        return ses.own(dz), flat                    # (flat: the caller takes its copy - graph mode - after its last chunk)

    def _flat_out(self):
        """The buffer d / d parameters is written to, in named_parameters() order."""
        return self._session.out('t.flat', (sum(p.numel() for p in self._ordered_params()),))

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
            xc = _args.check_x(x, self.img_channels, self.img_size)     # (model.K / n_iters are checked by _elbo_call, before any device work)
            w = _args.check_weights(weights, xc, self.img_size, 'weighted_elbo')
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
        K, T = _args.run_shape(self.K, self.n_iters)
        _args.read_objective(self.sigma, self.beta, self.iter_weights, T)
        x = _args.check_x(x, self.img_channels, self.img_size)
        weights = _args.check_weights(weights, x, self.img_size, 'weighted_elbo')
        dev, B = x.device, x.shape[0]
        cap = self.max_batch()
        if B > cap:
            pm0, plv0 = self.posterior.mean, self.posterior.logvar
            whole = pm0 is not None and plv0 is not None and tuple(pm0.shape) == (B, self.K, self.dim_latent) and pm0.device == dev
            runs, parts = split(B, cap), []
            for s, e, _ in runs:
                # the chunk's slice of the current posterior (or the initial posterior, as for a whole batch)
                self.posterior.mean, self.posterior.logvar = (pm0[s:e], plv0[s:e]) if whole else (None, None)
                self._elbo_nograd(x[s:e], cut(eps, s, e), cut(weights, s, e))
                parts.append(self._chunk_state())
            self.posterior.mean, self.posterior.logvar = pm0, plv0
            self._merge_chunk_state(parts, [w for _, _, w in runs], posterior=False)
            return self.elbo_terms[0, 0]
        pm, plv = self.posterior.mean, self.posterior.logvar
        if pm is None or plv is None or tuple(pm.shape) != (B, K, self.dim_latent) or pm.device != dev:
            pm = plv = None
        return self._elbo_call(x, eps, pm, plv, save=False, weights=weights)

    def _elbo_call(self, x, eps, pm, plv, save, weights=None, sigma_grad=False, input_grad=0):
        """One iodine_elbo of at most ``max_batch`` images from the posterior (pm, plv) - None: the initial one; ``save``: kept for
        iodine_elbo_backward.  x as ``_check_x``, weights as ``_check_weights`` return them.  -> the ELBO; with ``sigma_grad`` (a saved call
        only) -> (ELBO, d LL / d sigma)."""
        K, T = _args.run_shape(self.K, self.n_iters)
        obj = _args.read_objective(self.sigma, self.beta, self.iter_weights, T)
        dev, B = x.device, x.shape[0]
        input_grad = input_grad if save else 0
        ses = self._bind(dev)
        ses.prepare(dev, B, 2 if save else 0, K, T, None, obj, save and sigma_grad, input_grad, self.stable_encoding, self._joint())
        eps = self._normals(eps, (B, K, self.dim_latent), dev)
        if pm is not None:
            pm = ses.stage('e.pm', pm.detach().to(torch.float32).contiguous())
            plv = ses.stage('e.plv', plv.detach().to(torch.float32).contiguous())
        terms = ses.out('e.terms', (3,))
        xs = ses.stage('x', x)
        ses.call_serial += 1
        ws = ses.send_weights(weights)                      # (ws: alive until the call is queued)
        with ses.saving(save):
            ses.call('iodine_elbo', B, xs, pm, plv, eps, terms)
        terms = ses.own(terms)
        self.elbo_terms = terms.view(1, 3)
        sg = self._fetch_sigma_grad(1) if save and sigma_grad else None
        self._last_ig = self._fetch_input_grad(x, weights, input_grad) if input_grad else None
        self._fetch_last_elbo(x, terms)
        elbo = terms[0].clone() if save else terms[0]
        return (elbo, sg) if sigma_grad else elbo

    def _elbo_backward(self, serial, BK, grad_out, want_post, want_p, flat=None):
        """iodine_elbo_backward for the saved elbo ``serial``: (d / d posterior.mean, d / d posterior.logvar, flat parameter gradients),
        each None when not asked for.  ``flat``: a buffer of earlier chunks to accumulate into."""
        ses = self._session
        if serial != ses.call_serial:
            raise RuntimeError(self._STALE.format('elbo'))
        dev, (B, K) = ses.device, BK                # batch and slots of the saved call
        gl = ses.stage('e.gl', grad_out.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous())
        gpm, gplv = (ses.out(n, (B, K, self.dim_latent)) if want_post else None for n in ('e.gpm', 'e.gplv'))
        acc = flat is not None
        if want_p and flat is None:
            flat = self._flat_out()
        ses.call('iodine_elbo_backward', gl, gpm, gplv, flat if want_p else None, 1 if acc else 0)
        ses.call_serial += 1                        # the saved pass is consumed (no retain_graph)
        return ses.own(gpm), ses.own(gplv), flat            # (flat: the caller takes its copy - graph mode - after its last chunk)

    def _elbo_chunked_grad(self, x, eps, pm, plv, want_post, want_p, weights=None, sigma_grad=False, input_grad=0):
        """Differentiable elbo of a batch above ``max_batch`` (see _ElboGrad): forward + backward of every chunk with its share of the
        batch mean.  Returns the ELBO, (d / d posterior.mean, d / d posterior.logvar, flat parameter gradients) for grad_output 1 and, with
        ``sigma_grad``, d LL / d sigma of the batch (else None)."""
        dev, B = x.device, x.shape[0]
        runs, parts, grads, flat, shared = split(B, self.max_batch()), [], [], None, []
        pm0, plv0 = self.posterior.mean, self.posterior.logvar
        for s, e, share in runs:
            r = self._elbo_call(x[s:e].contiguous(), cut(eps, s, e), cut(pm, s, e), cut(plv, s, e), save=True,
                                weights=cut(weights, s, e), sigma_grad=sigma_grad, input_grad=input_grad)
            parts.append(self._chunk_state())
            w = torch.full((), share, device=dev, dtype=torch.float32)
            shared.append(scaled(w, r[1] if sigma_grad else None, *(self._last_ig or (None, None))))     # this chunk's share of the batch mean
            gpm, gplv, flat = self._elbo_backward(self._session.call_serial, (e - s, self.K), w, want_post, want_p, flat)
            if not want_p:
                flat = None
            grads.append((gpm, gplv))
        self.posterior.mean, self.posterior.logvar = pm0, plv0
        self._merge_chunk_state(parts, [w for _, _, w in runs], posterior=False)
        sig, *ig = merge(shared, (SUM, CAT0, CAT0))
        self._last_ig = tuple(ig) if input_grad else None
        return self.elbo_terms[0, 0].clone(), (*merge(grads, (CAT0, CAT0)), self._session.own(flat)), sig

    # ---- training: iodine.py:115-158 + lib/engine/train.py:60-63 -------------------------------------
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
        K, T = _args.run_shape(self.K, self.n_iters)
        _args.read_objective(self.sigma, self.beta, self.iter_weights, T)                      # (refusals before any device work; _train_forward hands it to the handle)
        x_given, w_given = x, weights
        x, _ = _args.check_frames(x, T + 1, 'forward' if state is None else 'forward from a state', self.img_channels, self.img_size, self.n_iters)
        weights = _args.check_weights(weights, x, self.img_size, 'forward')
        xi, wi = self._grad_inputs(x_given, w_given, x, weights)   # (the nodes' inputs 1 and 3: the caller's tensors where they require grad)
        B = x.shape[0]
        state = _args.check_state(state, B, K, self.dim_latent, int(self._cfg.ref_mlp_units), x.device, train=True)
        index = _args.check_attach_frames(attach_frames, T)
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
            loss, self.elbo_terms = _ChunkedTrainStep.apply(self, xi, eps, wi, state, bool(keep_state), *self._ordered_params(), *sg)
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
        B, hc = x.shape[0], None
        if not attach:
            self._fetch_last_elbo(x, terms[-1])
            self._fetch_posterior(B)
        if keep_state:
            hc = tuple(t.detach().view(B, self.K, -1) for t in self.lstm_hidden) if attach else self._fetch_pair('iodine_last_train_state', B, self.K, int(self._cfg.ref_mlp_units))
        if scalars:
            stats = torch.empty((2,), device=x.device, dtype=torch.float32)
            self._session.call('iodine_logger_scalars', stats)
            logger.update(init_mean=stats[0], init_logvar=stats[1])
        return hc

    def _train_forward(self, x, eps, state=None, weights=None, frames=None, sigma_grad=False, input_grad=0):
        """iodine_train_forward_frames -> (loss, ELBO terms, frames, S).  ``state``: None or the initial (post_mean, post_logvar, h, c);
        ``frames``: None -> (), or a tuple of evaluation indices, possibly empty -> the six (F, B, K, ...) tensors of those evaluations in
        the order of ``_FRAME_KEYS``; S: with ``sigma_grad`` the device scalar sum_e w_e dLL_e/dsigma (the forward then runs with option
        sigma_grad), else None.  NULL / 0 for what is not asked for: the library then runs the plain forward, launch for launch."""
        dev, B = x.device, x.shape[0]
        K, T = _args.run_shape(self.K, self.n_iters)
        obj = _args.read_objective(self.sigma, self.beta, self.iter_weights, T)
        ses = self._bind(dev)
        ses.prepare(dev, B, 1, K, T, x.shape[1] if x.dim() == 5 else 0, obj, sigma_grad, input_grad, self.stable_encoding, self._joint())
        loss, elbo_iter = ses.out('t.loss', ()), ses.out('t.elbo', (T + 1, 3))
        xs, eps = ses.stage('x', x), ses.stage('eps', eps)
        ses.call_serial += 1
        ws = ses.send_weights(weights)                      # (ws: alive until the call is queued)
        outs, sptrs, optrs, idx, F = (), None, None, None, len(frames or ())
        if frames is not None:
            L, S = self.dim_latent, self.img_size
            shapes = ((F, B, K, L), (F, B, K, 3, S, S), (F, B, K, 1, S, S), (F, B, K, 1, S, S), (F, B, K, L), (F, B, K, L))
            outs = [ses.out('tf.' + n, shp) for n, shp in zip(_FRAME_KEYS, shapes)]
        if F:
            optrs, idx = _lib.ptrs(outs), _lib.ints(frames)
        if state is not None:
            # (graph mode: the state goes through persistent staging buffers like reconstruct's, so the graph key repeats)
            st = [ses.stage('ts.' + n, t.detach()) for n, t in zip(('pm', 'plv', 'h', 'c'), state)]
            sptrs = _lib.ptrs(st)
        ses.call('iodine_train_forward_frames', B, xs, eps, sptrs, loss, elbo_iter, idx, F, optrs)
        out = (ses.own(loss), ses.own(elbo_iter), tuple(ses.own(t) for t in outs))
        # (what is read back once after the call, in stream order)
        self._last_ig = self._fetch_input_grad(x, weights, input_grad) if input_grad else None
        return (*out, self._fetch_sigma_grad(T + 1, obj[2]) if sigma_grad else None)

    def _train_chunked(self, x, eps, state=None, keep_state=False, weights=None, sigma_grad=False, input_grad=0):
        """Forward + backward of every chunk (see _ChunkedTrainStep): returns the batch loss, the (T+1, 3) ELBO terms of the whole
        batch, d loss / d parameters as one flat buffer in named_parameters() order and, with ``sigma_grad``, sum_e w_e dLL_e/dsigma of
        the batch (else None).  ``state``: a detached initial state, cut along the batch; ``keep_state``: every chunk's LSTM state is
        copied out for ``refinement_state``."""
        dev, B = x.device, x.shape[0]
        ses = self._bind(dev)
        flat = self._flat_out()
        runs, parts, hcs, shared = split(B, self.max_batch(training=True)), [], [], []
        for c, (s, e, share) in enumerate(runs):
            xc = x[s:e].contiguous()
            ec = self._eps(cut(eps, s, e, 1), e - s, dev)
            lc, tc, _, sc = self._train_forward(xc, ec, state and tuple(t[s:e].contiguous() for t in state), cut(weights, s, e),
                                                sigma_grad=sigma_grad, input_grad=input_grad)
            w = torch.full((), share, device=dev, dtype=torch.float32)
            shared.append(scaled(w, lc, sc, *(self._last_ig or (None, None))))       # this chunk's share of the batch mean
            ses.call('iodine_train_backward_flat', ses.stage('t.gl', w), flat, 1 if c else 0)
            hc = self._train_tail(xc, tc, keep_state=keep_state, scalars=c == 0)
            if keep_state:
                hcs.append(hc)
            self.elbo_terms = tc
            parts.append(self._chunk_state())
            ses.call_serial += 1                    # this chunk's saved forward is consumed
        with torch.no_grad():
            self._merge_chunk_state(parts, [w for _, _, w in runs])
            if keep_state:
                self._state = _RefineState(self.posterior.mean, self.posterior.logvar, *merge(hcs, (CAT0, CAT0)))
        loss, sig, *ig = merge(shared, (SUM, SUM, CAT0, CAT0))
        self._last_ig = tuple(ig) if input_grad else None
        return loss, self.elbo_terms, ses.own(flat), sig

    def _train_backward(self, grad_loss, serial, cot, want, BK, index, gf):
        """iodine_train_backward_frames for the saved forward ``serial`` -> (d loss / d parameters as one flat buffer, the four state
        gradients or None each).  ``cot``: the cotangents (mean, mask, mask_logits, z, posterior.mean, posterior.logvar) on the final
        elbo() of an attached forward and (h, c) (B * K, H) on the LSTM state after the last update; ``gf``: the six cotangents
        (F, B, K, ...) on the evaluations ``index`` in the order of ``_FRAME_KEYS``; each a tensor or None, ``grad_loss`` too.  ``want``:
        which of d / d (post_mean, post_logvar, h, c) of the initial state to return.  NULL / 0 for what is not asked for: the library
        then runs the narrower backward - without any of it the plain one -, launch for launch."""
        ses = self._session
        if serial != ses.call_serial:
            raise RuntimeError(self._STALE.format('forward'))
        dev = ses.device
        flat = self._flat_out()
        # (graph mode: the cotangents go through persistent staging buffers like every other tensor, so the graph key repeats)
        stage = lambda names, gs: [None if g is None else ses.stage(n, g.detach().to(device=dev, dtype=torch.float32).contiguous())
                                   for n, g in zip(names, gs)]
        cs = stage(('t.gl', 'a.mean', 'a.mask', 'a.logits', 'a.z', 'a.pm', 'a.plv', 'a.h', 'a.c'), (grad_loss, *cot))
        fs = stage(['f.' + n for n in _FRAME_KEYS], gf)
        outs, gptrs, fptrs, idx, F = (None,) * 4, None, None, None, 0
        if any(want):
            (B, K), L, H = BK, self.dim_latent, int(self._cfg.ref_mlp_units)
            outs = [ses.out('ts.g' + n, shp) if w else None
                    for n, shp, w in zip(('pm', 'plv', 'h', 'c'), ((B, K, L), (B, K, L), (B, K, H), (B, K, H)), want)]
            gptrs = _lib.ptrs(outs)
        if any(t is not None for t in fs):
            F = len(index)
            fptrs, idx = _lib.ptrs(fs), _lib.ints(index)
        ses.call('iodine_train_backward_frames', *cs, flat, 0, gptrs, idx, F, fptrs)
        ses.call_serial += 1                        # the saved forward is consumed (no retain_graph)
        # (graph mode: autograd may keep what we return as .grad; never the staging buffer)
        return ses.own(flat), tuple(ses.own(t) for t in outs)


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
