"""Reference-shaped training / evaluation loops around the HIP module (the callers either side of the hot path,
SURVEY.md section 8f): `lib/engine/train.py:44-108`, `lib/engine/eval.py:14-28`, with one process per GPU instead of
`torch.nn.DataParallel` (`lib/modeling/build.py:11-12`).

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m iodine_amd.engine --steps 200

runs on synthetic blob scenes (there are no datasets on the box); `--clevr DIR` / `--dsprites DIR` read the reference's
dataset layouts through `iodine_amd.data`.
"""
import argparse
import os
import time

import torch

from . import _args, parallel, synth
from .ari import ARIEvaluator
from .checkpoint import load_checkpoint, save_checkpoint
from .optim import FusedAdam, _check_max_norm, clip_grad_norm_, make_optimizer


class SyntheticScenes(torch.utils.data.Dataset):
    """Deterministic blob scenes with ground-truth masks (image index = seed), same item format as lib/data/clevr.py."""

    def __init__(self, n, img_size, seed=0):
        self.n, self.s, self.seed = n, img_size, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        imgs, masks = synth.make_images(1, self.s, seed=self.seed + i, kind='blobs')
        return torch.from_numpy(imgs[0]), torch.from_numpy(masks[0].astype('float32'))


class SyntheticClips(torch.utils.data.Dataset):
    """Clips of ``frames`` frames over ``SyntheticScenes``: frame i is the scene rolled by (i, 2 i) pixels (rows, columns), the masks roll
    with it.  Items: (clip (F, 3, S, S), masks (F, G, S, S))."""

    def __init__(self, n, img_size, frames, seed=0):
        self.scenes, self.frames = SyntheticScenes(n, img_size, seed), int(frames)

    def __len__(self):
        return len(self.scenes)

    def __getitem__(self, i):
        img, masks = self.scenes[i]
        roll = lambda t: torch.stack([torch.roll(t, shifts=(f, 2 * f), dims=(-2, -1)) for f in range(self.frames)])
        return roll(img), roll(masks)


def clip_chunks(F, T):
    """Frame ranges [(0, T+1), (T, 2T+1), ...] of the training forwards that cover a clip of ``F`` frames at ``T`` refinement iterations per
    call: a forward makes T + 1 ELBO evaluations, and the last frame of a chunk is the first of the next (the state is carried across it).
    ValueError unless F = c T + 1 with c >= 1."""
    if isinstance(T, bool) or int(T) != T or T < 1:
        raise ValueError(f'clip_chunks: the iteration count must be an integer >= 1; got {T!r}')
    if isinstance(F, bool) or int(F) != F or F < T + 1 or (F - 1) % T != 0:
        raise ValueError(f'clip_chunks: a clip trained in chunks of n_iters = {T} iterations has c * {T} + 1 frames with c >= 1 '
                         f'({T + 1}, {2 * T + 1}, ...); got {F!r}')
    return [(c * T, c * T + T + 1) for c in range((int(F) - 1) // int(T))]


def clip_weights(weights, clip_shape, chunk):
    """The per-pixel weights of chunk ``chunk`` = (first frame, one past the last) of a clip of shape ``clip_shape`` (B, F, C, S, S):
    ``weights`` (B, F, 1, S, S) / (B, F, S, S) - one weight image per frame - cut to the chunk's frames, the boundary frame included like
    in the clip itself; (B, 1, S, S) / (B, S, S) - the same weights for every frame - as they are; None -> None.  Host only."""
    if weights is None:
        return None
    if not torch.is_tensor(weights):
        raise ValueError(f'clip_backward: weights must be a tensor or None; got {type(weights).__name__}')
    B, F, S = clip_shape[0], clip_shape[1], clip_shape[-1]
    got = tuple(weights.shape)
    if got in ((B, 1, S, S), (B, S, S)):
        return weights
    if got in ((B, F, 1, S, S), (B, F, S, S)):
        return weights[:, chunk[0]:chunk[1]]
    raise ValueError(f'clip_backward: weights must have shape ({B}, {F}, 1, {S}, {S}) / ({B}, {F}, {S}, {S}), one weight image per frame of '
                     f'the clip {tuple(clip_shape)}, or ({B}, 1, {S}, {S}) / ({B}, {S}, {S}) for every frame; got {got}')


def border_weights(B, S, n, device=None):
    """Weights (B, 1, S, S) that take an ``n``-pixel frame around every image out of the objective (``--ignore-border``): 0 there, 1
    inside."""
    if isinstance(n, bool) or int(n) != n or not 0 <= n or 2 * n >= S:
        raise ValueError(f'border_weights: the border must be an integer with 0 <= 2 n < {S} (something must stay observed); got {n!r}')
    w = torch.zeros((B, 1, S, S), dtype=torch.float32, device=device)
    w[:, :, n:S - n, n:S - n] = 1.0
    return w


def clip_backward(model, clip, eps=None, bptt='truncated', weights=None, frame_loss=None):
    """Gradient of one clip (B, F, 3, S, S), F = c * n_iters + 1, accumulated into ``.grad`` chunk by chunk (``clip_chunks``); the caller
    zeroes the gradients before and steps the optimizer after.  Returns (clip loss, (F, 3) ELBO terms, one row per frame).

    Chunk c is a training forward over frames [cT, cT + T] from the state chunk c - 1 left, with ``eps[cT : cT + T + 1]`` of ``eps``
    (F, B, K, L) (None: drawn once for the whole clip from the model's generator).  The boundary frame was scored as the last evaluation of
    the chunk before, so chunks after the first run with evaluation-0 weight 0: ``model.iter_weights`` is set per chunk and restored
    afterwards.  The clip's loss is therefore that of ONE forward over all F frames with the weights (w_0, .., w_T, w_1, .., w_T, ...).

    ``bptt='truncated'``: one forward and one backward per chunk, the state carried detached - no gradient crosses a chunk boundary.
    ``bptt='exact'``: the gradient of that one long forward, at the memory of one chunk.  Pass 1 runs the training forwards under
    ``no_grad`` and keeps every chunk's entry state; pass 2 walks the chunks in reverse, runs each forward again from its entry state (the
    same bits) and back-propagates loss + <cotangents of the following chunk, (lambda_T, h_T, c_T)>; the gradient of the entry state is the
    cotangent handed to the chunk before.  About two forwards and one backward per chunk.

    ``weights``: per-pixel observation weights of the clip (``IODINE.forward``): (B, F, 1, S, S) / (B, F, S, S), one weight image per frame -
    every chunk, and every re-run of a chunk in the exact mode, gets the slice of its frames (``clip_weights``) - or (B, 1, S, S) /
    (B, S, S) for all frames.

    ``frame_loss``: per-frame auxiliary terms.  ``frame_loss(f, t)`` gets the clip frame index ``f`` and a dict of what the evaluation that
    scores frame ``f`` decoded - ``z``, ``post_mean``, ``post_logvar`` (B, K, L), ``mean`` (B, K, 3, S, S), ``mask``, ``mask_logits``
    (B, K, 1, S, S), attached (``IODINE.forward(attach_frames=...)``) - and returns a scalar tensor or None.  Every frame is scored exactly
    once, where its ELBO weight sits: chunk 0 attaches evaluations 0..T, later chunks 1..T.  The terms join the chunk's loss in its one
    ``backward()``; in the exact mode they are added in pass 2 only and their gradient crosses the chunk boundaries through the same
    cotangent hand-over as the loss's.  The call then returns (clip loss, ELBO terms, the detached sum of the terms)."""
    if bptt not in ('truncated', 'exact'):
        raise ValueError(f"clip_backward: bptt must be 'truncated' or 'exact'; got {bptt!r}")
    if clip.dim() != 5:
        raise ValueError(f'clip_backward: expected a clip (B, F, 3, S, S); got {tuple(clip.shape)}')
    K, T = _args.run_shape(model.K, model.n_iters)
    chunks = clip_chunks(clip.shape[1], T)
    B, F = clip.shape[0], clip.shape[1]
    saved = model.iter_weights
    w = _args.read_objective(model.sigma, model.beta, model.iter_weights, T)[2] or tuple((i + 1) / (T + 1) for i in range(T + 1))
    later = (0.0,) + tuple(w[1:])
    if len(chunks) > 1 and not any(torch.tensor(later, dtype=torch.float32).tolist()):
        raise ValueError(f'clip_backward: model.iter_weights = {saved!r} puts all weight on evaluation 0, which chunks after the first do not '
                         f'score (their first frame is the last one of the chunk before): they would carry no loss')
    shape = (F, B, K, model.dim_latent)
    if eps is None:
        eps = model._normals(None, shape, clip.device).clone()
    elif tuple(eps.shape) != shape:
        raise RuntimeError(f'clip_backward: eps must have shape {shape}, one slice per frame; got {tuple(eps.shape)}')
    clip_weights(weights, clip.shape, chunks[0])                             # (a wrong shape is refused before any device work)
    part = lambda c: (clip[:, chunks[c][0]:chunks[c][1]], eps[chunks[c][0]:chunks[c][1]])
    wpart = lambda c: clip_weights(weights, clip.shape, chunks[c])
    total, terms = None, [None] * len(chunks)
    aux_total = None
    attach = lambda c: None if frame_loss is None else tuple(range(0 if c == 0 else 1, T + 1))

    def scored(c, out):
        # out + the terms of the frames chunk c scores
        nonlocal aux_total
        if frame_loss is None:
            return out
        fr = model.frames
        for j, i in enumerate(fr['index']):
            term = frame_loss(chunks[c][0] + i, {k: fr[k][j] for k in ('z', 'mean', 'mask', 'mask_logits', 'post_mean', 'post_logvar')})
            if term is not None:
                out = out + term
                aux_total = term.detach() if aux_total is None else aux_total + term.detach()
        return out

    try:
        if bptt == 'truncated':
            state = None
            for c in range(len(chunks)):
                model.iter_weights = saved if c == 0 else later
                loss = model(*part(c), state=state, keep_state=True, weights=wpart(c), attach_frames=attach(c))
                scored(c, loss).backward()
                state = model.refinement_state()
                total = loss.detach() if total is None else total + loss.detach()
                terms[c] = model.elbo_terms if c == 0 else model.elbo_terms[1:]
        else:
            entry = [None]
            with torch.no_grad():                                            # pass 1: the entry state of every chunk
                for c in range(len(chunks) - 1):
                    model.iter_weights = saved if c == 0 else later
                    model(*part(c), state=entry[c], keep_state=True, weights=wpart(c))
                    entry.append(model.refinement_state())
            cot = None
            for c in reversed(range(len(chunks))):                           # pass 2: recompute, back-propagate, hand the cotangents on
                model.iter_weights = saved if c == 0 else later
                leaves = None if c == 0 else tuple(t.clone().requires_grad_(True) for t in entry[c])
                loss = model(*part(c), state=leaves, attach_state=True, weights=wpart(c), attach_frames=attach(c))
                out = scored(c, loss)
                if cot is not None:
                    ends = (model.posterior.mean, model.posterior.logvar) + tuple(t.view_as(cot[2]) for t in model.lstm_hidden)
                    out = out + sum((g * t).sum() for g, t in zip(cot, ends) if g is not None)
                out.backward()
                cot = None if leaves is None else tuple(t.grad for t in leaves)
                total = loss.detach() if total is None else total + loss.detach()
                terms[c] = model.elbo_terms if c == 0 else model.elbo_terms[1:]
    finally:
        model.iter_weights = saved
    if frame_loss is not None:
        return total, torch.cat(terms, 0), aux_total if aux_total is not None else torch.zeros((), device=clip.device)
    return total, torch.cat(terms, 0)


def beta_warmup(step, beta, warmup_steps):
    """KL weight of training step ``step`` (counted from 0) under ``--beta-warmup``: a linear ramp from 0 at step 0 to ``beta`` at step
    ``warmup_steps``, ``beta`` from there on; ``warmup_steps`` <= 0: ``beta`` throughout."""
    if warmup_steps <= 0 or step >= warmup_steps:
        return float(beta)
    return float(beta) * step / warmup_steps


def train(model, optimizer, dataloader, device, max_steps, print_every=10, checkpoint_path=None, log=print, max_grad_norm=None,
          beta=None, beta_warmup_steps=0, bptt=None, ignore_border=0, log_sigma=None, input_gain=None,
          mask_loss=0.0, mask_loss_kind='ce', mask_match='iou', sheet_every=0, sheet_path=None, sheet_images=8, sheet_scale=1):
    """train.py:44-108: loss = model(data); loss.mean(); zero_grad; backward; [all-reduce]; [clip]; step.  Returns the losses.
    ``dataloader``: a ``DataLoader`` (``make_dataloader``) or ``ResidentDataset.batches(...)`` (``iodine_amd.resident``), whose batches
    ``(x, gt, n_gt)`` are already on the device - ``gt`` packed ``(B, G, S, S)``, which ``pack_gt`` passes through - and whose epoch is set
    like a ``DistributedSampler``'s.
    ``max_grad_norm``: the global gradient norm is clipped at this value (train.py:64, commented out in the reference; the paper
    uses 5.0) AFTER the all-reduce, so every rank clips the same averaged gradient with the same coefficient - what
    ``clip_grad_norm_`` after DataParallel's reduce would do - and the replicas stay bitwise identical.  A ``FusedAdam`` takes it
    as its ``max_grad_norm`` (fused into the step, kept on the optimizer afterwards); in front of any other optimizer
    ``iodine_amd.optim.clip_grad_norm_`` runs.  The log line gains ``grad-norm`` (one ``.item()`` per ``print_every`` steps).
    ``beta`` / ``beta_warmup_steps``: with ``beta`` given, ``model.beta`` is set before every step to ``beta_warmup(step, beta,
    beta_warmup_steps)`` and is left at ``beta`` afterwards; None leaves ``model.beta`` alone.
    ``bptt``: 'truncated' or 'exact' - the loader yields clips (B, F, 3, S, S) with F = c * n_iters + 1 frames (``SyntheticClips``) and a step
    is ``clip_backward`` over the clip's chunks: ONE optimizer step per clip, the all-reduce and the clipping after the last chunk.
    ``ignore_border``: n > 0 trains with zero observation weight on an n-pixel frame around every image (``border_weights``, the
    ``weights=`` of ``IODINE.forward``).
    ``log_sigma``: a learned observation scale (``--learn-sigma``) - a float32 device scalar that requires grad and sits in a param group of
    ``optimizer``, kept outside the module (whose ``state_dict`` names are the reference's): ``model.sigma = log_sigma.exp()`` before
    every step, so ``loss.backward()`` fills ``log_sigma.grad``; the log line gains ``sigma``, the checkpoint an entry ``log_sigma``, and
    ``model.sigma`` is left at the learned value as a plain float.  Every step then costs one ``.item()`` and runs eagerly in graph mode.
    Its gradient is part of the global norm that ``max_grad_norm`` clips, with the fused optimizer (which takes the norm over all its param
    groups) and in front of any other alike.
    ``input_gain``: a learned front end (``--learn-input-gain``, ``InputGain``) whose parameters sit in a param group of ``optimizer``: the
    batch goes through it before the model, so ``loss.backward()`` reaches its parameters through ``x.grad`` - the gradient the model returns
    for an image that requires grad.  Its gradients join the all-reduce and the clipped global norm; the checkpoint gains the entry
    ``input_gain`` (its ``state_dict``).  Not combined with ``bptt``.
    ``mask_loss`` = w > 0: supervised masks.  A step is ``model(x, attach_state=True)`` plus ``w * matched_mask_loss(model.mask,
    pack_gt(data[1]), loss=mask_loss_kind, match=mask_match)`` (``iodine_amd.matching``: ground-truth objects assigned to slots on the device,
    three launches, no synchronise) and one ``backward()``; the log line gains ``mask-loss``.  A batch whose masks are all ``None`` / empty
    trains unsupervised - the semi-supervised case.  Not combined with ``bptt``.  With 0 (default) no launch, copy or attribute is added.
    ``sheet_every`` = n > 0 with ``sheet_path`` = ``OUT.png``: after every n-th optimizer step the decomposition sheet of the first
    ``sheet_images`` images of the current batch is written to ``OUT_<step:07d>.png`` (``save_sheet``; rank 0 only).  Its reconstruct draws
    its normals from a Philox stream training never uses, so the sequence of losses is bit-identical with and without it; with 0 (default)
    nothing is launched or copied."""
    sheet_every = int(sheet_every or 0)
    if sheet_every < 0 or (sheet_every and not sheet_path):
        raise ValueError(f'train: sheet_every must be >= 0 and needs sheet_path; got {sheet_every!r}, {sheet_path!r}')
    sheet_rank0 = not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0
    if input_gain is not None and bptt is not None:
        raise ValueError('train: input_gain is not combined with bptt (clip_backward differentiates its chunks itself)')
    mask_loss = float(mask_loss)
    if mask_loss < 0.0 or mask_loss != mask_loss:
        raise ValueError(f'train: mask_loss must be >= 0; got {mask_loss!r}')
    if mask_loss > 0.0:
        if bptt is not None:
            raise ValueError('train: mask_loss is not combined with bptt (clip_backward differentiates its chunks itself; use its frame_loss)')
        from . import matching
        matching._kind(mask_loss_kind, 'train: mask_loss_kind'), matching._kind(mask_match, 'train: mask_match')
    mask_term = None
    extra_params = ([log_sigma] if log_sigma is not None else []) + (list(input_gain.parameters()) if input_gain is not None else [])
    model.train()
    fused_clip = isinstance(optimizer, FusedAdam)
    if max_grad_norm is not None:
        max_grad_norm = _check_max_norm(max_grad_norm, 'max_grad_norm')
        if fused_clip:
            optimizer.max_grad_norm = max_grad_norm
    clipping = max_grad_norm is not None or (fused_clip and optimizer.max_grad_norm is not None)
    world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    losses, step, epoch = [], 0, 0
    while step < max_steps:
        sampler = getattr(dataloader, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)                                         # a new shuffle per pass over the data
        epoch += 1
        for data in dataloader:
            start = time.perf_counter()
            x = data[0].to(device, non_blocking=True)                        # "first one is image" (train.py:49)
            if beta is not None:
                model.beta = beta_warmup(step, beta, beta_warmup_steps)
            if log_sigma is not None:
                model.sigma = log_sigma.exp()
            if input_gain is not None:
                x = input_gain(x)
            w = border_weights(x.shape[0], x.shape[-1], ignore_border, device) if ignore_border else None
            if bptt is not None:
                optimizer.zero_grad()
                loss, _ = clip_backward(model, x, bptt=bptt, weights=w)
            elif mask_loss > 0.0 and _has_masks(data):
                loss = (model(x, attach_state=True) if w is None else model(x, weights=w, attach_state=True)).mean()
                gt = matching.pack_gt(data[1], x.shape[-1], device)
                mask_term = matching.matched_mask_loss(model.mask, gt, loss=mask_loss_kind, match=mask_match)
                optimizer.zero_grad()
                (loss + mask_loss * mask_term).backward()
                mask_term = mask_term.detach()
            else:
                loss = (model(x) if w is None else model(x, weights=w)).mean()
                optimizer.zero_grad()
                loss.backward()
                mask_term = None
            if world > 1:
                parallel.allreduce_gradients(list(model.parameters()) + extra_params)   # replaces DataParallel's reduce
            if clipping and not fused_clip:
                grad_norm = clip_grad_norm_(list(model.parameters()) + extra_params, max_grad_norm)
            optimizer.step()
            if clipping and fused_clip:
                grad_norm = optimizer.last_grad_norm
            losses.append(loss.item())
            step += 1
            if sheet_every and step % sheet_every == 0 and sheet_rank0:
                root, ext = os.path.splitext(sheet_path)
                save_sheet(model, data, '{}_{:07d}{}'.format(root, step, ext or '.png'), device, images=sheet_images, scale=sheet_scale,
                           draw=step, log=lambda *a: None)
                model.train()
            if step % print_every == 0:
                log('iter: {}, loss: {:.4f}, batch-time: {:.4f}s, lr: {}{}{}{}'.format(
                    step, losses[-1], time.perf_counter() - start, optimizer.param_groups[0]['lr'],
                    ', grad-norm: {:.4f}'.format(grad_norm.item()) if clipping else '',
                    ', sigma: {:.5f}'.format(log_sigma.detach().exp().item()) if log_sigma is not None else '',
                    ', mask-loss: {:.4f}'.format(mask_term.item() if mask_term is not None else 0.0) if mask_loss > 0.0 else ''))
            if step >= max_steps:
                break
    if beta is not None:
        model.beta = float(beta)
    extra = {}
    if log_sigma is not None:
        model.sigma = float(log_sigma.detach().exp().item())
        extra['log_sigma'] = log_sigma.detach().cpu()
    if input_gain is not None:
        extra['input_gain'] = {k: v.detach().cpu() for k, v in input_gain.state_dict().items()}
    if checkpoint_path and (not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0):
        save_checkpoint(checkpoint_path, model, optimizer, epoch=0, iteration=step, **extra)
    return losses


def _has_masks(data):
    """whether a batch (image, masks) carries at least one ground-truth mask"""
    if len(data) < 2 or data[1] is None:
        return False
    if torch.is_tensor(data[1]):
        return data[1].numel() > 0
    return any(m is not None and len(m) > 0 for m in data[1])


def add_sigma_group(optimizer, log_sigma, lr):
    """``log_sigma`` as a param group of its own, behind the model's (the layout ``resume`` expects)"""
    optimizer.add_param_group({'params': [log_sigma], 'lr': lr, 'weight_decay': 0.0})


def resume(path, model, optimizer, log_sigma=None, lr=3e-4):
    """``load_checkpoint`` for a run with or without ``--learn-sigma``; the file is read once.  A checkpoint written with ``--learn-sigma``
    holds the entry ``log_sigma`` and, in its optimizer state, the param group of that scalar: ``log_sigma`` joins ``optimizer`` before the
    state loads and takes the saved value.  An older checkpoint has neither: the state loads into the model's groups and a fresh group is added
    behind them.  Such a checkpoint resumed WITHOUT a ``log_sigma`` is refused in words - its optimizer state would not fit, and dropping the
    learned scale silently would train on at another sigma.  Returns the extra entries (epoch, iteration, ...)."""
    ckpt = torch.load(path, map_location=torch.device('cpu'))
    saved = 'log_sigma' in ckpt
    if saved and log_sigma is None:
        raise ValueError(f'{path} was written with --learn-sigma: it holds a learned log_sigma = {float(ckpt["log_sigma"]):.5f} (sigma '
                         f'{float(ckpt["log_sigma"].exp()):.5f}) and the optimizer state of its param group - resume it with --learn-sigma')
    if saved:
        add_sigma_group(optimizer, log_sigma, lr)
    extra = load_checkpoint(ckpt, model, optimizer)
    if saved:
        with torch.no_grad():
            log_sigma.copy_(extra['log_sigma'].to(log_sigma.device))
    elif log_sigma is not None:
        add_sigma_group(optimizer, log_sigma, lr)
    return extra


class InputGain(torch.nn.Module):
    """The front end of ``--learn-input-gain``: a per-channel gain and offset in front of the model, six parameters, the identity at the
    start.  It is trained through the gradient the model returns for an image that requires grad (``x.grad``), by the same optimiser step -
    the smallest front end that shows that gradient arriving (``main`` evaluates on the raw images afterwards: the six parameters belong to
    the training loop, the checkpoint entry ``input_gain`` carries them).  ``x``: images (B, 3, S, S) or a clip (B, E, 3, S, S)."""

    def __init__(self, device, channels=3):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.ones(channels, device=device))
        self.offset = torch.nn.Parameter(torch.zeros(channels, device=device))

    def forward(self, x):
        return x * self.gain.view(-1, 1, 1) + self.offset.view(-1, 1, 1)


def make_log_sigma(sigma, device):
    """The parameter of ``--learn-sigma``: log(sigma) as a float32 scalar on ``device`` that requires grad"""
    import math
    return torch.full((), math.log(float(sigma)), dtype=torch.float32, device=device, requires_grad=True)


def evaluate(model, dataloader, device, evaluator=None, slots=None, iters=None, bound_samples=0, restarts=0, min_component_area=0,
             adaptive=None):
    """eval.py:14-28 with the ARI evaluator of lib/eval/ari_eval.py (works under no_grad, unlike the reference).  With
    several ranks every rank evaluates its shard; the samples DistributedSampler appended to pad the shards to equal length
    are dropped (they duplicate the first images) and ``evaluator.global_mean`` holds the ARI over the whole dataset.
    ``slots`` / ``iters``: evaluate at that K / T (``model.K`` / ``model.n_iters`` for the duration of the call, restored afterwards;
    e.g. weights trained at K = 7, T = 5 evaluated at K = 11) - the ARI tables take K from the masks.
    ``bound_samples`` = S > 0: after each batch's ``reconstruct`` one ``model.predictive(x, samples=S)`` from the posterior it left; the
    dataset means of the S-sample importance-weighted bound and of the S-sample Monte-Carlo ELBO (per image, nats) are left in
    ``evaluator.iwae`` / ``evaluator.elbo_mc`` (over all ranks, like ``global_mean``).  0 (default): no launch is added and neither
    attribute is set.
    ``restarts`` = C > 1: every batch is refined C times (``model.restarts(x, chains=C)``) and the evaluators, which keep calling
    ``model.reconstruct``, get the best chain's decode per image through a thin proxy; ``evaluator.stability``, ``evaluator.best_score`` and
    ``evaluator.first_score`` are the dataset means (over all ranks) of ``Restarts.stability``, of the best chain's score and of chain 0's -
    what selecting gains, next to the metric.  ``bound_samples`` then samples around the chosen posterior.  0 or 1 (default): the path and
    the bits of an evaluation without it, and none of the three attributes.
    ``min_component_area`` = N > 0: beside the evaluator's own scores, the argmax map of every decode is split into connected components
    (``iodine_amd.objects.components``) and ``evaluator.cleaned`` holds the dataset means (over all ranks) of ``components_per_slot`` (per
    non-empty slot), ``small_pixel_share`` (valid pixels in components below N) and of ``SegmentationEvaluator``'s ``aris / mious / scs /
    mscs`` on the maps with those components absorbed.  0 (default): no launch is added, no attribute is set.
    ``adaptive`` = dict(tol=, rtol=, max_iters=, min_iters=, check_every=) (any subset that names a tolerance): the evaluators get the decodes
    of ``model.reconstruct_adaptive(x, **adaptive)`` - every image refined until its ELBO estimate stops improving - and
    ``evaluator.adaptive`` holds, over all ranks, ``mean_iters``, ``hist`` (images per iteration count, index 0 .. max_iters), ``at_max``
    (the share of images that ran to max_iters) and ``max_iters``.  Not together with ``restarts``.  None (default): the usual path."""
    if isinstance(bound_samples, bool) or int(bound_samples) != bound_samples or bound_samples < 0:
        raise ValueError(f'evaluate: bound_samples must be an integer >= 0; got {bound_samples!r}')
    if isinstance(restarts, bool) or int(restarts) != restarts or restarts < 0:
        raise ValueError(f'evaluate: restarts must be an integer >= 0; got {restarts!r}')
    if isinstance(min_component_area, bool) or int(min_component_area) != min_component_area or min_component_area < 0:
        raise ValueError(f'evaluate: min_component_area must be an integer >= 0; got {min_component_area!r}')
    if adaptive is not None:
        if not isinstance(adaptive, dict) or set(adaptive) - {'tol', 'rtol', 'max_iters', 'min_iters', 'check_every'}:
            raise ValueError(f'evaluate: adaptive must be a dict of tol, rtol, max_iters, min_iters, check_every; got {adaptive!r}')
        if restarts > 1:
            raise ValueError('evaluate: adaptive= and restarts= do not combine (every chain of a restart runs the fixed iteration count)')
    saved = (model.K, model.n_iters)
    if slots is not None:
        model.K = slots
    if iters is not None:
        model.n_iters = iters
    try:
        return _evaluate(model, dataloader, device, evaluator, int(bound_samples), int(restarts), int(min_component_area), adaptive)
    finally:
        model.K, model.n_iters = saved


class _BestOfRestarts:
    """What ``evaluate(restarts=C)`` hands the evaluators in place of the model: ``reconstruct(x)`` runs ``model.restarts(x, chains=C)`` and
    returns the best chain's decode per image; everything else is the model's.  ``rows``: per image (stability, best score, chain 0's)."""

    def __init__(self, model, chains):
        self._model, self._chains, self.rows = model, chains, []

    def __getattr__(self, name):
        return getattr(self._model, name)

    def reconstruct(self, x):
        res = self._model.restarts(x, chains=self._chains)
        best = res.score.gather(0, res.best.view(1, -1))[0]
        self.rows.extend(zip(res.stability.tolist(), best.tolist(), res.score[0].tolist()))
        return res.pred, res.mask, res.mean


class _AdaptiveDecodes:
    """What ``evaluate(adaptive=...)`` hands the evaluators in place of the model: ``reconstruct(x)`` runs ``model.reconstruct_adaptive(x,
    **options)`` and returns its decode; everything else is the model's.  ``iters``: per image, the updates it received."""

    def __init__(self, model, options):
        self._model, self._options, self.iters, self.max_iters = model, dict(options), [], 0

    def __getattr__(self, name):
        return getattr(self._model, name)

    def reconstruct(self, x):
        res = self._model.reconstruct_adaptive(x, **self._options)
        self.iters.extend(res.iters.tolist())
        self.max_iters = int(res.ll.shape[0])
        return res.pred, res.mask, res.mean


class _CleanedMaps:
    """What ``evaluate(min_component_area=N)`` hands the evaluators in place of the model (or of ``_BestOfRestarts``): ``reconstruct(x)`` is
    the wrapped one, and beside it the argmax map of the returned masks goes through ``objects.components(min_area=N, clean=True)`` - the
    map is taken from the masks, so the best chain of a restart is read like a plain decode.  ``component_rows``: per image (components
    per non-empty slot, share of the valid pixels in small components); ``replay.reconstruct(x)`` returns the same decode with the cleaned
    map as a hard mask, for a second evaluator on the same batch."""

    def __init__(self, inner, min_area):
        self._inner, self._min_area, self.component_rows, self._last = inner, min_area, [], None
        self.replay = self._Replay(self)

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def reconstruct(self, x):
        from .objects import components, seg_to_mask, slot_table
        pred, mask, mean = self._inner.reconstruct(x)
        K, P = int(mask.shape[-4]), int(mask.shape[-1]) ** 2
        comp = components(slot_table(mask, segmentation=True)[1], K, min_area=self._min_area, max_components=0, clean=True)
        per_slot, count = comp.per_slot.cpu().double(), comp.count.cpu().double()
        n = per_slot[..., 0] + per_slot[..., 1]                               # components of every slot
        self.component_rows.extend(zip((n.sum(-1) / (n > 0).sum(-1).clamp_min(1)).tolist(),
                                       (count[:, 2] / (P - count[:, 3]).clamp_min(1)).tolist()))
        self._last = (pred, seg_to_mask(comp.clean, K), mean)
        return pred, mask, mean

    class _Replay:
        def __init__(self, owner):
            self._owner = owner

        def reconstruct(self, x):
            return self._owner._last


def _evaluate(model, dataloader, device, evaluator, bound_samples=0, restarts=0, min_component_area=0, adaptive=None):
    evaluator = evaluator or ARIEvaluator()
    evaluator.reset()
    bounds = []                                                              # per image: (iwae, elbo_mc)
    model.eval()
    scored = _BestOfRestarts(model, restarts) if restarts > 1 else model     # (what the evaluators call reconstruct on)
    adapted = scored = _AdaptiveDecodes(model, adaptive) if adaptive is not None else scored
    cleaned = None
    if min_component_area:
        from .matching import SegmentationEvaluator
        scored, cleaned = _CleanedMaps(scored, min_component_area), SegmentationEvaluator()
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    world = torch.distributed.get_world_size() if dist_on else 1
    rank = torch.distributed.get_rank() if dist_on else 0
    n_total = len(dataloader.dataset)
    mine = len(range(rank, n_total, world)) if world > 1 else n_total       # un-padded share of this rank (sampler stride = world)
    with torch.no_grad():
        for data in dataloader:
            image, masks = data[0], data[1]
            if torch.is_tensor(masks):                                       # a ResidentDataset batch: packed on the device, with counts
                batch = (image.to(device), masks, data[2])
            else:
                batch = (image.to(device), [m.numpy() for m in masks])
            evaluator.evaluate(scored, batch)
            if cleaned is not None:                                          # the same decode, its map cleaned
                cleaned.evaluate(scored.replay, batch)
            if bound_samples:
                out = model.predictive(image.to(device), samples=bound_samples)
                bounds.extend(zip(out.iwae.tolist(), out.elbo_mc.tolist()))
    lists = tuple(getattr(evaluator, 'per_image', ('aris',)))                # every per-image list the evaluator declares
    for name in lists:
        del getattr(evaluator, name)[mine:]
    if bound_samples:
        del bounds[mine:]
        tot = torch.tensor([sum(q[0] for q in bounds), sum(q[1] for q in bounds), float(len(bounds))], dtype=torch.float64,
                           device=device if dist_on and torch.distributed.get_backend() == 'nccl' else 'cpu')
        if world > 1:
            torch.distributed.all_reduce(tot)
        n = max(float(tot[2]), 1.0)
        evaluator.iwae, evaluator.elbo_mc = float(tot[0]) / n, float(tot[1]) / n
    if restarts > 1:
        rows = scored.rows[:mine]
        tot = torch.tensor([sum(q[i] for q in rows) for i in range(3)] + [float(len(rows))], dtype=torch.float64,
                           device=device if dist_on and torch.distributed.get_backend() == 'nccl' else 'cpu')
        if world > 1:
            torch.distributed.all_reduce(tot)
        n = max(float(tot[3]), 1.0)
        evaluator.stability, evaluator.best_score, evaluator.first_score = (float(tot[i]) / n for i in range(3))
    if adaptive is not None:                                                 # images per iteration count, over all ranks
        M = adapted.max_iters
        hist = torch.zeros(M + 1, dtype=torch.float64, device=device if dist_on and torch.distributed.get_backend() == 'nccl' else 'cpu')
        for t in adapted.iters[:mine]:
            hist[t] += 1
        if world > 1:
            torch.distributed.all_reduce(hist)
        n = max(float(hist.sum()), 1.0)
        evaluator.adaptive = dict(mean_iters=float((hist * torch.arange(M + 1, dtype=torch.float64, device=hist.device)).sum()) / n,
                                  hist=[int(v) for v in hist.tolist()], at_max=float(hist[M]) / n, max_iters=M)
    stats = torch.tensor([float(sum(evaluator.aris)), float(len(evaluator.aris))], dtype=torch.float64,
                         device=device if dist_on and torch.distributed.get_backend() == 'nccl' else 'cpu')
    if world > 1:
        torch.distributed.all_reduce(stats)
    evaluator.global_mean = float(stats[0] / stats[1]) if float(stats[1]) > 0 else 0.0
    if lists != ('aris',):                                                   # means of the other lists over all ranks; NaN = no score
        kept = [[v for v in getattr(evaluator, name) if v == v] for name in lists]
        more = torch.tensor([[float(sum(v)), float(len(v))] for v in kept], dtype=torch.float64, device=stats.device)
        if world > 1:
            torch.distributed.all_reduce(more)
        evaluator.global_means = {name: (float(s / c) if float(c) > 0 else 0.0) for name, (s, c) in zip(lists, more)}
        evaluator.global_means['aris'] = evaluator.global_mean
    if cleaned is not None:                                                  # the same reductions over the cleaned maps' lists and the rows
        rows = scored.component_rows[:mine]
        cols = [[q[0] for q in rows], [q[1] for q in rows]] + [[v for v in getattr(cleaned, name)[:mine] if v == v] for name in cleaned.per_image]
        tot = torch.tensor([[float(sum(v)), float(len(v))] for v in cols], dtype=torch.float64, device=stats.device)
        if world > 1:
            torch.distributed.all_reduce(tot)
        names = ('components_per_slot', 'small_pixel_share') + tuple(cleaned.per_image)
        evaluator.cleaned = {name: (float(s / c) if float(c) > 0 else 0.0) for name, (s, c) in zip(names, tot)}
    return evaluator


@torch.no_grad()
def save_traversal(model, x, path, top=8, n_values=7, log=print):
    """The disentanglement figure of image 0 of ``x``: reconstruct the batch, rank each slot's latent units by KL, move the ``top`` of them
    one at a time along the posterior (``mu + v sigma``, ``n_values`` values of v in [-2, 2]) and save ``grids (K, 3, top S, n_values S)`` -
    rows are units, columns values -, ``dims (K, top)``, ``values`` and ``kl (K, L)`` as an .npz.  One ``IODINE.edit`` call behind
    ``iodine_amd.traverse.traverse``: the scene is decoded once, every variation decodes one slot-image."""
    import numpy as np

    from .traverse import latent_kl, traverse
    model.eval()
    model.reconstruct(x)
    post = (model.posterior.mean, model.posterior.logvar)
    t = traverse(model, model.z, image=0, posterior=post, top=top, values=torch.linspace(-2.0, 2.0, n_values), mode='sigma')
    grids = torch.stack([t.grid(i) for i in range(len(t.slots))])
    np.savez(path, grids=grids.cpu().numpy(), dims=t.dims.numpy(), values=t.values.numpy(), kl=latent_kl(post[0][0], post[1][0]).cpu().numpy())
    log(f'traversal of image 0: {len(t.slots)} slots x {t.dims.shape[1]} units x {n_values} values -> {path}')
    return t


SHEET_STREAM = 1 << 63      # Philox stream ids of the sheets' normals: training counts its draws up from 0 and never gets here


@torch.no_grad()
def save_sheet(model, data, path, device, images=8, scale=1, trajectory=None, draw=0, log=print):
    """The decomposition sheet (``iodine_amd.figures.decomposition``) of the first ``images`` images of a batch - a ``DataLoader`` batch
    ``(image, masks)`` or a ``ResidentDataset`` batch ``(x, gt, n_gt)``; of a clip, frame 0 - as a PNG: image, reconstruction,
    segmentation and the slots, with the ``gt`` panel and matched colours when the batch carries masks.  ``trajectory=b``: the refinement
    figure of image b instead, one row per decode.  The normals come from ``iodine_randn(model seed, SHEET_STREAM + draw)`` and are passed
    as an explicit ``eps``, so the model's own stream of draws - and with it a training run around this call - is untouched."""
    from . import _lib, figures
    x = data[0].to(device)
    if x.dim() == 5:
        x = x[:, 0]
    n = 1 if trajectory is not None else max(1, min(int(images), int(x.shape[0])))
    eps = torch.empty((model.n_iters + 1, n, model.K, model.dim_latent), dtype=torch.float32, device=device)
    _lib.call('iodine_randn', device, eps, eps.numel(), model._seed, (SHEET_STREAM + int(draw)) & (2 ** 64 - 1))
    gt = data[1] if _has_masks(data) and x.dim() == 4 and data[0].dim() == 4 else None
    model.eval()
    out = figures.decomposition(model, x, gt=gt, n=n, trajectory=trajectory, eps=eps, scale=scale)
    figures.write_png(path, out)
    log('sheet: {} x {} pixels, {} -> {}'.format(out.shape[0], out.shape[1],
        'refinement of image {}'.format(trajectory) if trajectory is not None else '{} images'.format(n), path))
    return out


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', choices=['clevr6', 'dsprites'], default='dsprites')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--batch', type=int, default=8, help='images per GPU')
    ap.add_argument('--lr', type=float, default=3e-4)                        # configs/clevr6_prop.yaml:19
    ap.add_argument('--clip', type=float, default=None, metavar='FLOAT',
                    help='clip the global gradient norm at this value (train.py:64; the paper uses 5.0)')
    ap.add_argument('--clevr'); ap.add_argument('--dsprites')
    ap.add_argument('--resume'); ap.add_argument('--save')
    ap.add_argument('--conv-precision', type=int, choices=[0, 1, 2], default=1,
                    help='3x3 convs of the tuned decoder and refinement stacks: 0 = exact fp32 MFMA, 1 = split-fp16 (3 x f16 MFMA, fp32-class '
                         'accuracy; default), 2 = as 1 with the weight-stationary decoder convs on ONE fp16 MFMA per product (fp16-class: '
                         'meant for evaluation - --resume with --eval-samples / --traverse; training runs, outside the 1e-3 gradient budget)')
    ap.add_argument('--gen-conv-precision', type=int, choices=[0, 1], default=0,
                    help='generic decoder convs C -> C (KERNEL_SIZE 5 / 7, other channel counts): 0 = exact fp32 MFMA, '
                         '1 = split-fp16 (3 x f16 MFMA, fp32-class accuracy) forward and data gradient')
    ap.add_argument('--sigma', type=float, default=None, metavar='FLOAT',
                    help='likelihood scale (model.sigma); default: ARCH.SIGMA of the config')
    ap.add_argument('--beta', type=float, default=1.0, metavar='FLOAT', help='weight of the KL term (model.beta)')
    ap.add_argument('--beta-warmup', type=int, default=0, metavar='STEPS',
                    help='ramp the KL weight linearly from 0 to --beta over the first STEPS training steps')
    ap.add_argument('--iter-weights', choices=['linspace', 'uniform', 'last'], default='linspace',
                    help='per-iteration loss weights (model.iter_weights): (i+1)/(T+1), 1/(T+1) each, or the final ELBO only')
    ap.add_argument('--clip-frames', type=int, default=0, metavar='F',
                    help='train on synthetic clips of F = c * ITERS + 1 frames (frame i = the scene rolled by (i, 2i) pixels), one optimizer '
                         'step per clip, the refinement state carried from chunk to chunk')
    ap.add_argument('--bptt', choices=['truncated', 'exact'], default='truncated',
                    help='with --clip-frames: no gradient across chunk boundaries, or the exact gradient of the whole clip by recomputation')
    ap.add_argument('--ignore-border', type=int, default=0, metavar='N',
                    help='train with zero observation weight on an N-pixel frame around every image (per-pixel weights: the border is not '
                         'part of the objective, the reconstruction still covers it)')
    ap.add_argument('--learn-sigma', action='store_true',
                    help='learn the likelihood scale: a parameter log_sigma (initially log of --sigma / ARCH.SIGMA) in its own param group, '
                         'model.sigma = exp(log_sigma) before every step; saved as the checkpoint entry log_sigma')
    ap.add_argument('--stable-encoding', action='store_true',
                    help='mask_posterior channel of the refinement input as a max-subtracted softmax (model.stable_encoding): finite where the '
                         "reference's un-stabilised form is 0 / 0, which a small or shrinking sigma reaches")
    ap.add_argument('--likelihood', choices=['per_channel', 'joint'], default=None,
                    help="form of the pixel likelihood (model.likelihood): 'per_channel', the reference's K-component mixture for each colour "
                         "channel, or 'joint', the paper's one mixture per pixel over the RGB vector; without the flag the model keeps its own (ARCH.LIKELIHOOD, else 'per_channel').  Not written into state_dict (which keeps "
                         "the reference's layout): pass it again with --resume")
    ap.add_argument('--learn-input-gain', action='store_true',
                    help='learn a per-channel gain and offset applied to every batch before the model (six parameters in their own param '
                         'group, trained through the gradient into the image); saved as the checkpoint entry input_gain')
    ap.add_argument('--eval-samples', type=int, default=0, metavar='S',
                    help='also report the S-sample importance-weighted bound (IWAE) and the S-sample Monte-Carlo ELBO of the evaluation set, '
                         'per image in nats (one model.predictive call per batch; 0: off)')
    ap.add_argument('--eval-restarts', type=int, default=0, metavar='C',
                    help='evaluate the best of C refinement chains per image (IODINE.restarts) and report the stability of the chains and '
                         'the gain of selecting; 0 / 1 = one chain, the usual evaluation')
    ap.add_argument('--eval-adaptive-rtol', type=float, default=None, metavar='X',
                    help='evaluate with adaptive refinement (IODINE.reconstruct_adaptive): an image stops once its ELBO estimate rises by less '
                         'than tol + X |ELBO| between two evaluations; reports the mean and histogram of the iteration counts and the share '
                         'of images at the maximum beside the usual metrics')
    ap.add_argument('--eval-adaptive-tol', type=float, default=None, metavar='Y', help='with adaptive evaluation: the absolute tolerance in nats')
    ap.add_argument('--eval-max-iters', type=int, default=None, metavar='N', help='with adaptive evaluation: the most updates per image (default: ITERS)')
    ap.add_argument('--eval-check-every', type=int, default=1, metavar='R', help='with adaptive evaluation: updates per round')
    ap.add_argument('--mask-loss', type=float, default=0.0, metavar='W',
                    help='supervised masks: add W * matched_mask_loss(model.mask, ground truth) to every step whose batch carries masks '
                         '(ground-truth objects assigned to slots on the device; 0: off)')
    ap.add_argument('--mask-loss-kind', choices=['ce', 'iou'], default='ce', help='with --mask-loss: the loss of a matched (object, slot) pair')
    ap.add_argument('--mask-match', choices=['iou', 'ce'], default='iou', help='with --mask-loss: the cost the assignment minimises')
    ap.add_argument('--metrics', action='store_true',
                    help='evaluate with SegmentationEvaluator: matched mIoU, segmentation covering (SC) and mSC beside the ARI')
    ap.add_argument('--min-component-area', type=int, default=0, metavar='N',
                    help='with --metrics: also split every argmax map into connected components (iodine_amd.objects.components) and report '
                         'the components per non-empty slot, the share of pixels in components below N pixels, and ARI / mIoU / SC / mSC of '
                         'the maps with those components absorbed by a neighbour (0: off)')
    ap.add_argument('--resident', nargs='?', const='', default=None, metavar='CACHE.npz',
                    help='keep the data set in device memory and assemble every batch there (iodine_amd.resident): --clevr / --dsprites are '
                         'ingested once - and written to CACHE.npz, or loaded from it when it exists -, without a data set the synthetic scenes '
                         '(or, with --clip-frames, clips) are generated on the device; training and evaluation then run without host work '
                         'per batch')
    ap.add_argument('--augment', metavar='SPEC',
                    help='with --resident: train on random windows cut on the device (iodine_amd.windows.Augment) - a comma-separated list of '
                         'flip, scale=LO:HI, ratio=LO:HI, translate=PIXELS|full, gain=G, e.g. flip,scale=0.7:1,ratio=0.8:1.25,translate=8,'
                         'gain=0.1; evaluation keeps the centre window')
    ap.add_argument('--native-frames', action='store_true',
                    help='with --resident and --clevr: keep the frames at their native size (FrameStore.from_clevr; --resident CACHE.npz '
                         'caches that store) and cut the centre crop, or the --augment windows, on the device')
    ap.add_argument('--crop', type=int, default=192, metavar='PIXELS', help='with --native-frames: the side of the centre crop (192)')
    ap.add_argument('--traverse', metavar='OUT.npz',
                    help='instead of training: after loading (--resume), reconstruct the first batch, traverse the latent units of image 0 '
                         '(each slot, the units with the largest KL, moved along the posterior) and save the grids; see save_traversal')
    ap.add_argument('--traverse-top', type=int, default=8, metavar='N', help='with --traverse: units per slot, by descending KL')
    ap.add_argument('--traverse-values', type=int, default=7, metavar='V', help='with --traverse: values per unit, linspace(-2, 2, V) posterior sigmas')
    ap.add_argument('--sheet', metavar='OUT.png',
                    help='write the decomposition sheet of the first evaluation batch after training / --resume: image, reconstruction, '
                         'ground truth (when the batch carries masks, with matched colours), segmentation and one panel per slot, a row per '
                         'image, rendered on the device (iodine_amd.figures)')
    ap.add_argument('--sheet-images', type=int, default=8, metavar='N', help='with --sheet / --sheet-every: images (rows) per sheet')
    ap.add_argument('--sheet-scale', type=int, default=1, metavar='Z', help='with --sheet / --sheet-every: integer magnification 1..8')
    ap.add_argument('--sheet-trajectory', type=int, default=None, metavar='B',
                    help='with --sheet: the refinement figure of image B of the batch instead, one row per decode (ITERS + 1 rows)')
    ap.add_argument('--sheet-every', type=int, default=0, metavar='STEPS',
                    help='with --sheet OUT.png: also write OUT_<step>.png from the first images of the current batch every STEPS training '
                         'steps; the training losses are bit-identical with and without it')
    return ap


def _sheet_kw(args):
    if args.sheet_every and not args.sheet:
        raise SystemExit('--sheet-every needs --sheet OUT.png (the step files are named after it)')
    return dict(sheet_every=args.sheet_every, sheet_path=args.sheet, sheet_images=args.sheet_images, sheet_scale=args.sheet_scale)


def _final_sheet(args, model, batches, device, rank):
    """``--sheet``: the sheet of the first batch of ``batches``, rank 0 only"""
    if args.sheet and rank == 0:
        save_sheet(model, next(iter(batches)), args.sheet, device, images=args.sheet_images, scale=args.sheet_scale,
                   trajectory=args.sheet_trajectory)


def main(argv=None):
    from . import IODINE
    from .data import CLEVR, MultiDSprites, make_dataloader
    from .model import clevr6_arch, dsprites_arch
    args = make_parser().parse_args(argv)
    if (args.augment or args.native_frames) and args.resident is None:
        raise SystemExit('--augment / --native-frames cut their windows from a device-resident store: add --resident')
    if args.native_frames and not args.clevr:
        raise SystemExit('--native-frames ingests a CLEVR folder at its native size: add --clevr')
    if args.min_component_area < 0 or (args.min_component_area and not args.metrics):
        raise SystemExit('--min-component-area N >= 0 reports beside the scores of --metrics: add --metrics')
    try:
        args.augment = parse_augment(args.augment) if args.augment else None   # (a bad spec is refused before any work)
    except ValueError as e:
        raise SystemExit(str(e))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank, local = int(os.environ.get('RANK', '0')), int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        torch.distributed.init_process_group('nccl', rank=rank, world_size=world)    # RCCL on ROCm
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    arch = clevr6_arch() if args.config == 'clevr6' else dsprites_arch()
    torch.manual_seed(0)                                                     # same initial replica on every rank
    model = IODINE(arch).to(device)
    model.manual_seed(1000 + rank)                                           # ... but its own reparameterisation noise
    if args.conv_precision != 1:
        model.set_option('conv_precision', args.conv_precision)
    if args.gen_conv_precision:
        model.set_option('gen_conv_precision', args.gen_conv_precision)
    if args.sigma is not None:
        model.sigma = args.sigma
    model.beta, model.iter_weights = args.beta, args.iter_weights
    model.stable_encoding = args.stable_encoding
    if args.likelihood is not None:
        model.likelihood = args.likelihood
    if rank == 0:
        print('objective: likelihood {}, sigma {}, beta {}, iter_weights {}'.format(model.likelihood, model.sigma, model.beta, model.iter_weights))
    optimizer = make_optimizer(model, base_lr=args.lr, max_grad_norm=args.clip)
    log_sigma = make_log_sigma(model.sigma, device) if args.learn_sigma else None
    if args.resume:
        resume(args.resume, model, optimizer, log_sigma, args.lr)
    elif log_sigma is not None:
        add_sigma_group(optimizer, log_sigma, args.lr)
    input_gain = None
    if args.learn_input_gain:
        if args.resume or args.clip_frames:
            raise SystemExit('--learn-input-gain starts a fresh run on still images; it cannot be combined with --resume / --clip-frames')
        input_gain = InputGain(device)
        optimizer.add_param_group({'params': list(input_gain.parameters()), 'lr': args.lr, 'weight_decay': 0.0})
    if args.clevr:
        ds = CLEVR(args.clevr)
    elif args.dsprites:
        ds = MultiDSprites(args.dsprites)
    else:
        ds = SyntheticScenes(args.batch * world * 8, arch.IMG_SIZE)
    if args.resident is not None and not args.traverse:
        return _main_resident(args, arch, model, optimizer, ds, device, rank, world, log_sigma, input_gain)
    if args.traverse:
        image = next(iter(make_dataloader(ds, args.batch, shuffle=False, rank=rank, world_size=world)))[0]
        if rank == 0:
            save_traversal(model, image.to(device), args.traverse, args.traverse_top, args.traverse_values)
        return
    train_ds = ds
    if args.clip_frames and args.mask_loss:
        raise SystemExit('--mask-loss trains on still images; it cannot be combined with --clip-frames')
    if args.clip_frames:
        clip_chunks(args.clip_frames, arch.ITERS)                           # (refuse a frame count that does not split before any work)
        if args.clevr or args.dsprites:
            raise SystemExit('--clip-frames trains on synthetic clips; it cannot be combined with --clevr / --dsprites')
        train_ds = SyntheticClips(args.batch * world * 8, arch.IMG_SIZE, args.clip_frames)
    dl = make_dataloader(train_ds, args.batch, shuffle=True, rank=rank, world_size=world)
    losses = train(model, optimizer, dl, device, args.steps, checkpoint_path=args.save,
                   log=print if rank == 0 else (lambda *a: None), beta=args.beta, beta_warmup_steps=args.beta_warmup,
                   bptt=args.bptt if args.clip_frames else None, ignore_border=args.ignore_border, log_sigma=log_sigma,
                   input_gain=input_gain, mask_loss=args.mask_loss, mask_loss_kind=args.mask_loss_kind, mask_match=args.mask_match,
                   **_sheet_kw(args))
    evaluator = None
    if args.metrics:
        from .matching import SegmentationEvaluator
        evaluator = SegmentationEvaluator()
    ev = evaluate(model, make_dataloader(ds, args.batch, shuffle=False, rank=rank, world_size=world), device, evaluator=evaluator,
                  bound_samples=args.eval_samples, restarts=args.eval_restarts, min_component_area=args.min_component_area,
                  adaptive=_adaptive_options(args))
    _report(args, rank, losses, ev)
    _final_sheet(args, model, make_dataloader(ds, args.batch, shuffle=False, rank=rank, world_size=world), device, rank)


def _resident_store(args, arch, ds, device, rank, frames=0):
    """the store of ``--resident``: the data set ingested (or its cache loaded), or the synthetic scenes / clips generated on the device"""
    from .resident import ResidentDataset
    log = print if rank == 0 else (lambda *a: None)
    if not (args.clevr or args.dsprites):
        return ResidentDataset.synthetic(len(ds), arch.IMG_SIZE, frames=frames, device=device)
    cache = args.resident or None
    if cache and os.path.exists(cache):
        log(f'resident: loading {cache}')
        return ResidentDataset.load(cache, device)
    store = ResidentDataset.from_dataset(ds, device, log=log)                # (no workers: this process has the device open by now)
    if cache and rank == 0:
        store.save(cache)
        log(f'resident: wrote {cache}')
    return store


def parse_augment(spec):
    """``--augment SPEC`` -> the keyword arguments of ``windows.Augment``: a comma-separated list of ``flip``, ``scale=LO:HI`` (or one
    number), ``ratio=LO:HI``, ``translate=PIXELS`` or ``translate=full``, ``gain=G``.  A ``ValueError`` names the entry it cannot read;
    the ranges themselves are ``Augment``'s to check."""
    kw = {}
    for entry in (e.strip() for e in str(spec).split(',')):
        key, eq, value = entry.partition('=')
        if key not in ('flip', 'scale', 'ratio', 'translate', 'gain'):
            raise ValueError(f'--augment: unknown entry {entry!r} (flip, scale=LO:HI, ratio=LO:HI, translate=PIXELS|full, gain=G)')
        if key in kw:
            raise ValueError(f'--augment: {key} is given twice')
        if key == 'flip':
            if eq:
                raise ValueError(f'--augment: flip takes no value; got {entry!r}')
            kw[key] = True
            continue
        try:
            if key == 'translate' and value == 'full':
                kw[key] = 'full'
            elif key in ('scale', 'ratio'):
                parts = [float(p) for p in value.split(':')]
                if len(parts) not in (1, 2):
                    raise ValueError
                kw[key] = (parts[0], parts[-1])
            else:
                kw[key] = float(value)
        except ValueError:
            raise ValueError(f'--augment: cannot read {entry!r} ({key}={"LO:HI" if key in ("scale", "ratio") else "NUMBER"})') from None
    return kw


def _native_store(args, device, ds, rank):
    """the store of ``--native-frames``: the CLEVR folder at its native size (or its cache loaded)"""
    from .windows import FrameStore
    log = print if rank == 0 else (lambda *a: None)
    cache = args.resident or None
    if cache and os.path.exists(cache):
        log(f'resident: loading {cache}')
        return FrameStore.load(cache, device)
    frames = FrameStore.from_clevr(ds, device, log=log)
    if cache and rank == 0:
        frames.save(cache)
        log(f'resident: wrote {cache}')
    return frames


def _main_resident(args, arch, model, optimizer, ds, device, rank, world, log_sigma, input_gain):
    """``main`` from a device-resident store: the same training and evaluation calls, batches from ``ResidentDataset.batches`` - or, with
    ``--augment`` / ``--native-frames``, from ``FrameStore.batches`` (iodine_amd.windows)"""
    if args.clip_frames and args.mask_loss:
        raise SystemExit('--mask-loss trains on still images; it cannot be combined with --clip-frames')
    if args.clip_frames:
        clip_chunks(args.clip_frames, arch.ITERS)
        if args.clevr or args.dsprites:
            raise SystemExit('--clip-frames trains on synthetic clips; it cannot be combined with --clevr / --dsprites')
    if args.native_frames:
        from .windows import Augment, Center
        frames = _native_store(args, device, ds, rank)
        if rank == 0:
            print('resident: {} frames of {} x {}, uint8 images, {:.1f} MiB on {}; windows of {} -> {}'.format(
                len(frames), frames.height, frames.width, frames.nbytes() / 2 ** 20, device, args.crop, arch.IMG_SIZE))
        policy = Augment(crop=args.crop, **args.augment) if args.augment is not None else Center(args.crop)
        train_batches = frames.batches(args.batch, arch.IMG_SIZE, policy, shuffle=True, rank=rank, world_size=world)
        eval_batches = lambda: frames.batches(args.batch, arch.IMG_SIZE, Center(args.crop), shuffle=False, rank=rank, world_size=world)
    else:
        store = _resident_store(args, arch, ds, device, rank)
        train_store = _resident_store(args, arch, ds, device, rank, frames=args.clip_frames) if args.clip_frames else store
        if rank == 0:
            print('resident: {} items of {} x {}, {} images, {:.1f} MiB on {}'.format(len(store), store.size, store.size,
                  'uint8' if store.image_kind == 0 else 'float32', (store.nbytes() + (train_store.nbytes() if train_store is not store else 0)) / 2 ** 20, device))
        if args.augment is not None:
            from .windows import Augment, FrameStore
            train_batches = FrameStore.from_resident(train_store).batches(args.batch, store.size, Augment(**args.augment), shuffle=True,
                                                                          rank=rank, world_size=world)
        else:
            train_batches = train_store.batches(args.batch, shuffle=True, rank=rank, world_size=world)
        eval_batches = lambda: store.batches(args.batch, shuffle=False, rank=rank, world_size=world)
    losses = train(model, optimizer, train_batches, device, args.steps,
                   checkpoint_path=args.save, log=print if rank == 0 else (lambda *a: None), beta=args.beta,
                   beta_warmup_steps=args.beta_warmup, bptt=args.bptt if args.clip_frames else None, ignore_border=args.ignore_border,
                   log_sigma=log_sigma, input_gain=input_gain, mask_loss=args.mask_loss, mask_loss_kind=args.mask_loss_kind,
                   mask_match=args.mask_match, **_sheet_kw(args))
    evaluator = None
    if args.metrics:
        from .matching import SegmentationEvaluator
        evaluator = SegmentationEvaluator()
    ev = evaluate(model, eval_batches(), device, evaluator=evaluator, bound_samples=args.eval_samples, restarts=args.eval_restarts,
                  min_component_area=args.min_component_area, adaptive=_adaptive_options(args))
    _report(args, rank, losses, ev)
    _final_sheet(args, model, eval_batches(), device, rank)


def _adaptive_options(args):
    """the ``adaptive=`` of ``evaluate`` from the --eval-adaptive-* flags (None: not asked for)"""
    if args.eval_adaptive_rtol is None and args.eval_adaptive_tol is None:
        return None
    opts = dict(rtol=args.eval_adaptive_rtol or 0.0, check_every=args.eval_check_every)
    if args.eval_adaptive_tol is not None:
        opts['tol'] = args.eval_adaptive_tol
    elif not opts['rtol'] > 0:
        opts['tol'] = 0.0
    if args.eval_max_iters is not None:
        opts['max_iters'] = args.eval_max_iters
    return opts


def _report(args, rank, losses, ev):
    if rank == 0:
        print('first loss {:.2f} -> last loss {:.2f}; Ari over all ranks: {}'.format(losses[0], losses[-1], ev.global_mean))
        if args.metrics:
            print('mIoU {:.4f}, SC {:.4f}, mSC {:.4f} over all ranks'.format(*[ev.global_means[n] for n in ('mious', 'scs', 'mscs')]))
        if args.min_component_area:
            print('connected components: {:.3f} per non-empty slot, {:.4%} of the pixels in components below {} pixels; those absorbed: '
                  'Ari {}, mIoU {:.4f}, SC {:.4f}, mSC {:.4f}'.format(ev.cleaned['components_per_slot'], ev.cleaned['small_pixel_share'],
                                                                       args.min_component_area,
                                                                       *[ev.cleaned[n] for n in ('aris', 'mious', 'scs', 'mscs')]))
        if args.eval_restarts > 1:
            print('best of {} chains per image: stability {:.4f}, score {:.3f} (chain 0 alone: {:.3f})'.format(
                args.eval_restarts, ev.stability, ev.best_score, ev.first_score))
        if getattr(ev, 'adaptive', None):
            a = ev.adaptive
            print('adaptive refinement: {:.3f} iterations per image (max {}), {:.2%} of the images at the maximum; images per count 0..{}: {}'.format(
                a['mean_iters'], a['max_iters'], a['at_max'], a['max_iters'], a['hist']))
        if args.eval_samples:
            print('{}-sample bounds per image: IWAE {:.3f}, Monte-Carlo ELBO {:.3f}'.format(args.eval_samples, ev.iwae, ev.elbo_mc))


if __name__ == '__main__':
    main()
