"""Fused Adam over all parameters in one launch, with optional global-norm gradient clipping.

Mirrors ``make_optimizer`` of the reference (lib/solver/build.py:5-16): ``torch.optim.Adam`` over every parameter
with ``lr = TRAIN.BASE_LR`` and ``weight_decay = TRAIN.WEIGHT_DECAY``; ``optimizer.step()`` is lib/engine/train.py:65.
The state (``exp_avg``, ``exp_avg_sq``, ``step``) and the param-group layout (one group per parameter) are torch's /
the reference's, so ``state_dict()`` round-trips with the ``'optimizer'`` entry of a reference checkpoint
(lib/utils/checkpoint.py:36-54; tests/golden/ckpt_tiny is one written by the reference).  No CPU / eager fallback.

Clipping is the line the reference carries commented out in front of the step, ``# clip_grad_norm_(model.parameters(), 5.0)``
(lib/engine/train.py:64; the paper clips at 5.0): ``clip_grad_norm_`` below is the stand-alone form,
``FusedAdam(max_grad_norm=...)`` the fused one (one deterministic norm over all gradients, the coefficient read from device
memory by the Adam kernel: no host synchronisation, no extra pass over the gradients).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib

_NONFINITE = ('propagate', 'skip')


def _check_max_norm(max_norm, what):
    max_norm = float(max_norm)
    if math.isnan(max_norm) or max_norm <= 0.0:
        raise ValueError(f'{what} must be a positive number (inf allowed), got {max_norm}')
    return max_norm


def _check_grad(p):
    if p.device.type != 'cuda' or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.device != p.device:
        raise RuntimeError('FusedAdam / clip_grad_norm_ need float32 parameters and gradients on a ROCm device (no CPU fallback)')
    if not p.grad.is_contiguous():
        p.grad = p.grad.contiguous()


class _GradNorm:
    """Device buffers of the norm: the partial-sum scratch, ``out4`` = (total_norm, clip_coef, non-finite flag, count of
    non-finite norms) and the gradient table; rebuilt only when an address or a size changes."""

    def __init__(self):
        self.out4 = None
        self.scratch = None
        self._cached = None

    def buffers(self, dev, total):
        if self.out4 is None or self.out4.device != dev:
            self.out4 = torch.zeros(4, dtype=torch.float32, device=dev)
            self.scratch = None
        need = _lib.lib().iodine_grad_norm_scratch_bytes(total)
        if self.scratch is None or self.scratch.numel() * 8 < need:
            self.scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)

    def table(self, grads):
        """(ptrs, offsets, total) with only the gradient column filled (the norm and the scale read nothing else)."""
        key = tuple((g.data_ptr(), g.numel()) for g in grads)
        if self._cached is None or self._cached[0] != key:
            ptrs, offs, tot = [], [], 0
            for a, n in key:
                ptrs.extend((0, a, 0, 0)); offs.append(tot); tot += n
            dev = grads[0].device
            self._cached = (key, torch.tensor(ptrs, dtype=torch.int64).to(dev), torch.tensor(offs, dtype=torch.int64).to(dev), tot)
        return self._cached[1:]

    def norm(self, ptrs, offs, n, total, max_norm, dev):
        self.buffers(dev, total)
        _lib.call('iodine_grad_norm', dev, ptrs, offs, n, total, max_norm, self.scratch, self.scratch.numel() * 8, self.out4)


_standalone = {}        # device -> _GradNorm of clip_grad_norm_


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """``torch.nn.utils.clip_grad_norm_`` (lib/engine/train.py:64) on ROCm tensors: a deterministic fp64 norm over all
    gradients, ``clip_coef = min(1, max_norm / (total_norm + 1e-6))`` and ``grad *= clip_coef`` in place - three launches,
    no host synchronisation.  Returns the total norm as a 0-dim DEVICE tensor."""
    if float(norm_type) != 2.0:
        raise ValueError(f'clip_grad_norm_: only norm_type = 2 is implemented, got {norm_type}')
    max_norm = _check_max_norm(max_norm, 'max_norm')
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    ps = [p for p in parameters if p.grad is not None and p.grad.numel() > 0]
    if not ps:
        raise ValueError('clip_grad_norm_: no parameter has a gradient')
    for p in ps:
        _check_grad(p)
    dev = ps[0].device
    if any(p.device != dev for p in ps):
        raise RuntimeError('clip_grad_norm_: all gradients must live on one device')
    gn = _standalone.setdefault(dev, _GradNorm())
    ptrs, offs, total = gn.table([p.grad for p in ps])
    gn.norm(ptrs, offs, len(ps), total, max_norm, dev)
    _lib.call('iodine_grad_scale', dev, ptrs, offs, len(ps), total, C.c_void_p(gn.out4.data_ptr() + 4))
    for p in ps:
        torch.autograd.graph.increment_version(p.grad)        # written through raw pointers
    return gn.out4[0].clone()


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (amsgrad=False, maximize=False) as one HIP launch per bucket of equal hyper-parameters.

    ``max_grad_norm``: clip the global 2-norm of ALL gradients (every param group, every bucket) like
    ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` in front of the step (lib/engine/train.py:64), fused: one norm, then
    the Adam kernel multiplies each gradient by the coefficient it reads from device memory; ``.grad`` itself is not rewritten.
    ``last_grad_norm`` is the norm of the last step and ``skipped_steps`` the count of non-finite norms, both device scalars
    (views of one buffer, overwritten by the next step; reading them with ``.item()`` is the caller's synchronisation).
    ``nonfinite='propagate'`` is torch's behaviour (NaN / inf flow into the parameters); ``'skip'`` leaves parameters and both
    moments untouched when the norm is inf / NaN - ``state['step']`` still advances, because the host cannot know without a
    synchronisation.  Both are attributes of the optimizer, NOT entries of ``defaults`` / ``param_groups``: ``state_dict()``
    keeps the reference's layout."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 nonfinite='propagate'):
        if nonfinite not in _NONFINITE:
            raise ValueError(f'nonfinite must be one of {_NONFINITE}, got {nonfinite!r}')
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm, 'max_grad_norm')
        self.nonfinite = nonfinite
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._tables = {}
        self._gradnorm = _GradNorm()

    @property
    def last_grad_norm(self):
        return None if self._gradnorm.out4 is None else self._gradnorm.out4[0]

    @property
    def skipped_steps(self):
        return None if self._gradnorm.out4 is None else self._gradnorm.out4[3]

    def _table(self, gi, ps):
        """(ptrs, offsets, total) device tables for one fused bucket; rebuilt when any address changes."""
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]['exp_avg'].data_ptr(),
                     self.state[p]['exp_avg_sq'].data_ptr(), p.numel()) for p in ps)
        cached = self._tables.get(gi)
        if cached is None or cached[0] != key:
            dev = ps[0].device
            ptrs, offs, tot = [], [], 0
            for k in key:
                ptrs.extend(k[:4]); offs.append(tot); tot += k[4]
            cached = (key, torch.tensor(ptrs, dtype=torch.int64).to(dev), torch.tensor(offs, dtype=torch.int64).to(dev), tot)
            self._tables[gi] = cached
        return cached[1], cached[2], cached[3]

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        # The reference builds ONE PARAM GROUP PER PARAMETER (lib/solver/build.py:10-14); groups that share their
        # hyper-parameters and step count are fused into a single launch (one launch per step for the reference layout).
        buckets = {}
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.device.type != 'cuda' or p.dtype != torch.float32:
                    raise RuntimeError('FusedAdam needs float32 parameters on a ROCm device (no CPU fallback)')
                if not p.grad.is_contiguous():
                    p.grad = p.grad.contiguous()
                st = self.state[p]
                if not st:
                    st['step'] = torch.tensor(0.0)            # torch.optim.Adam keeps the step as a CPU float32 tensor
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                key = (group['lr'], tuple(group['betas']), group['eps'], group['weight_decay'], int(st['step']), p.device)
                buckets.setdefault(key, []).append(p)
        clip = self.max_grad_norm is not None and bool(buckets)
        if clip:
            # lib/engine/train.py:64: ONE norm over every gradient, in front of all buckets.  A single bucket (the reference
            # layout) lends its table; several buckets get a table of all gradients, cached like the buckets' own.
            every = [p for ps in buckets.values() for p in ps]
            dev = every[0].device
            if any(p.device != dev for p in every):
                raise RuntimeError('FusedAdam(max_grad_norm=...): all parameters must live on one device')
            if any(p.grad.dtype != torch.float32 or p.grad.device != dev for p in every):
                raise RuntimeError('FusedAdam needs float32 gradients on a ROCm device (no CPU fallback)')
            if len(buckets) == 1:
                key = next(iter(buckets))
                ptrs, offs, total = self._table(key[:4] + (dev,), every)
            else:
                ptrs, offs, total = self._gradnorm.table([p.grad for p in every])
            self._gradnorm.norm(ptrs, offs, len(every), total, self.max_grad_norm, dev)
            clipped = (self._gradnorm.out4, int(self.nonfinite == 'skip'))
        for key, ps in buckets.items():
            lr, (b1, b2), eps, wd, t0, dev = key
            t = t0 + 1
            ptrs, offs, total = self._table(key[:4] + (dev,), ps)
            if clip:
                _lib.call('iodine_adam_step_clipped', dev, ptrs, offs, len(ps), total, lr, b1, b2, eps, wd, t, *clipped)
            else:
                _lib.call('iodine_adam_step', dev, ptrs, offs, len(ps), total, lr, b1, b2, eps, wd, t)
            for p in ps:
                st = self.state[p]
                st['step'] = st['step'] + 1 if torch.is_tensor(st['step']) else t     # int steps: checkpoints of old torch
                # the kernel wrote through raw pointers: tell torch (and IODINE._sync_params, which re-packs the weights
                # when a parameter's version counter moves) that the tensor changed in place
                torch.autograd.graph.increment_version(p)
        return loss


def make_optimizer(model, base_lr=3e-4, weight_decay=0.0, max_grad_norm=None, nonfinite='propagate'):
    """lib/solver/build.py:5-16: Adam with one param group per parameter (``params += [{'params': [value], 'lr': lr,
    'weight_decay': weight_decay}]``), so ``optimizer.state_dict()`` has the reference's layout and the ``'optimizer'``
    entry of a reference checkpoint (lib/utils/checkpoint.py:36-54) loads with ``load_state_dict``.  ``max_grad_norm`` /
    ``nonfinite``: lib/engine/train.py:64 fused into the step (see ``FusedAdam``); they do not enter the state dict."""
    params = [{'params': [p], 'lr': base_lr, 'weight_decay': weight_decay}
              for _, p in model.named_parameters() if p.requires_grad]
    return FusedAdam(params, lr=base_lr, max_grad_norm=max_grad_norm, nonfinite=nonfinite)
