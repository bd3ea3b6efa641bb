"""Adaptive refinement: refine every image until its own posterior stops improving (``IODINE.reconstruct_adaptive``).

``Adaptive`` is what that call returns.  ``select`` / ``move`` are thin wrappers of the two stateless device steps the library runs between
two rounds of the call (``iodine_adaptive_select`` / ``iodine_adaptive_move``, include/iodine_hip.h), for loops of one's own: which of the
active images stop after ``t`` updates, as two stably compacted lists, and a table of row gathers / scatters in one launch.
tests/adaptive_reference.py is the numpy definition of the stopping rule."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional

import torch

from . import _args, _lib


@dataclasses.dataclass
class Adaptive:
    """What ``IODINE.reconstruct_adaptive`` returns.  ``pred (B, 3, S, S)``, ``mask (B, K, 1, S, S)``, ``mean (B, K, 3, S, S)``, ``z``,
    ``post_mean``, ``post_logvar (B, K, L)``: for image b what ``reconstruct`` returns for it at ``n_iters = iters[b]``, bit for bit;
    ``iters (B)`` int32 - the updates image b received; ``ll``, ``kl (max_iters, B)`` float32 - the per-image terms of its ELBO evaluations,
    NaN from row ``iters[b]`` on; ``score (max_iters, B)`` float64 = ll - beta kl; ``active``: list of ints, the batch every round ran at (0
    for rounds that did not run).  Detached tensors."""
    pred: torch.Tensor
    mask: torch.Tensor
    mean: torch.Tensor
    z: torch.Tensor
    post_mean: torch.Tensor
    post_logvar: torch.Tensor
    iters: torch.Tensor
    ll: torch.Tensor
    kl: torch.Tensor
    score: torch.Tensor
    active: list


def controls(max_iters, min_iters, check_every, tol, rtol, who='adaptive'):
    """The checked ``iodine_adaptive_ctl`` of a call; every refusal a ValueError on the host."""
    for name, v in (('max_iters', max_iters), ('min_iters', min_iters), ('check_every', check_every)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f'{who}: {name} must be an integer; got {v!r}')
    if max_iters < 1:
        raise ValueError(f'{who}: max_iters must be >= 1; got {max_iters}')
    if not 1 <= min_iters <= max_iters:
        raise ValueError(f'{who}: min_iters must be in 1..max_iters = {max_iters}; got {min_iters}')
    if check_every < 1:
        raise ValueError(f'{who}: check_every must be >= 1; got {check_every}')
    for name, v in (('tol', tol), ('rtol', rtol)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f'{who}: {name} must be a real number; got {v!r}')
    if math.isnan(tol):
        raise ValueError(f'{who}: tol must not be NaN (any finite number, -inf = never stop early, +inf = stop at the first permitted check)')
    if not rtol >= 0:
        raise ValueError(f'{who}: rtol must be >= 0; got {rtol!r}')
    return _lib.AdaptiveCtl(max_iters, min_iters, check_every, float(tol), float(rtol))


def _i32(t, name, n=None):
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or (n is not None and t.shape[0] < n):
        raise ValueError(f'adaptive: {name} must be a 1-D int32 tensor' + (f' of at least {n} entries' if n is not None else ''))
    return t.contiguous()


@torch.no_grad()
def select(terms, t, iters, ll, kl, *, tol, rtol=0.0, min_iters=2, check_every=1, beta=1.0, idx=None, budget=None):
    """One decision step.  ``terms (R, n, 2)`` float32 = {ll, kl} of the round's evaluations t - R .. t - 1 for the n active images in
    their current layout; ``idx (n)`` int32 their original indices (None: position = index); ``iters (B)`` int32 and the traces ``ll``,
    ``kl (max_iters, B)`` float32 are updated in place; ``budget (B)`` int32 or None.  Returns ``(idx_out, pos_out, stop_idx, stop_pos,
    counts)``, int32 device tensors: the first ``counts[0]`` entries of ``idx_out`` / ``pos_out`` are the original indices / positions of
    the images that continue, in position order, the first ``counts[1]`` of ``stop_idx`` / ``stop_pos`` those that stop.  No synchronise."""
    _args.all_tensors((terms, iters, ll, kl), 'adaptive.select: terms, iters, ll and kl must be tensors')
    if terms.dim() != 3 or terms.shape[2] != 2 or terms.dtype != torch.float32 or terms.shape[1] < 1:
        raise ValueError(f'adaptive.select: terms must be float32 of shape (R, n, 2); got {terms.dtype} {tuple(terms.shape)}')
    R, n = int(terms.shape[0]), int(terms.shape[1])
    if ll.dim() != 2 or ll.shape != kl.shape or ll.dtype != torch.float32 or kl.dtype != torch.float32:
        raise ValueError('adaptive.select: ll and kl must be float32 of one shape (max_iters, B)')
    M, B = int(ll.shape[0]), int(ll.shape[1])
    ctl = controls(M, min_iters, check_every, tol, rtol, 'adaptive.select')
    iters, idx, budget = _i32(iters, 'iters', B), _i32(idx, 'idx', n), _i32(budget, 'budget', B)
    _args.one_device([terms, iters, ll, kl] + [v for v in (idx, budget) if v is not None],
                     'adaptive.select runs only on a ROCm device (gfx950), all tensors on one; there is no CPU fallback')
    if not (ll.is_contiguous() and kl.is_contiguous()):
        raise ValueError('adaptive.select: ll and kl are written in place and must be contiguous')
    dev = terms.device
    out = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call('iodine_adaptive_select', dev, terms.contiguous(), idx, n, R, int(t), B, C.byref(ctl), float(beta), budget, *out, counts, iters, ll, kl)
    return (*out, counts)


@torch.no_grad()
def move(entries):
    """Row gathers / scatters in one launch per 16 entries.  ``entries``: tuples ``(src, dst, src_index, dst_index, rows)`` - float32
    contiguous tensors whose rows are ``src[i]`` / ``dst[i]`` (same row size), int32 index tensors or None (row r itself), and the number of
    rows to move; row r goes from ``src[src_index[r]]`` to ``dst[dst_index[r]]``.  ``src`` and ``dst`` of an entry must not share memory (the
    library refuses overlapping ranges).  No synchronise."""
    table, dev, keep = [], None, []
    for i, (src, dst, si, di, rows) in enumerate(entries):
        _args.all_tensors((src, dst), f'adaptive.move: entry {i}: src and dst must be tensors')
        if src.dtype != torch.float32 or dst.dtype != torch.float32 or src.dim() < 1 or dst.dim() < 1 or src.shape[1:].numel() != dst.shape[1:].numel():
            raise ValueError(f'adaptive.move: entry {i}: src and dst must be float32 with rows of one size')
        if not (src.is_contiguous() and dst.is_contiguous()):
            raise ValueError(f'adaptive.move: entry {i}: src and dst must be contiguous')
        si, di = _i32(si, 'src_index', rows), _i32(di, 'dst_index', rows)
        _args.one_device([src, dst] + [v for v in (si, di) if v is not None],
                         'adaptive.move runs only on a ROCm device (gfx950), all tensors on one; there is no CPU fallback')
        dev = dev or src.device
        keep += [si, di]
        table.append(_lib.MoveEntry(src.data_ptr(), dst.data_ptr(), int(src.shape[1:].numel()), si.data_ptr() if si is not None else None,
                                    di.data_ptr() if di is not None else None, int(rows), int(src.shape[0]), int(dst.shape[0])))
    for s in range(0, len(table), 16):
        part = table[s:s + 16]
        _lib.call('iodine_adaptive_move', dev, (_lib.MoveEntry * len(part))(*part), len(part))
