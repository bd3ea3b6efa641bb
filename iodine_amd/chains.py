"""Refinement restarts: several decodes of the same images - the chains of ``IODINE.restarts`` - scored, labelled and folded into one labelling.

IODINE's inference is stochastic and multi-stable: the same image refined with other noise can settle into another decomposition.
``chain_score`` takes C decodes of B images, ``mask (C, B, K, 1, S, S)`` and ``mean (C, B, K, 3, S, S)`` with row ``c B + b`` as ``reconstruct``
returns them for the batch repeated chain-major, and returns the (weighted) log-likelihood ``ll (C, B)`` of every decode against the image and
its arg-max map ``seg (C, B, S, S)`` in one launch of ``iodine_chain_score``.  ``chain_consensus`` folds C such maps, relabelled by ``perm (C,
B, K)`` - slot i of chain c is slot ``perm[c, b, i]`` of the common labelling, e.g. ``matching.assign(1 - slot_iou(overlap_table(seg,
seg_of_one_chain, K, K)).float())[0]`` - into per-pixel votes, their arg-max, its share of the chains, each chain's share of pixels that
agree with a reference chain, and the mean relabelled soft mask (``iodine_chain_consensus``).  The kernels are stateless and need no model;
like ``objects.slot_table`` there is no CPU path.  tests/restarts_reference.py is the numpy definition of both.
"""
from __future__ import annotations

import collections

import torch

from . import _args, _lib
from .objects import MAX_SIZE, MAX_SLOTS

MAX_CHAINS = 1024
Consensus = collections.namedtuple('Consensus', 'votes consensus agreement match mask_mean')


def chain_score(x, mask, mean, sigma, weights=None, joint=False, ll=True, segmentation=True):
    """``x (B, 3, S, S)``, ``mask (C, B, K, 1, S, S)``, ``mean (C, B, K, 3, S, S)`` float32 on one ROCm device, ``weights (B, S, S)`` or None
    -> ``(ll (C, B) float32, seg (C, B, S, S) uint8)``, None where not asked for.  ``ll[c, b] = sum_p w_p LL_p`` with ``LL_p = sum_c
    logsumexp_k(log(m_k + 1e-12) + l_kc)`` or, with ``joint``, ``logsumexp_k(log(m_k + 1e-12) + sum_c l_kc)``, ``l_kc`` the Gaussian
    log-density of ``x_c`` around ``mean_kc`` at scale ``sigma``; ``seg = argmax_k mask`` with the lowest index on a tie (the map of
    ``slot_table``).  Bitwise reproducible."""
    tensors = (x, mask, mean) + ((weights,) if weights is not None else ())
    _args.all_tensors(tensors, 'chain_score: x, mask, mean (and weights) must be torch tensors')
    if mask.dim() != 6 or mask.shape[3] != 1 or mask.shape[4] != mask.shape[5]:
        raise ValueError(f'chain_score: mask must be (C, B, K, 1, S, S), got {tuple(mask.shape)}')
    Cn, B, K, S = (int(mask.shape[i]) for i in (0, 1, 2, 5))
    if not 1 <= Cn <= MAX_CHAINS or B < 1 or not 1 <= K <= MAX_SLOTS or not 1 <= S <= MAX_SIZE:
        raise ValueError(f'chain_score: C must be in 1..{MAX_CHAINS}, B >= 1, K in 1..{MAX_SLOTS} and S in 1..{MAX_SIZE}, got mask '
                         f'{tuple(mask.shape)}')
    if tuple(mean.shape) != (Cn, B, K, 3, S, S) or tuple(x.shape) != (B, 3, S, S):
        raise ValueError(f'chain_score: for this mask mean must be {(Cn, B, K, 3, S, S)} and x {(B, 3, S, S)}, got {tuple(mean.shape)} and '
                         f'{tuple(x.shape)}')
    if weights is not None and tuple(weights.shape) != (B, S, S):
        raise ValueError(f'chain_score: weights must be {(B, S, S)}, got {tuple(weights.shape)}')
    if not (ll or segmentation):
        raise ValueError('chain_score: neither ll nor segmentation is asked for')
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError(f'chain_score: sigma must be > 0; got {sigma!r}')
    _args.one_device((mask,) + tensors, 'chain_score needs x, mask, mean (and weights) on one ROCm device (no CPU fallback)')
    dev = mask.device
    xs, mk, mn = (t.detach().to(torch.float32).contiguous() for t in (x, mask, mean))
    w = None if weights is None else weights.detach().to(torch.float32).contiguous()
    out_ll = torch.empty((Cn, B), dtype=torch.float32, device=dev) if ll else None
    seg = torch.empty((Cn, B, S, S), dtype=torch.uint8, device=dev) if segmentation else None
    _lib.call('iodine_chain_score', dev, xs, w, mk, mn, Cn, B, K, S, sigma, int(bool(joint)), out_ll, seg)
    return out_ll, seg


def chain_consensus(seg, perm, ref=None, mask=None):
    """``seg (C, B, S, S)`` uint8, ``perm (C, B, K)`` int32, ``ref (B)`` int32 or None, ``mask (C, B, K, 1, S, S)`` float32 or None ->
    ``Consensus(votes (B, K, S, S) int32, consensus (B, S, S) uint8, agreement (B, S, S), match (C, B) or None without ref, mask_mean (B, K,
    1, S, S) or None without mask)``.  With t_c(p) = perm[c, b, seg[c, b, p]]: ``votes[b, j, p]`` counts the chains with t_c(p) = j,
    ``consensus`` is their arg-max (lowest index on a tie), ``agreement`` its share of the C chains, ``match[c, b]`` the share of pixels with
    t_c = t_ref[b], ``mask_mean[b, j]`` the mean over the chains of the soft mask each maps to j.  A label >= K or a perm / ref entry outside
    its range leaves that pixel (chain) out of every count: the votes then sum to less than C."""
    given = (seg, perm) + tuple(t for t in (ref, mask) if t is not None)
    _args.all_tensors(given, 'chain_consensus: seg, perm (and ref, mask) must be torch tensors')
    if seg.dim() != 4 or seg.dtype != torch.uint8 or seg.shape[2] != seg.shape[3]:
        raise ValueError(f'chain_consensus: seg must be uint8 (C, B, S, S), got {seg.dtype} {tuple(seg.shape)}')
    Cn, B, S = int(seg.shape[0]), int(seg.shape[1]), int(seg.shape[3])
    if perm.dim() != 3 or perm.dtype != torch.int32 or tuple(perm.shape[:2]) != (Cn, B):
        raise ValueError(f'chain_consensus: perm must be int32 ({Cn}, {B}, K), got {perm.dtype} {tuple(perm.shape)}')
    K = int(perm.shape[2])
    if not 1 <= Cn <= MAX_CHAINS or B < 1 or not 1 <= K <= MAX_SLOTS or not 1 <= S <= MAX_SIZE:
        raise ValueError(f'chain_consensus: C must be in 1..{MAX_CHAINS}, B >= 1, K in 1..{MAX_SLOTS} and S in 1..{MAX_SIZE}, got seg '
                         f'{tuple(seg.shape)}, perm {tuple(perm.shape)}')
    if ref is not None and (ref.dtype != torch.int32 or tuple(ref.shape) != (B,)):
        raise ValueError(f'chain_consensus: ref must be int32 ({B},), got {ref.dtype} {tuple(ref.shape)}')
    if mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != (Cn, B, K, 1, S, S)):
        raise ValueError(f'chain_consensus: mask must be float32 {(Cn, B, K, 1, S, S)}, got {mask.dtype} {tuple(mask.shape)}')
    _args.one_device(given, 'chain_consensus needs seg, perm (and ref, mask) on one ROCm device (no CPU fallback)')
    dev = seg.device
    sg, pr = seg.contiguous(), perm.contiguous()
    rf = None if ref is None else ref.contiguous()
    mk = None if mask is None else mask.detach().contiguous()
    votes = torch.empty((B, K, S, S), dtype=torch.int32, device=dev)
    cons = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    agree = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    match = torch.empty((Cn, B), dtype=torch.float32, device=dev) if rf is not None else None
    mmean = torch.empty((B, K, 1, S, S), dtype=torch.float32, device=dev) if mk is not None else None
    _lib.call('iodine_chain_consensus', dev, sg, pr, rf, mk, Cn, B, K, S, votes, cons, agree, match, mmean)
    return Consensus(votes, cons, agree, match, mmean)
