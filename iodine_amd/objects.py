"""Object-level read-outs of a decode: per-slot tables, segmentation maps and the overlap of two segmentations.

``slot_table`` turns the soft output of ``reconstruct`` / ``decode`` / a ``trajectory`` entry - ``mask (*, K, 1, S, S)`` and optionally
``mean (*, K, 3, S, S)`` - into one row of ``SLOT_COLUMNS`` per slot and, on request, the argmax segmentation map, in one launch of
``iodine_slot_table``.  ``overlap_table`` counts the co-occurrences of two such maps (``iodine_seg_overlap``): the contingency table
``ari.compute_ari`` takes, between two runs or two frames instead of against ground truth; ``slot_iou`` is the intersection over union
that follows from its row and column sums, and ``matching.assign(1 - slot_iou(overlap_table(a, b, K, K)).float())`` (on the device) is the
slot permutation between the two segmentations - what following the slots from frame to frame needs.  The kernels are stateless and need no model; like ``ari.ari_tables`` there is no CPU path.
"""
from __future__ import annotations

import torch

from . import _args, _lib

# columns of the table, in order (include/iodine_hip.h, iodine_slot_table)
SLOT_COLUMNS = ('soft_area', 'hard_area', 'soft_cx', 'soft_cy', 'hard_cx', 'hard_cy', 'x0', 'y0', 'x1', 'y1', 'r', 'g', 'b', 'peak')
MAX_SLOTS = 16
MAX_SIZE = 1024


def slot_table(mask: torch.Tensor, mean=None, segmentation: bool = False):
    """``mask (*, K, 1, S, S)``, ``mean (*, K, 3, S, S)`` or None -> ``table (*, K, 14)`` float32 on the device, columns ``SLOT_COLUMNS``;
    with ``segmentation=True`` the pair ``(table, seg (*, S, S) uint8)``, ``seg = argmax_K mask`` with the lowest index winning a tie.
    Any leading dimensions: ``(B, ...)`` or the ``(T + 1, B, ...)`` of a trajectory.  Empty slots read ``hard_area`` 0 and -1 in the hard
    centroid and the box; without ``mean`` the colour columns are 0."""
    given = (mask,) if mean is None else (mask, mean)
    _args.all_tensors(given, 'slot_table: mask (and mean) must be torch tensors')
    _args.one_device(given, 'slot_table needs mask (and mean) on one ROCm device (no CPU fallback)')
    if mask.dim() < 4 or mask.shape[-3] != 1 or mask.shape[-1] != mask.shape[-2]:
        raise ValueError(f'slot_table: mask must be (*, K, 1, S, S), got {tuple(mask.shape)}')
    lead, K, S = tuple(mask.shape[:-4]), int(mask.shape[-4]), int(mask.shape[-1])
    if not 1 <= K <= MAX_SLOTS or not 1 <= S <= MAX_SIZE:
        raise ValueError(f'slot_table: K must be in 1..{MAX_SLOTS} and S in 1..{MAX_SIZE}, got K = {K}, S = {S}')
    if mean is not None and tuple(mean.shape) != lead + (K, 3, S, S):
        raise ValueError(f'slot_table: mean must be {lead + (K, 3, S, S)} for this mask, got {tuple(mean.shape)}')
    B = _args.lead_count(lead, f'slot_table: empty leading dimensions {lead}')
    dev = mask.device
    mk = mask.detach().to(torch.float32).contiguous()
    mn = None if mean is None else mean.detach().to(torch.float32).contiguous()
    table = torch.empty(lead + (K, len(SLOT_COLUMNS)), dtype=torch.float32, device=dev)
    seg = torch.empty(lead + (S, S), dtype=torch.uint8, device=dev) if segmentation else None
    _lib.call('iodine_slot_table', dev, mk, mn, B, K, S, table, seg)
    return (table, seg) if segmentation else table


def overlap_table(seg_a: torch.Tensor, seg_b: torch.Tensor, ka: int, kb: int) -> torch.Tensor:
    """Two label maps ``(*, S, S)`` uint8 of one shape, as ``slot_table`` returns them -> ``(*, ka, kb)`` int32 on the device,
    ``[..., i, j] = #{p : seg_a = i and seg_b = j}``.  The last two dimensions are always the pixels of one map (a flat ``(B, P)`` map goes
    in as ``(B, 1, P)``).  Pixels labelled ``>= ka`` in ``seg_a`` or ``>= kb`` in ``seg_b`` are left out."""
    _args.all_tensors((seg_a, seg_b), 'overlap_table: seg_a and seg_b must be torch tensors')
    _args.one_device((seg_a, seg_b), 'overlap_table needs both maps on one ROCm device (no CPU fallback)')
    if seg_a.dtype != torch.uint8 or seg_b.dtype != torch.uint8:
        raise ValueError(f'overlap_table: the maps must be uint8, got {seg_a.dtype} and {seg_b.dtype}')
    if seg_a.shape != seg_b.shape or seg_a.dim() < 2:
        raise ValueError(f'overlap_table: the maps must be (*, S, S) of one shape, got {tuple(seg_a.shape)} and {tuple(seg_b.shape)}')
    ka, kb = int(ka), int(kb)
    if not 1 <= ka <= MAX_SLOTS or not 1 <= kb <= MAX_SLOTS:
        raise ValueError(f'overlap_table: ka and kb must be in 1..{MAX_SLOTS}, got {ka}, {kb}')
    lead = tuple(seg_a.shape[:-2])
    P = int(seg_a.shape[-2]) * int(seg_a.shape[-1])
    few = f'overlap_table: need at least one map of 1..{MAX_SIZE * MAX_SIZE} pixels, got {tuple(seg_a.shape)}'
    B = _args.lead_count(lead, few)
    if not 1 <= P <= MAX_SIZE * MAX_SIZE:
        raise ValueError(few)
    a, b = seg_a.contiguous(), seg_b.contiguous()
    table = torch.empty(lead + (ka, kb), dtype=torch.int32, device=a.device)
    _lib.call('iodine_seg_overlap', a.device, a, b, B, ka, kb, P, table)
    return table


def slot_iou(table) -> torch.Tensor:
    """Intersection over union of every pair of segments from an overlap table ``(*, ka, kb)``:
    ``t / (rowsum_i + colsum_j - t)`` in float64, 0 where the denominator is 0 (both segments empty)."""
    t = torch.as_tensor(table).to(torch.float64)
    if t.dim() < 2:
        raise ValueError(f'slot_iou: the table must be (*, ka, kb), got {tuple(t.shape)}')
    union = t.sum(-1, keepdim=True) + t.sum(-2, keepdim=True) - t
    return torch.where(union > 0, t / union.clamp_min(1e-300), torch.zeros_like(t))
