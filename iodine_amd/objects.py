"""Object-level read-outs of a decode: per-slot tables, segmentation maps and the overlap of two segmentations.

``slot_table`` turns the soft output of ``reconstruct`` / ``decode`` / a ``trajectory`` entry - ``mask (*, K, 1, S, S)`` and optionally
``mean (*, K, 3, S, S)`` - into one row of ``SLOT_COLUMNS`` per slot and, on request, the argmax segmentation map, in one launch of
``iodine_slot_table``.  ``overlap_table`` counts the co-occurrences of two such maps (``iodine_seg_overlap``): the contingency table
``ari.compute_ari`` takes, between two runs or two frames instead of against ground truth; ``slot_iou`` is the intersection over union
that follows from its row and column sums, and ``matching.assign(1 - slot_iou(overlap_table(a, b, K, K)).float())`` (on the device) is the
slot permutation between the two segmentations - what following the slots from frame to frame needs.  The kernels are stateless and need no model; like ``ari.ari_tables`` there is no CPU path.

``components`` reads a map as objects instead of slots: the connected components of every label (``iodine_seg_components``), numbered as
``scipy.ndimage.label`` numbers them, with their areas, boxes and coordinate sums, the counts per slot, and on request the map with the
components below ``min_area`` absorbed by a neighbour (``clean_segmentation``); ``seg_to_mask`` turns such a map back into a hard mask
for everything that takes masks.  This one has a CPU path (``iodine_seg_components_host``, the same rule, serial).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _args, _lib

# columns of the table, in order (include/iodine_hip.h, iodine_slot_table)
SLOT_COLUMNS = ('soft_area', 'hard_area', 'soft_cx', 'soft_cy', 'hard_cx', 'hard_cy', 'x0', 'y0', 'x1', 'y1', 'r', 'g', 'b', 'peak')
MAX_SLOTS = 16
MAX_SIZE = 1024
# connected components (include/iodine_hip.h, iodine_seg_components): the columns of table, count and per_slot, in order
COMPONENT_COLUMNS = ('slot', 'area', 'sum_col', 'sum_row', 'x0', 'y0', 'x1', 'y1')
COUNT_COLUMNS = ('kept', 'small', 'small_pixels', 'invalid_pixels')
PER_SLOT_COLUMNS = ('kept', 'small', 'largest_area', 'small_pixels')
COMPONENTS_LDS_MAX_SIZE = 128   # IODINE_COMPONENTS_LDS_MAX_SIZE: up to here one block per image holds the parent array in LDS
MAX_COMPONENT_BATCH = 65535     # maps in one device call


class Components(NamedTuple):
    """what ``components`` returns; ``table``, ``area_map`` and ``clean`` are None where they were not asked for"""
    labels: torch.Tensor
    count: torch.Tensor
    per_slot: torch.Tensor
    table: Optional[torch.Tensor]
    area_map: Optional[torch.Tensor]
    clean: Optional[torch.Tensor]


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


def _check_components(seg, slots, connectivity, min_area, max_components, table):
    """host-side checks of ``components``: what the entry point would refuse, as ValueError -> (lead, S, ints)"""
    _args.all_tensors((seg,), 'components: seg must be a torch tensor')
    if seg.dtype != torch.uint8 or seg.dim() < 2 or seg.shape[-1] != seg.shape[-2]:
        raise ValueError(f'components: seg must be uint8 (*, S, S), got {seg.dtype} {tuple(seg.shape)}')
    values = (slots, connectivity, min_area, max_components)
    if any(isinstance(v, bool) or int(v) != v for v in values):
        raise ValueError(f'components: slots, connectivity, min_area and max_components must be integers, got {values!r}')
    slots, connectivity, min_area, max_components = (int(v) for v in values)
    S = int(seg.shape[-1])
    if not 1 <= slots <= MAX_SLOTS or not 1 <= S <= MAX_SIZE:
        raise ValueError(f'components: slots must be in 1..{MAX_SLOTS} and S in 1..{MAX_SIZE}, got slots = {slots}, S = {S}')
    if connectivity not in (4, 8):
        raise ValueError(f'components: connectivity must be 4 or 8, got {connectivity}')
    if min_area < 1:
        raise ValueError(f'components: min_area must be >= 1, got {min_area}')
    if max_components < (1 if table else 0):
        raise ValueError(f'components: max_components must be >= {1 if table else 0}, got {max_components}')
    return tuple(seg.shape[:-2]), S, slots, connectivity, min_area, max_components


def components(seg: torch.Tensor, slots: int, connectivity: int = 4, min_area: int = 1, max_components: int = 64,
               area_map: bool = False, clean: bool = False) -> Components:
    """Connected components of label maps ``seg (*, S, S)`` uint8, as ``slot_table(..., segmentation=True)`` returns them: the rule of
    ``iodine_seg_components`` (include/iodine_hip.h).  A pixel is valid if ``seg < slots``; equal valid 4- / 8-neighbours are joined; a
    component of at least ``min_area`` pixels is kept and numbered in the raster order of its first pixel (as ``scipy.ndimage.label``
    numbers), any other is small.  Returns ``Components``, all int32 on seg's device:

    - ``labels (*, S, S)``: id of the kept component, -1 for small and invalid pixels;
    - ``count (*, 4)``: ``COUNT_COLUMNS``;  ``per_slot (*, slots, 4)``: ``PER_SLOT_COLUMNS``;
    - ``table (*, max_components, 8)``: ``COMPONENT_COLUMNS`` of kept component i in row i, -1 in the rows beyond the kept count
      (``max_components=0``: None); centroids are ``sum_col / area``, ``sum_row / area``;
    - ``area_map (*, S, S)`` with ``area_map=True``: area of the pixel's component, small ones included (else None);
    - ``clean (*, S, S)`` uint8 with ``clean=True``: every small component takes the slot of its largest kept 4-neighbour component (the
      smaller first pixel on a tie; none: unchanged).  One pass, not iterated (else None).

    A device tensor runs ``iodine_seg_components`` on the current stream (one allocation of scratch, no synchronise); a CPU tensor goes
    image by image through ``iodine_seg_components_host``, the same rule."""
    lead, S, slots, connectivity, min_area, M = _check_components(seg, slots, connectivity, min_area, max_components, max_components != 0)
    B = _args.lead_count(lead, f'components: empty leading dimensions {lead}')
    dev = seg.device
    if dev.type not in ('cuda', 'cpu'):
        raise RuntimeError(f'components: seg must be on a ROCm device or on the CPU, got {dev}')
    sg = seg.detach().contiguous()

    def new(*shape, dtype=torch.int32):
        return torch.empty(lead + shape, dtype=dtype, device=dev)
    labels, count, per_slot = new(S, S), new(4), new(slots, 4)
    table = new(M, 8) if M else None
    amap = new(S, S) if area_map else None
    cl = new(S, S, dtype=torch.uint8) if clean else None
    if dev.type == 'cuda':
        if B > MAX_COMPONENT_BATCH:
            raise ValueError(f'components: at most {MAX_COMPONENT_BATCH} maps a call, got {B}')
        nbytes = _lib.fn('iodine_seg_components_scratch_bytes')(B, S)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.call('iodine_seg_components', dev, sg, B, slots, S, connectivity, min_area, M, labels, amap, count, per_slot, table, cl,
                  scratch, nbytes)
    else:
        host = _lib.fn('iodine_seg_components_host')
        flat = [None if t is None else t.view((B,) + tuple(t.shape[len(lead):])) for t in (sg, labels, amap, count, per_slot, table, cl)]
        for b in range(B):
            s, *outs = [None if t is None else _lib.ptr(t[b]) for t in flat]
            _lib.check(host(s, slots, S, connectivity, min_area, M, *outs), None, 'iodine_seg_components_host')
    return Components(labels, count, per_slot, table, amap, cl)


def clean_segmentation(seg: torch.Tensor, slots: int, min_area: int, connectivity: int = 4) -> torch.Tensor:
    """``seg (*, S, S)`` uint8 with every component below ``min_area`` pixels given to its largest kept 4-neighbour component:
    ``components(..., clean=True).clean`` (one pass, see there)."""
    return components(seg, slots, connectivity=connectivity, min_area=min_area, max_components=0, clean=True).clean


def seg_to_mask(seg: torch.Tensor, slots: int) -> torch.Tensor:
    """A label map ``(*, S, S)`` uint8 as a hard mask ``(*, slots, 1, S, S)`` float32, 1 where ``seg == k`` (a pixel ``>= slots`` is 0 in
    every plane): what ``ari_tables``, ``segmentation_scores``, ``slot_table`` and ``figures.sheet`` take.  Plain torch ops."""
    _args.all_tensors((seg,), 'seg_to_mask: seg must be a torch tensor')
    if seg.dtype != torch.uint8 or seg.dim() < 2 or isinstance(slots, bool) or int(slots) != slots or not 1 <= int(slots) <= MAX_SLOTS:
        raise ValueError(f'seg_to_mask: seg must be uint8 (*, S, S) and slots an integer in 1..{MAX_SLOTS}, got {seg.dtype} '
                         f'{tuple(seg.shape)}, slots = {slots!r}')
    k = torch.arange(int(slots), dtype=torch.uint8, device=seg.device).view((int(slots), 1, 1, 1))
    return (seg.unsqueeze(-3).unsqueeze(-3) == k).to(torch.float32)


def slot_iou(table) -> torch.Tensor:
    """Intersection over union of every pair of segments from an overlap table ``(*, ka, kb)``:
    ``t / (rowsum_i + colsum_j - t)`` in float64, 0 where the denominator is 0 (both segments empty)."""
    t = torch.as_tensor(table).to(torch.float64)
    if t.dim() < 2:
        raise ValueError(f'slot_iou: the table must be (*, ka, kb), got {tuple(t.shape)}')
    union = t.sum(-1, keepdim=True) + t.sum(-2, keepdim=True) - t
    return torch.where(union > 0, t / union.clamp_min(1e-300), torch.zeros_like(t))
