"""Slots matched to ground-truth masks: the assignment, a supervised mask loss, matched mIoU and segmentation covering.

The K slots are exchangeable, so anything that compares ``mask (*, K, 1, S, S)`` with ground-truth object masks ``gt (*, G, S, S)`` first needs
a minimum-cost assignment of objects to slots per image.  Three launches do all of it on the device (include/iodine_hip.h,
``iodine_mask_overlap`` / ``iodine_mask_match`` / ``iodine_mask_match_backward``): one pass over the pixels for the overlap statistics, one
tiny pass for costs, assignment, per-image loss and backward coefficients, one pass over the pixels for the gradient.  Nothing synchronises
and nothing is copied to the host.

* ``pack_gt`` turns the loader's per-image tuple of ``(N_b, S, S)`` masks into ``(B, G, S, S)`` uint8 on the device.  A row without pixels
  is padding wherever it sits (the convention of ``ari.ari_tables``).
* ``overlap`` returns the statistics, ``assign`` solves any ``(*, G, K)`` cost on the device, ``match_masks`` both plus cost and IoU.
* ``matched_mask_loss`` is one ``torch.autograd.Function``: ``model(x, attach_state=True)`` leaves ``model.mask`` attached, and
  ``loss + w * matched_mask_loss(model.mask, gt)`` trains with one ``backward()``.  The assignment is a constant of the gradient.
* ``segmentation_scores`` / ``SegmentationEvaluator``: matched mIoU, segmentation covering (SC) and its unweighted mean (mSC) from the
  hard tables of ``iodine_ari_table`` and ``objects.slot_table``, beside the ARI of ``ari.ARIEvaluator``.

Cost kinds: ``'iou'`` = 1 - I / (n + a - I), ``'ce'`` = N / n with I = sum gt m, a = sum m, n = sum gt, N = -sum gt log(m + eps).  Like
the other stateless kernels there is no CPU path."""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _args, _lib
from .ari import compute_ari
from .objects import MAX_SIZE, MAX_SLOTS, SLOT_COLUMNS, slot_table

KINDS = {'iou': 0, 'ce': 1}
Overlap = collections.namedtuple('Overlap', 'inter nll mask_area gt_area')
Match = collections.namedtuple('Match', 'assign cost iou stats')
Scores = collections.namedtuple('Scores', 'miou sc msc')


def _kind(name, what):
    if name not in KINDS:
        raise ValueError(f"{what} must be 'iou' or 'ce'; got {name!r}")
    return KINDS[name]


def _eps(eps, who):
    eps = float(eps)
    if not eps > 0.0:
        raise ValueError(f'{who}: eps must be > 0; got {eps!r}')
    return eps


def _check_pair(mask, gt, who):
    """(lead, B, K, G, S) of ``mask (*, K, 1, S, S)`` float32 and ``gt (*, G, S, S)`` uint8 on one ROCm device"""
    _args.all_tensors((mask, gt), f'{who}: mask and gt must be torch tensors (pack_gt packs the loader\'s tuple)')
    _args.one_device((mask, gt), f'{who} needs mask and gt on one ROCm device (no CPU fallback)')
    if mask.dim() < 5 or mask.shape[-3] != 1 or mask.shape[-1] != mask.shape[-2]:
        raise ValueError(f'{who}: mask must be (*, K, 1, S, S) with at least one leading dimension, got {tuple(mask.shape)}')
    if mask.dtype != torch.float32:
        raise ValueError(f'{who}: mask must be float32, got {mask.dtype}')
    if gt.dtype != torch.uint8:
        raise ValueError(f'{who}: gt must be uint8 0/1 (pack_gt), got {gt.dtype}')
    lead, K, S = tuple(mask.shape[:-4]), int(mask.shape[-4]), int(mask.shape[-1])
    if gt.dim() != len(lead) + 3 or tuple(gt.shape[:-3]) != lead or tuple(gt.shape[-2:]) != (S, S):
        raise ValueError(f'{who}: gt must be {lead + ("G", S, S)} for this mask, got {tuple(gt.shape)}')
    G = int(gt.shape[-3])
    if not 1 <= K <= MAX_SLOTS or not 1 <= G <= MAX_SLOTS or not 1 <= S <= MAX_SIZE:
        raise ValueError(f'{who}: K and G must be in 1..{MAX_SLOTS} and S in 1..{MAX_SIZE}, got K = {K}, G = {G}, S = {S}')
    return lead, _args.lead_count(lead, f'{who}: empty leading dimensions {lead}'), K, G, S


def pack_gt(gt_masks, size=None, device=None):
    """The loader's masks -> ``(B, G, S, S)`` uint8 on ``device``, G = max(1, max N_b), rows beyond an image's N_b zero.  ``gt_masks``: a
    tuple / list with one ``(N_b, S, S)`` array or tensor per image (any dtype, non-zero = inside), where an entry may be ``None`` or have
    N_b = 0 - an unlabelled image, whose rows are all padding; or a 4-D tensor, which is passed through (as uint8, on ``device``).  ``size``:
    S, needed when no entry carries it.  The packing runs on the host; one copy goes to the device."""
    if isinstance(gt_masks, torch.Tensor):
        if gt_masks.dim() != 4:
            raise ValueError(f'pack_gt: a tensor must be (B, G, S, S), got {tuple(gt_masks.shape)}')
        out = gt_masks if gt_masks.dtype == torch.uint8 else (gt_masks != 0).to(torch.uint8)
        return out.to(device) if device is not None else out
    items = []
    for m in gt_masks:
        if m is None:
            items.append(None)
            continue
        t = torch.as_tensor(np.asarray(m)) if not isinstance(m, torch.Tensor) else m.detach().cpu()
        if t.dim() != 3 or t.shape[-1] != t.shape[-2]:
            raise ValueError(f'pack_gt: every entry must be (N, S, S) or None, got {tuple(t.shape)}')
        items.append(t)
    if not items:
        raise ValueError('pack_gt: no images')
    sizes = {int(t.shape[-1]) for t in items if t is not None} | ({int(size)} if size is not None else set())
    if len(sizes) != 1:
        raise ValueError(f'pack_gt: need one image size S (from the masks or size=), got {sorted(sizes)}')
    S = sizes.pop()
    G = max([1] + [int(t.shape[0]) for t in items if t is not None])
    if G > MAX_SLOTS:
        raise ValueError(f'pack_gt: at most {MAX_SLOTS} masks per image, got {G}')
    out = torch.zeros((len(items), G, S, S), dtype=torch.uint8)
    for b, t in enumerate(items):
        if t is not None and t.shape[0]:
            out[b, :t.shape[0]] = (t != 0).to(torch.uint8)
    return out.to(device) if device is not None else out


def _overlap(mk, g8, B, K, G, S, eps, nll):
    dev = mk.device
    inter = torch.empty((B, G, K), dtype=torch.float32, device=dev)
    nl = torch.empty((B, G, K), dtype=torch.float32, device=dev) if nll else None
    area = torch.empty((B, K), dtype=torch.float32, device=dev)
    n = torch.empty((B, G), dtype=torch.int32, device=dev)
    _lib.call('iodine_mask_overlap', dev, mk, g8, B, K, G, S, eps, inter, nl, area, n)
    return inter, nl, area, n


def _match(stats, B, K, G, match_kind, loss_kind, want_cost):
    inter, nl, area, n = stats
    dev = inter.device
    asg = torch.empty((B, G), dtype=torch.int32, device=dev)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    coef = torch.empty((B, G, 2), dtype=torch.float32, device=dev)
    cost = torch.empty((B, G, K), dtype=torch.float32, device=dev) if want_cost else None
    iou = torch.empty((B, G, K), dtype=torch.float32, device=dev) if want_cost else None
    _lib.call('iodine_mask_match', dev, inter, nl, area, n, B, K, G, match_kind, loss_kind, asg, loss, coef, cost, iou)
    return asg, loss, coef, cost, iou


def overlap(mask, gt, eps=1e-6, nll=True):
    """``mask (*, K, 1, S, S)`` float32, ``gt (*, G, S, S)`` uint8 -> ``Overlap(inter (*, G, K), nll (*, G, K) or None, mask_area (*, K),
    gt_area (*, G) int32)`` on the device, in one launch that reads every mask plane once.  Bitwise reproducible."""
    lead, B, K, G, S = _check_pair(mask, gt, 'overlap')
    inter, nl, area, n = _overlap(mask.detach().contiguous(), gt.contiguous(), B, K, G, S, _eps(eps, 'overlap'), bool(nll))
    return Overlap(inter.view(lead + (G, K)), None if nl is None else nl.view(lead + (G, K)), area.view(lead + (K,)), n.view(lead + (G,)))


def assign(cost, row_valid=None):
    """Minimum-cost assignment of rows to columns of any ``cost (*, G, K)`` on the device, G, K <= 16: ``(assign (*, G) int32, total (*,)
    float32)``.  ``row_valid (*, G)``: rows that are 0 / False are padding; with M = min(real rows, K), exactly M real rows get distinct
    columns, every other row reads -1, and ``total`` is the sum of the matched costs.  A matrix with a NaN / inf in a real row is refused:
    all -1 and a NaN total.  ``assign(1 - slot_iou(overlap_table(a, b, K, K)).float())`` is the slot permutation between two
    segmentations."""
    if not isinstance(cost, torch.Tensor):
        raise ValueError('assign: cost must be a torch tensor')
    if cost.device.type != 'cuda' or (isinstance(row_valid, torch.Tensor) and row_valid.device != cost.device):
        raise RuntimeError('assign needs cost (and row_valid) on one ROCm device (no CPU fallback)')
    if cost.dim() < 2 or cost.dtype != torch.float32:
        raise ValueError(f'assign: cost must be float32 (*, G, K), got {cost.dtype} {tuple(cost.shape)}')
    lead, G, K = tuple(cost.shape[:-2]), int(cost.shape[-2]), int(cost.shape[-1])
    if not 1 <= G <= MAX_SLOTS or not 1 <= K <= MAX_SLOTS:
        raise ValueError(f'assign: G and K must be in 1..{MAX_SLOTS}, got {G}, {K}')
    B = _args.lead_count(lead, f'assign: empty leading dimensions {lead}')
    rv = None
    if row_valid is not None:
        if not isinstance(row_valid, torch.Tensor) or tuple(row_valid.shape) != lead + (G,):
            raise ValueError(f'assign: row_valid must be a tensor {lead + (G,)}, got {getattr(row_valid, "shape", row_valid)!r}')
        rv = (row_valid != 0).to(torch.uint8).contiguous()
    c = cost.detach().contiguous()
    asg = torch.empty(lead + (G,), dtype=torch.int32, device=c.device)
    total = torch.empty(lead, dtype=torch.float32, device=c.device)
    _lib.call('iodine_assign', c.device, c, rv, B, G, K, asg, total)
    return asg, total


def match_masks(mask, gt, cost='iou', eps=1e-6):
    """``Match(assign (*, G) int32, cost (*, G, K), iou (*, G, K), stats)``: the assignment that minimises ``cost`` ('iou' or 'ce') between
    ground-truth rows and slots, the cost it minimised, the soft IoU I / (n + a - I) and the ``Overlap`` statistics.  Padding rows read -1
    in ``assign`` and 0 in ``cost`` / ``iou``."""
    kind = _kind(cost, 'match_masks: cost')
    lead, B, K, G, S = _check_pair(mask, gt, 'match_masks')
    stats = _overlap(mask.detach().contiguous(), gt.contiguous(), B, K, G, S, _eps(eps, 'match_masks'), kind == 1)
    asg, _, _, c, iou = _match(stats, B, K, G, kind, kind, True)
    inter, nl, area, n = stats
    st = Overlap(inter.view(lead + (G, K)), None if nl is None else nl.view(lead + (G, K)), area.view(lead + (K,)), n.view(lead + (G,)))
    return Match(asg.view(lead + (G,)), c.view(lead + (G, K)), iou.view(lead + (G, K)), st)


class _MatchedMaskLoss(torch.autograd.Function):
    """per-image loss (B,) and the assignment (B, G); backward = one launch of iodine_mask_match_backward"""

    @staticmethod
    def forward(ctx, mask, gt, loss_kind, match_kind, eps, dims):
        B, K, G, S = dims
        mk = mask.detach().contiguous()
        stats = _overlap(mk, gt, B, K, G, S, eps, loss_kind == 1 or match_kind == 1)
        asg, loss, coef, _, _ = _match(stats, B, K, G, match_kind, loss_kind, False)
        ctx.save_for_backward(mk, gt, asg, coef)
        ctx.args = (dims, loss_kind, eps, mask.shape)
        ctx.mark_non_differentiable(asg)
        return loss, asg

    @staticmethod
    def backward(ctx, grad_loss, _grad_assign):
        mk, gt, asg, coef = ctx.saved_tensors
        (B, K, G, S), loss_kind, eps, shape = ctx.args
        gl = grad_loss.detach().to(torch.float32).contiguous()
        grad = torch.empty(shape, dtype=torch.float32, device=mk.device)
        _lib.call('iodine_mask_match_backward', mk.device, mk, gt, asg, coef, gl, B, K, G, S, loss_kind, eps, grad)
        return grad, None, None, None, None, None


def matched_mask_loss(mask, gt, loss='ce', match='iou', eps=1e-6, reduction='mean'):
    """Supervised mask loss under the minimum-cost assignment of ground-truth rows to slots.  ``mask (*, K, 1, S, S)``: ``model.mask`` after
    ``model(x, attach_state=True)``, or ``model.frames['mask'] (F, B, K, 1, S, S)`` with ``gt (F, B, G, S, S)``; leading dimensions are
    flattened.  Per image l_b = mean over the M matched rows of the ``loss`` value of (row, slot) - 'ce': N / n, 'iou': 1 - I / U - and 0 for
    an image without a real row; ``match`` picks the cost the assignment minimises, independently.  ``reduction='mean'``: sum l_b / B (an
    unlabelled image contributes 0), ``'none'``: l of shape ``lead``.  The gradient reaches ``mask`` only, with the assignment held constant;
    slots that are no row's match get exactly 0.  The result carries ``.assign (*, G)`` int32, detached.  Forward = two launches, backward
    = one; nothing synchronises."""
    lk, mk = _kind(loss, 'matched_mask_loss: loss'), _kind(match, 'matched_mask_loss: match')
    if reduction not in ('mean', 'none'):
        raise ValueError(f"matched_mask_loss: reduction must be 'mean' or 'none'; got {reduction!r}")
    lead, B, K, G, S = _check_pair(mask, gt, 'matched_mask_loss')
    per, asg = _MatchedMaskLoss.apply(mask, gt.contiguous(), lk, mk, _eps(eps, 'matched_mask_loss'), (B, K, G, S))
    out = per.mean() if reduction == 'mean' else per.view(lead)
    out.assign = asg.view(lead + (G,))
    return out


def _hard_tables(mask, gt):
    """(T (B, G, K) int64, hard_area (B, K) float64) on the host from the existing hard kernels"""
    lead, B, K, G, S = _check_pair(mask, gt, 'segmentation_scores')
    mk, g8 = mask.detach().contiguous(), gt.contiguous()
    table = torch.empty((B, G, K), dtype=torch.int32, device=mk.device)
    _lib.call('iodine_ari_table', mk.device, mk, g8, B, K, G, S * S, table)
    hard = slot_table(mk.view(B, K, 1, S, S))[..., SLOT_COLUMNS.index('hard_area')]
    return table.cpu().to(torch.int64), hard.cpu().to(torch.float64)


def scores_from_tables(table, hard_area, device):
    """``Scores`` from the hard contingency tables ``table (B, G, K)`` (``ari.ari_tables``) and ``hard_area (B, K)``: the arithmetic of
    ``segmentation_scores``; only the assignment runs on ``device``."""
    T = torch.as_tensor(np.asarray(table)).to(torch.float64)
    h = torch.as_tensor(np.asarray(hard_area)).to(torch.float64)
    n = T.sum(-1)                                                            # every pixel has an arg-max slot
    union = n[..., None] + h[:, None, :] - T
    iou = torch.where(union > 0, T / union.clamp_min(1.0), torch.zeros_like(T))
    real = n > 0
    asg, _ = assign((1.0 - iou).to(torch.float32).to(device), real.to(device))
    asg = asg.cpu().long()
    picked = torch.gather(iou, 2, asg.clamp_min(0)[..., None])[..., 0] * (asg >= 0)
    best = iou.max(-1).values * real
    nr = real.sum(-1).to(torch.float64)
    nan = torch.full_like(nr, float('nan'))
    some = nr > 0
    miou = torch.where(some, picked.sum(-1) / nr.clamp_min(1.0), nan)
    msc = torch.where(some, best.sum(-1) / nr.clamp_min(1.0), nan)
    sc = torch.where(some, (n * best).sum(-1) / n.sum(-1).clamp_min(1.0), nan)
    return Scores(miou.numpy(), sc.numpy(), msc.numpy())


def segmentation_scores(mask, gt):
    """Per-image ``Scores(miou, sc, msc)`` (float64 numpy, host) of the arg-max segmentation of ``mask (B, K, 1, S, S)`` against
    ``gt (B, G, S, S)``, from the hard tables: T = the contingency table of ``iodine_ari_table``, h_k = ``hard_area`` of ``slot_table``,
    IoU_gk = T_gk / (n_g + h_k - T_gk) over the real rows R (n_g > 0).  mIoU = (1 / |R|) sum_g IoU_{g, pi(g)} with pi = ``assign(1 - IoU)``
    and unmatched rows counting 0; mSC = (1 / |R|) sum_g max_k IoU_gk; SC = sum_g n_g max_k IoU_gk / sum_g n_g.  An image without a real
    row has no score: its entries are NaN and the evaluator's means leave it out."""
    T, h = _hard_tables(mask, gt)
    return scores_from_tables(T, h, mask.device)


class SegmentationEvaluator:
    """``ARIEvaluator``'s protocol (evaluate / reset / get_results) with matched mIoU, SC and mSC beside the ARI: ``aris`` is computed exactly
    as ``ARIEvaluator`` computes it, ``mious`` / ``scs`` / ``mscs`` hold one entry per image (NaN for an image without a real row, which the
    means leave out).  ``per_image`` names the lists ``engine.evaluate`` trims and reduces over ranks."""
    per_image = ('aris', 'mious', 'scs', 'mscs')

    def __init__(self):
        self.reset()

    def evaluate(self, model, data):
        from .ari import ari_tables, gt_counts
        image, gt_masks = data[0], data[1]
        pred, pred_mask, mean = model.reconstruct(image)
        tables = ari_tables(pred_mask, gt_masks)
        for b, n in enumerate(gt_counts(data)):
            self.aris.append(compute_ari(tables[b, :n]))
        hard = slot_table(pred_mask)[..., SLOT_COLUMNS.index('hard_area')].cpu()
        s = scores_from_tables(tables, hard, pred_mask.device)
        self.mious.extend(s.miou.tolist()); self.scs.extend(s.sc.tolist()); self.mscs.extend(s.msc.tolist())

    def reset(self):
        self.aris, self.mious, self.scs, self.mscs = [], [], [], []

    @staticmethod
    def _mean(v):
        v = [x for x in v if x == x]
        return float(np.mean(v)) if v else 0

    def get_results(self):
        return 'Ari: {}, mIoU: {}, SC: {}, mSC: {}'.format(np.mean(self.aris) if self.aris else 0, self._mean(self.mious),
                                                           self._mean(self.scs), self._mean(self.mscs))
