"""ARI evaluation with the argmax + contingency table computed on the device.

Mirrors ``ARIEvaluator`` (lib/eval/ari_eval.py:7-46) and ``compute_ari`` (lib/utils/ari.py:6-33): the model's soft
masks are binarised by argmax over K, the (N_gt x K) table of pixel co-occurrences is built with int32 atomics by
``iodine_ari_table``, and the pair-count formula on that tiny integer table is evaluated on the host in float64
(``n choose 2 = n (n - 1) / 2`` is exact at these magnitudes, like ``scipy.special.comb``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def compute_ari(table) -> float:
    """lib/utils/ari.py:6-33."""
    t = np.asarray(table, dtype=np.float64)
    c2 = lambda v: v * (v - 1.0) / 2.0
    a, b = t.sum(axis=1), t.sum(axis=0)
    n = a.sum()
    ca, cb, cn, ct = c2(a).sum(), c2(b).sum(), c2(n), c2(t).sum()
    if cb == ca == cn == ct:
        return 1.0
    return float((ct - ca * cb / cn) / (0.5 * (ca + cb) - (ca * cb) / cn))


def ari_tables(mask: torch.Tensor, gt_masks) -> np.ndarray:
    """mask (B,K,1,S,S) on the device, gt_masks: list of (N_b, S, S) 0/1 arrays -> int tables (B, G, K), G = max N_b; or gt_masks already
    packed - a (B, G, S, S) uint8 tensor on the mask's device (``pack_gt``, a ``ResidentDataset`` batch), used as it is: no host pass."""
    if mask.device.type != 'cuda':
        raise RuntimeError('ari_tables needs the masks on a ROCm device (no CPU fallback)')
    B, K, _, S, _ = mask.shape
    if isinstance(gt_masks, torch.Tensor):
        if gt_masks.dtype != torch.uint8 or tuple(gt_masks.shape[:1] + gt_masks.shape[2:]) != (B, S, S) or gt_masks.device != mask.device:
            raise ValueError(f'ari_tables: packed masks must be uint8 ({B}, G, {S}, {S}) on {mask.device}, got {gt_masks.dtype} '
                             f'{tuple(gt_masks.shape)} on {gt_masks.device}')
        gt, G = gt_masks.contiguous(), int(gt_masks.shape[1])
    else:
        G = max(int(m.shape[0]) for m in gt_masks)
        gt = torch.zeros((B, G, S, S), dtype=torch.uint8)
        for b, m in enumerate(gt_masks):
            gt[b, :m.shape[0]] = torch.as_tensor(np.asarray(m)).to(torch.uint8)
        gt = gt.to(mask.device)
    table = torch.empty((B, G, K), dtype=torch.int32, device=mask.device)
    mk = mask.detach().to(torch.float32).contiguous()
    _lib.call('iodine_ari_table', mask.device, mk, gt, B, K, G, S * S, table)
    return table.cpu().numpy()


def gt_counts(data):
    """masks per image of a batch (image, gt_masks[, counts]): from the per-image list, or - with packed masks (B, G, S, S) - the third entry
    (a ``ResidentDataset`` batch carries it); an image's ARI and scores use its first ``counts[b]`` rows"""
    if isinstance(data[1], torch.Tensor):
        if len(data) < 3:
            raise ValueError('packed ground-truth masks (B, G, S, S) need the per-image counts as a third entry of the batch')
        return [int(n) for n in data[2]]
    return [int(m.shape[0]) for m in data[1]]


class ARIEvaluator:
    """Same protocol as lib/eval/base.py:1-11 / lib/eval/ari_eval.py:7-46: evaluate(model, data), reset(), get_results().  ``data`` is
    (image, list of masks) or (image, packed masks (B, G, S, S) uint8 on the device, counts (B,))."""

    def __init__(self):
        self.aris = []

    def evaluate(self, model, data):
        image, gt_masks = data[0], data[1]
        pred, pred_mask, mean = model.reconstruct(image)
        tables = ari_tables(pred_mask, gt_masks)
        for b, n in enumerate(gt_counts(data)):
            self.aris.append(compute_ari(tables[b, :n]))

    def reset(self):
        self.aris = []

    def get_results(self):
        return 'Ari: {}'.format(np.mean(self.aris) if self.aris else 0)
