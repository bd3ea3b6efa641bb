"""Float64 restatement of iodine_amd.matching (include/iodine_hip.h, iodine_mask_overlap / iodine_assign / iodine_mask_match /
iodine_mask_match_backward) in plain torch on the host: statistics, the two cost kinds, a brute-force assignment, the matched loss with
its autograd gradient, and the hard-table scores.  ``m + eps`` is rounded to fp32 before the float64 log, so the device's add is the same
number and only the log differs."""
import itertools

import numpy as np
import torch

KINDS = ('iou', 'ce')


def planted(B, K, G, S, seed, empty_rows=(), empty_images=()):
    """Planted inputs: ``gt`` a random partition of the image into G regions plus background, ``mask = softmax_K(randn + 2 gt_i)`` with
    every object planted on a random slot (distinct slots while they last).  ``empty_rows``: rows zeroed in every image (padding in the
    middle); ``empty_images``: images without any object.  Returns (mask (B, K, 1, S, S) float32, gt (B, G, S, S) uint8)."""
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, G + 1, (B, S, S), generator=g)                 # G = background
    gt = torch.stack([(label == i) for i in range(G)], 1)
    for r in empty_rows:
        gt[:, r] = False
    for b in empty_images:
        gt[b] = False
    logits = torch.randn(B, K, S, S, generator=g)
    for b in range(B):
        perm = torch.randperm(K, generator=g)
        for i in range(G):
            k = int(perm[i % K])
            logits[b, k] += 2.0 * gt[b, i].float()
    mask = torch.softmax(logits, 1).unsqueeze(2).contiguous()
    return mask, gt.to(torch.uint8).contiguous()


def stats(mask, gt, eps=1e-6):
    """(inter (B, G, K), nll (B, G, K), mask_area (B, K), gt_area (B, G) int64) in float64; ``mask`` may require grad (float64 then)"""
    m = mask[:, :, 0].to(torch.float64)                                      # (B, K, S, S)
    t = (gt != 0).to(torch.float64)
    a32 = (mask[:, :, 0].detach().to(torch.float32) + torch.tensor(eps, dtype=torch.float32)).to(torch.float64)
    arg = m + (a32 - m.detach())                                             # the value of the fp32 add, the gradient of m + eps
    inter = torch.einsum('bgyx,bkyx->bgk', t, m)
    nll = -torch.einsum('bgyx,bkyx->bgk', t, torch.log(arg))
    return inter, nll, m.sum((-1, -2)), (gt != 0).sum((-1, -2)).to(torch.int64)


def pair_values(kind, inter, nll, area, n):
    """(B, G, K) float64 of kind 'iou' / 'ce'; padding rows (n = 0) hold 0"""
    nn = n.to(torch.float64)[..., None]
    safe = nn.clamp_min(1.0)
    if kind == 'iou':
        v = 1.0 - inter / (safe + area[:, None, :] - inter)
    else:
        v = nll / safe
    return torch.where(nn > 0, v, torch.zeros_like(v))


def brute_force(cost, valid=None):
    """Exhaustive minimum over injective maps of exactly M = min(|R|, K) real rows to columns, G, K <= 6.  ``cost`` (G, K) array.
    Returns (assign list of length G, best total, gap to the second-best total - inf when there is only one candidate)."""
    c = np.asarray(cost, dtype=np.float64)
    G, K = c.shape
    real = [g for g in range(G) if valid is None or valid[g]]
    M = min(len(real), K)
    totals = []
    for rows in itertools.combinations(real, M):
        for cols in itertools.permutations(range(K), M):
            totals.append((sum(c[r, k] for r, k in zip(rows, cols)), rows, cols))
    totals.sort(key=lambda t: t[0])
    best = totals[0]
    assign = [-1] * G
    for r, k in zip(best[1], best[2]):
        assign[r] = k
    gap = totals[1][0] - best[0] if len(totals) > 1 else float('inf')
    return assign, float(best[0]), float(gap)


def matched_loss(kind, inter, nll, area, n, assign):
    """per-image loss (B,) float64 with ``assign`` (B, G) held fixed (differentiable through the statistics)"""
    L = pair_values(kind, inter, nll, area, n)
    a = torch.as_tensor(assign).long()
    on = (a >= 0).to(torch.float64)
    picked = torch.gather(L, 2, a.clamp_min(0)[..., None])[..., 0] * on
    M = on.sum(-1)
    return torch.where(M > 0, picked.sum(-1) / M.clamp_min(1.0), torch.zeros_like(M))


def loss_and_grad(mask, gt, assign, kind, eps=1e-6, grad_loss=None):
    """(per-image loss (B,), d sum_b grad_loss_b loss_b / d mask (B, K, 1, S, S)) in float64 through autograd"""
    m = mask.detach().to(torch.float64).requires_grad_(True)
    per = matched_loss(kind, *stats(m, gt, eps), assign)
    w = torch.ones_like(per) if grad_loss is None else grad_loss.to(torch.float64)
    grad, = torch.autograd.grad((per * w).sum(), m)
    return per.detach(), grad


def hard_scores(mask, gt):
    """per-image (miou, sc, msc) float64 lists from the arg-max segmentation (lowest index on a tie), NaN without a real row; the matching
    is the brute force on 1 - IoU"""
    B, K = mask.shape[:2]
    seg = mask[:, :, 0].argmax(1)
    out = []
    for b in range(B):
        t = (gt[b] != 0)
        n = t.sum((-1, -2)).double()
        real = [g for g in range(t.shape[0]) if n[g] > 0]
        if not real:
            out.append((float('nan'),) * 3)
            continue
        hard = torch.stack([(seg[b] == k) for k in range(K)])
        T = (t[:, None] & hard[None]).sum((-1, -2)).double()
        h = hard.sum((-1, -2)).double()
        iou = T / (n[:, None] + h[None] - T).clamp_min(1.0)
        a, _, _ = brute_force((1.0 - iou).numpy(), [bool(n[g] > 0) for g in range(t.shape[0])])
        miou = sum(float(iou[g, a[g]]) for g in real if a[g] >= 0) / len(real)
        best = iou.max(1).values
        msc = float(sum(best[g] for g in real)) / len(real)
        sc = float(sum(n[g] * best[g] for g in real) / sum(n[g] for g in real))
        out.append((miou, sc, msc))
    return out
