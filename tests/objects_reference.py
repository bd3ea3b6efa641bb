"""Plain torch float64 restatement of ``iodine_slot_table`` and ``iodine_seg_overlap`` (include/iodine_hip.h), shared by
test_objects_cpu.py and test_gpu_objects.py.  Written from the column table of the header, not from the kernel: every sum is one float64
``sum`` over the image, the argmax an explicit loop with a strict ``>`` so that the lowest index wins a tie whatever ``torch.argmax``
does with it."""
import torch

COLUMNS = ('soft_area', 'hard_area', 'soft_cx', 'soft_cy', 'hard_cx', 'hard_cy', 'x0', 'y0', 'x1', 'y1', 'r', 'g', 'b', 'peak')


def segmentation(mask):
    """mask (B, K, 1, S, S) -> (B, S, S) uint8: first maximal slot per pixel (strict >, from -inf upwards: a NaN never wins)."""
    B, K, _, S, _ = mask.shape
    m = mask[:, :, 0]
    best = torch.zeros((B, S, S), dtype=torch.int64)
    bv = torch.full((B, S, S), float('-inf'), dtype=m.dtype)
    for k in range(K):
        upd = m[:, k] > bv
        bv = torch.where(upd, m[:, k], bv)
        best = torch.where(upd, torch.full_like(best, k), best)
    return best.to(torch.uint8)


def slot_table(mask, mean=None):
    """mask (B, K, 1, S, S), mean (B, K, 3, S, S) or None, CPU tensors -> (table (B, K, 14) float64, seg (B, S, S) uint8)."""
    mask = mask.detach().cpu()
    B, K, _, S, _ = mask.shape
    seg = segmentation(mask)
    m = mask[:, :, 0].to(torch.float64)
    col = torch.arange(S, dtype=torch.float64).view(1, 1, 1, S).expand(B, K, S, S)
    row = torch.arange(S, dtype=torch.float64).view(1, 1, S, 1).expand(B, K, S, S)
    t = torch.zeros((B, K, 14), dtype=torch.float64)
    area = m.sum((-1, -2))
    t[..., 0] = area
    safe = torch.where(area == 0, torch.ones_like(area), area)
    used = (area != 0).to(torch.float64)
    t[..., 2] = (m * col).sum((-1, -2)) / safe * used
    t[..., 3] = (m * row).sum((-1, -2)) / safe * used
    if mean is not None:
        c = mean.detach().cpu().to(torch.float64)
        t[..., 10:13] = (m[:, :, None] * c).sum((-1, -2)) / safe[..., None] * used[..., None]
    t[..., 13] = m.amax((-1, -2))
    for b in range(B):
        for k in range(K):
            ys, xs = torch.nonzero(seg[b] == k, as_tuple=True)
            n = int(ys.numel())
            t[b, k, 1] = n
            if n == 0:
                t[b, k, 4:10] = -1.0
                continue
            t[b, k, 4] = float(xs.sum()) / n
            t[b, k, 5] = float(ys.sum()) / n
            t[b, k, 6], t[b, k, 7], t[b, k, 8], t[b, k, 9] = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
    return t, seg


def overlap_table(seg_a, seg_b, ka, kb):
    """(B, ...) uint8 label maps -> (B, ka, kb) int64 counts; a pixel with a label >= ka / >= kb is left out."""
    a = seg_a.detach().cpu().to(torch.int64).flatten(1)
    b = seg_b.detach().cpu().to(torch.int64).flatten(1)
    out = torch.zeros((a.shape[0], ka, kb), dtype=torch.int64)
    for n in range(a.shape[0]):
        keep = (a[n] < ka) & (b[n] < kb)
        out[n] = torch.bincount(a[n][keep] * kb + b[n][keep], minlength=ka * kb).view(ka, kb)
    return out
