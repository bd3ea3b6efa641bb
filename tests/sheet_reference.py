"""Float32 numpy restatement of the decomposition sheet (include/iodine_hip.h, iodine_render_sheet): the bytes the GPU tests compare
against.  Plain loops over rows and panels, array ops inside a panel; every multiply, add, subtract and divide is one float32 numpy
operation, so nothing is fused.  Reads nothing but its arguments."""
import numpy as np

F = np.float32
KINDS = {'image': 0, 'pred': 1, 'seg': 2, 'overlay': 3, 'gt': 4, 'error': 5, 'slot_masked': 6, 'slot_mean': 7, 'slot_mask': 8}


def quantise(v):
    """(uint8)(int)(clamp(v) * 255 + 0.5), clamp(v) = v > 0 ? (v < 1 ? v : 1) : 0: a NaN fails `v > 0` and becomes 0"""
    v = np.asarray(v, dtype=F)
    with np.errstate(invalid='ignore'):
        c = np.where(v > 0, np.where(v < 1, v, F(1)), F(0)).astype(F)
    return (c * F(255) + F(0.5)).astype(np.int32).astype(np.uint8)


def argmax_labels(mask):
    """mask (K, S, S) -> (S, S) labels: strict `>` from -inf, slot 0 upwards - the lowest index wins a tie, a NaN never wins"""
    K = mask.shape[0]
    best = np.full(mask.shape[1:], -np.inf, dtype=F)
    lab = np.zeros(mask.shape[1:], dtype=np.int64)
    for k in range(K):
        with np.errstate(invalid='ignore'):
            win = mask[k] > best
        best = np.where(win, mask[k], best)
        lab = np.where(win, k, lab)
    return lab


def gt_labels(gt):
    """gt (G, S, S) uint8 -> (S, S): the lowest row with a non-zero byte, -1 where there is none"""
    lab = np.full(gt.shape[1:], -1, dtype=np.int64)
    for g in range(gt.shape[0] - 1, -1, -1):
        lab = np.where(gt[g] != 0, g, lab)
    return lab


def panel(kind, slot, r, palette, x=None, pred=None, mask=None, mean=None, gt=None, colors=None, gt_colors=None,
          background=(1., 1., 1.), alpha=0.5, edges=True, edge=(255, 255, 255), error_gain=4.0):
    """Panel of row r as uint8 (S, S, 3), at the source resolution.  Arrays: x / pred (R,3,S,S), mask (R,K,S,S), mean (R,K,3,S,S),
    gt (R,G,S,S), colors (R,K) / gt_colors (R,G) or None; palette (17, 3) uint8."""
    pal = np.asarray(palette, dtype=np.uint8)
    palf = pal.astype(F) / F(255)
    if kind in ('image', 'pred', 'slot_mean'):
        src = x[r] if kind == 'image' else pred[r] if kind == 'pred' else mean[r, slot]
        return quantise(src).transpose(1, 2, 0)
    if kind in ('seg', 'overlay'):
        lab = argmax_labels(mask[r])
        ci = lab if colors is None else np.minimum(colors[r].astype(np.int64)[lab], 16)
        if kind == 'seg':
            return pal[ci]
        a = F(alpha)
        oma = F(1) - a
        out = np.empty(lab.shape + (3,), dtype=np.uint8)
        for c in range(3):
            out[..., c] = quantise(oma * x[r, c].astype(F) + a * palf[ci, c])
        if edges:
            S = lab.shape[0]
            e = np.zeros(lab.shape, dtype=bool)
            e[:, :S - 1] |= lab[:, :S - 1] != lab[:, 1:]
            e[:S - 1, :] |= lab[:S - 1, :] != lab[1:, :]
            out[e] = np.asarray(edge, dtype=np.uint8)
        return out
    if kind == 'gt':
        lab = gt_labels(gt[r])
        ci = np.where(lab < 0, 16, lab) if gt_colors is None else np.where(lab < 0, 16, np.minimum(gt_colors[r].astype(np.int64)[np.maximum(lab, 0)], 16))
        return pal[ci]
    if kind == 'error':
        d = [np.abs(x[r, c].astype(F) - pred[r, c].astype(F)) for c in range(3)]
        s = (d[0] + d[1]) + d[2]
        with np.errstate(over='ignore', invalid='ignore'):
            g = quantise(F(error_gain) * s / F(3))
        return np.stack([g, g, g], axis=-1)
    if kind == 'slot_masked':
        m = mask[r, slot].astype(F)
        om = F(1) - m
        with np.errstate(over='ignore', invalid='ignore'):
            return np.stack([quantise(m * mean[r, slot, c].astype(F) + om * F(background[c])) for c in range(3)], axis=-1)
    if kind == 'slot_mask':
        g = quantise(mask[r, slot])
        return np.stack([g, g, g], axis=-1)
    raise ValueError(kind)


def sheet(panels, palette, mask, scale=1, pad=2, pad_value=(255, 255, 255), **kw):
    """panels: [(kind name, slot)]; mask (R,K,S,S) (the singleton channel dropped).  -> uint8 (H, W, 3)"""
    R, _, S, _ = mask.shape
    side = S * scale
    H, W = pad + R * (side + pad), pad + len(panels) * (side + pad)
    out = np.empty((H, W, 3), dtype=np.uint8)
    out[:] = np.asarray(pad_value, dtype=np.uint8)
    for r in range(R):
        for c, (kind, slot) in enumerate(panels):
            p = panel(kind, slot, r, palette, mask=mask, **kw)
            p = np.repeat(np.repeat(p, scale, axis=0), scale, axis=1)             # nearest-neighbour replication
            y0, x0 = pad + r * (side + pad), pad + c * (side + pad)
            out[y0:y0 + side, x0:x0 + side] = p
    return out
