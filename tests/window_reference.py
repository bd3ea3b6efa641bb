"""The resampling rule of windowed batches (iodine_batch_window, iodine_amd.windows) in numpy fp64 - the definition the kernel and every
test refer to.  No torch.

A window is a row of 8 float32 values ``y0, x0, h, w, flip, gain_r, gain_g, gain_b``: ``y0, x0, h, w`` in source pixels (fractional
values allowed, h, w > 0, the window inside the H x W frame), flip 0 or 1, gains >= 0.  Output pixel (i, j) of an S x S image is crop-then-
resize with a triangle filter, separably - PIL's BILINEAR with antialiasing on the cut-out window.  Per axis (``axis_taps``; rows shown):

    scale = h / S, support = max(scale, 1), centre = y0 + (i + 0.5) scale
    taps: the whole rows r of [lo, hi), lo = max(floor(y0), 0, int(centre - support + 0.5)),
                                       hi = min(ceil(y0 + h), H, int(centre + support + 0.5)), int truncating
    weight of r: max(0, 1 - |r + 0.5 - centre| / support), normalised by the sum over the taps

(the taps are clamped to the window rounded outward to whole pixels: a window is resampled as if it had been cut out first; scale <= 4, so
at most 9 taps).  Image: ``out = clamp(gain_c sum_r sum_q wy_r wx_q v[r][q][c], 0, 1)``, v = u / 255 (the float32 division of ToTensor)
for a uint8 frame or the stored float, columns first, then rows.  Masks: the uint16 word of source pixel ``(floor(centre_y(i)),
floor(centre_x(j)))``, clamped to the frame - PIL's NEAREST - unpacked to 0/1 planes.  flip = 1: output column j holds what column S - 1 - j
would have held, image and masks."""
import numpy as np

MAX_TAPS = 9


def axis_taps(o0, length, n_src, S):
    """one axis: ``(first (S,) int, count (S,) int, weights (S, 9) float64 - zero beyond count -, nearest (S,) int)``"""
    o0, length = float(o0), float(length)
    scale = length / S
    support = max(scale, 1.0)
    first, count, nearest = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    weights = np.zeros((S, MAX_TAPS), dtype=np.float64)
    for i in range(S):
        centre = o0 + (i + 0.5) * scale
        lo = max(int(np.floor(o0)), 0, int(centre - support + 0.5))
        hi = min(int(np.ceil(o0 + length)), n_src, int(centre + support + 0.5))
        assert 1 <= hi - lo <= MAX_TAPS, (o0, length, n_src, S, i, lo, hi)
        w = np.maximum(0.0, 1.0 - np.abs(np.arange(lo, hi) + 0.5 - centre) / support)
        total = 0.0
        for v in w:                                                          # ascending, like the device's sum
            total += v
        first[i], count[i] = lo, hi - lo
        weights[i, :hi - lo] = w / total
        nearest[i] = min(max(int(np.floor(centre)), 0), n_src - 1)
    return first, count, weights, nearest


def _values(frame):
    """a frame as float64 (3, H, W): uint8 (H, W, 3) through the float32 division, float32 (3, H, W) as stored"""
    f = np.asarray(frame)
    if f.dtype == np.uint8:
        assert f.ndim == 3 and f.shape[2] == 3
        return (f.astype(np.float32) / np.float32(255.0)).astype(np.float64).transpose(2, 0, 1)
    assert f.dtype == np.float32 and f.ndim == 3 and f.shape[0] == 3
    return f.astype(np.float64)


def _resample(v, taps, axis):
    """apply one axis' taps to ``v`` along ``axis``"""
    first, count, weights, _ = taps
    v = np.moveaxis(v, axis, -1)
    out = np.zeros(v.shape[:-1] + (len(first),), dtype=np.float64)
    for i in range(len(first)):
        for k in range(count[i]):
            out[..., i] += weights[i, k] * v[..., first[i] + k]
    return np.moveaxis(out, -1, axis)


def window_image(frame, row, S):
    """one frame (uint8 (H, W, 3) or float32 (3, H, W)) through the window ``row`` -> float64 (3, S, S)"""
    v = _values(frame)
    H, W = v.shape[1:]
    r = np.asarray(row, dtype=np.float32).astype(np.float64)
    out = _resample(_resample(v, axis_taps(r[1], r[3], W, S), 2), axis_taps(r[0], r[2], H, S), 1)     # columns first, then rows
    out = np.clip(r[5:8, None, None] * out, 0.0, 1.0)
    return out[:, :, ::-1].copy() if r[4] != 0 else out


def window_words(words, row, S):
    """the uint16 words (H, W) of a frame through the window -> uint16 (S, S)"""
    words = np.asarray(words)
    H, W = words.shape
    r = np.asarray(row, dtype=np.float32).astype(np.float64)
    ny, nx = axis_taps(r[0], r[2], H, S)[3], axis_taps(r[1], r[3], W, S)[3]
    out = words[ny[:, None], nx[None, :]]
    return out[:, ::-1].copy() if r[4] != 0 else out


def unpack(words, planes):
    """uint16 words (..., S, S) -> uint8 0/1 planes (..., planes, S, S), as iodine_batch_gather unpacks them"""
    w = np.asarray(words, dtype=np.uint16)
    return np.stack([((w >> np.uint16(g)) & np.uint16(1)).astype(np.uint8) for g in range(planes)], axis=-3)


def window_batch(images, masks, index, rows, S, planes):
    """a batch: frames ``images[index[j]]`` (and ``masks[index[j]]``, or None) through ``rows[j]`` -> ``(x float64 (B, 3, S, S), gt uint8
    (B, planes, S, S) or None)``"""
    x = np.stack([window_image(images[i], rows[j], S) for j, i in enumerate(index)])
    gt = None if masks is None else np.stack([unpack(window_words(masks[i], rows[j], S), planes) for j, i in enumerate(index)])
    return x, gt
