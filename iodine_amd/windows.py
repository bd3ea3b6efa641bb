"""Windowed batches: frames kept at their native size in device memory, every item of a batch cut out of its frame on the device.

``resident.ResidentDataset`` freezes one crop at one size into the store.  A ``FrameStore`` keeps the frames as decoded - uint8
``(N, H, W, 3)`` or float32 ``(N, 3, H, W)``, masks uint16 ``(N, H, W)`` bit-words, a frame axis after ``N`` for clips - and
``window(index, size, policy)`` is ``iodine_batch_window`` (include/iodine_hip.h): per item a window ``y0, x0, h, w, flip, gain_r, gain_g,
gain_b`` of its frame, resampled to ``size x size`` with PIL's antialiased BILINEAR (masks: NEAREST), mirrored and scaled per channel, in
one launch.  The rule is stated in fp64 in tests/window_reference.py.  So one store serves every model size and every crop, and training
gets random windows, flips, scale changes and colour gains without host work per batch.

A window policy is a plain object with ``rows(indices, H, W, size, seed, epoch) -> float32 (n, 8)`` on the host: ``Center`` (the
reference's centre crop) and ``Augment`` (an item's window depends on ``(seed, epoch, index)`` alone - not on the batch size, the order or
the number of ranks).  ``check_rows`` validates the rows on the host before any launch: the kernel trusts them.  There is no CPU path."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib, synth
from .data import CLEVR, center_crop_box
from .objects import MAX_SLOTS
from .resident import ResidentBatches, ResidentDataset, check_fits, separate_masks_fast

MAX_SCALE = 4.0                                                              # source pixels per output pixel: at most 9 taps per axis
MAX_SIZE, MAX_FRAME = 512, 4096
EPOCH_STRIDE = 1000003


def _check_size(size, H, W):
    if isinstance(size, bool) or int(size) != size or not 1 <= size <= MAX_SIZE:
        raise ValueError(f'windows: size must be an integer in 1..{MAX_SIZE}; got {size!r}')
    if not (1 <= H <= MAX_FRAME and 1 <= W <= MAX_FRAME):
        raise ValueError(f'windows: frames must be 1..{MAX_FRAME} pixels high and wide; got {H} x {W}')
    return int(size)


def check_rows(rows, H, W, size):
    """The host-side contract of ``iodine_batch_window``'s windows: float32 ``(n, 8)``, finite, h, w > 0, the window inside the H x W frame,
    ``h / size`` and ``w / size`` at most 4, flip 0 or 1, gains >= 0.  A ``ValueError`` names the first row that breaks it."""
    r = np.asarray(rows)
    if r.dtype != np.float32 or r.ndim != 2 or r.shape[1] != 8 or r.shape[0] < 1:
        raise ValueError(f'windows: window rows must be float32 (n, 8); got {r.dtype} {r.shape}')
    d = r.astype(np.float64)
    y0, x0, h, w, flip, gains = d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4], d[:, 5:8]
    with np.errstate(invalid='ignore'):
        bad = ~np.isfinite(d).all(axis=1)
        bad |= ~((h > 0) & (w > 0) & (y0 >= 0) & (x0 >= 0) & (y0 + h <= H) & (x0 + w <= W))
        bad |= ~((h / size <= MAX_SCALE) & (w / size <= MAX_SCALE))
        bad |= ~((flip == 0) | (flip == 1))
        bad |= ~(gains >= 0).all(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f'windows: row {i} = {r[i].tolist()} is not a window of a {H} x {W} frame at size {size} (finite, h and w > 0, inside '
                         f'the frame, h / size and w / size <= {MAX_SCALE:g}, flip 0 or 1, gains >= 0)')
    return r


def _crop_of(crop, H, W, size, scale_hi=1.0, stretch=1.0):
    crop = min(H, W) if crop is None else crop
    if not (isinstance(crop, (int, float)) and not isinstance(crop, bool)) or not crop > 0:
        raise ValueError(f'windows: crop must be a number > 0; got {crop!r}')
    if crop > min(H, W):
        raise ValueError(f'windows: crop {crop} is larger than the {H} x {W} frame')
    if crop * scale_hi * stretch / size > MAX_SCALE:
        raise ValueError(f'windows: crop * scale / size = {crop * scale_hi * stretch / size:g} exceeds {MAX_SCALE:g} source pixels per output '
                         f'pixel (crop {crop}, largest scale {scale_hi:g}, aspect stretch {stretch:g}, size {size})')
    return crop


class Center:
    """The reference's centre box (``data.center_crop_box``) of ``crop`` pixels, default ``min(H, W)``; no flip, gains 1."""

    def __init__(self, crop=None):
        self.crop = crop

    def rows(self, indices, H, W, size, seed=0, epoch=0):
        size = _check_size(size, H, W)
        crop = _crop_of(self.crop, H, W, size)
        if int(crop) != crop:
            raise ValueError(f'windows: Center takes a whole crop; got {crop!r}')
        left, top, _, _ = center_crop_box(H, W, int(crop))
        row = np.array([top, left, crop, crop, 0, 1, 1, 1], dtype=np.float32)
        return np.tile(row, (len(np.asarray(indices).reshape(-1)), 1))


def _pair(v, name):
    lo, hi = (v, v) if isinstance(v, (int, float)) else tuple(v)
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo <= 0 or hi < lo:
        raise ValueError(f'windows: {name} must be a (lo, hi) range with 0 < lo <= hi; got {v!r}')
    return lo, hi


def item_uniforms(indices, seed, epoch, n=8):
    """``synth.uniform01(n, seed + 1000003 * epoch, stream=index)`` for every index at once: float64 ``(len(indices), n)``"""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.size and idx.min() < 0:
        raise ValueError('windows: indices must be >= 0')
    with np.errstate(over='ignore'):
        key = synth._splitmix(np.uint64(int(seed) + EPOCH_STRIDE * int(epoch)) * np.uint64(0x2545F4914F6CDD1D) + idx.astype(np.uint64))
        bits = synth._splitmix(np.arange(n, dtype=np.uint64)[None, :] ^ key[:, None])
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


class Augment:
    """Random windows.  Item ``index`` of epoch ``epoch`` draws ``u = synth.uniform01(8, seed + 1000003 * epoch, stream=index)`` and, in fp64:

        s = scale_lo + u0 (scale_hi - scale_lo);  a = exp(ln ratio_lo + u1 (ln ratio_hi - ln ratio_lo))
        h = min(H, crop s / sqrt(a)),  w = min(W, crop s sqrt(a))
        y0 = clamp((H - h) / 2 + (2 u2 - 1) translate, 0, H - h),  x0 likewise with u3;  translate='full': y0 = u2 (H - h), x0 = u3 (W - w)
        flip = flip enabled and u4 < 0.5;  gain_c = 1 + gain (2 u_{5+c} - 1)

    each rounded to float32 once (h and w first; y0 and x0 are placed with the rounded h and w and rounded down where rounding up would
    leave the frame).  ``crop`` defaults to ``min(H, W)``.  The defaults are the identity on a square frame of the model's size."""

    def __init__(self, crop=None, scale=(1, 1), ratio=(1, 1), translate=0, flip=False, gain=0.0):
        self.crop = crop
        self.scale, self.ratio = _pair(scale, 'scale'), _pair(ratio, 'ratio')
        if translate != 'full' and (isinstance(translate, (bool, str)) or not math.isfinite(float(translate)) or float(translate) < 0):
            raise ValueError(f"windows: translate must be a number of pixels >= 0 or 'full'; got {translate!r}")
        self.translate = translate if translate == 'full' else float(translate)
        self.flip = bool(flip)
        gain = float(gain)
        if not 0.0 <= gain < 1.0:
            raise ValueError(f'windows: gain must be in [0, 1); got {gain!r}')
        self.gain = gain

    def rows(self, indices, H, W, size, seed=0, epoch=0):
        size = _check_size(size, H, W)
        stretch = math.sqrt(max(self.ratio[1], 1.0 / self.ratio[0]))         # the longer side of the most stretched window
        crop = float(_crop_of(self.crop, H, W, size, self.scale[1], stretch))
        u = item_uniforms(indices, seed, epoch)
        s = self.scale[0] + u[:, 0] * (self.scale[1] - self.scale[0])
        a = np.exp(math.log(self.ratio[0]) + u[:, 1] * (math.log(self.ratio[1]) - math.log(self.ratio[0])))
        out = np.empty((u.shape[0], 8), dtype=np.float32)
        for col, n_src, length, k in ((0, H, crop * s / np.sqrt(a), 2), (1, W, crop * s * np.sqrt(a), 3)):
            length = np.minimum(float(n_src), length).astype(np.float32)     # (n_src is a float32: rounding cannot pass it)
            room = n_src - length.astype(np.float64)
            if self.translate == 'full':
                o0 = u[:, k] * room
            else:
                o0 = np.clip(room / 2 + (2 * u[:, k] - 1) * self.translate, 0.0, room)
            o32 = o0.astype(np.float32)
            o32 = np.where(o32.astype(np.float64) + length.astype(np.float64) > n_src, np.nextafter(o32, np.float32(-1)), o32)
            out[:, col], out[:, 2 + col] = np.maximum(o32, np.float32(0)), length
        out[:, 4] = (u[:, 4] < 0.5) if self.flip else 0
        out[:, 5:8] = 1.0 + self.gain * (2 * u[:, 5:8] - 1)
        return out


class FrameBatches(ResidentBatches):
    """What ``FrameStore.batches`` returns: ``ResidentBatches``' contract (``dataset``, ``sampler.set_epoch``, ``len``, ``order``) with the
    epoch's window rows computed once on the host and uploaded once, next to the index list; a batch is a slice of both."""

    def __init__(self, store, batch_size, size, policy, shuffle, seed, epoch, rank, world_size, drop_last):
        super().__init__(store, batch_size, shuffle, seed, epoch, rank, world_size, drop_last)
        self.size, self.policy = _check_size(size, store.height, store.width), policy
        policy.rows(np.zeros(1, dtype=np.int64), store.height, store.width, self.size, self.seed, self.epoch)   # refuse bad arguments now

    def __iter__(self):
        store = self.dataset
        mine = self.order()
        rows = check_rows(self.policy.rows(mine.numpy(), store.height, store.width, self.size, self.seed, self.epoch), store.height,
                          store.width, self.size)
        per = max(store.frames, 1)
        entries = store.entry_index(mine).to(store.device)
        dev_rows = torch.from_numpy(np.repeat(rows, per, axis=0)).to(store.device)
        stop = mine.numel() - (mine.numel() % self.batch_size if self.drop_last else 0)
        for lo in range(0, stop, self.batch_size):
            hi = lo + self.batch_size
            yield store._launch(mine[lo:hi], self.size, entries[lo * per:hi * per], dev_rows[lo * per:hi * per])


class FrameStore:
    """See the module text.  Build one with ``from_resident``, ``from_clevr`` or ``load``."""

    def __init__(self, images, masks, n_gt, device=None):
        images, n_gt = torch.as_tensor(images), torch.as_tensor(n_gt)
        masks = None if masks is None else torch.as_tensor(masks)
        if images.dtype == torch.uint8 and images.dim() in (4, 5) and images.shape[-1] == 3:
            self.image_kind, self.frames, (self.height, self.width) = 0, (images.shape[1] if images.dim() == 5 else 0), images.shape[-3:-1]
        elif images.dtype == torch.float32 and images.dim() in (4, 5) and images.shape[-3] == 3:
            self.image_kind, self.frames, (self.height, self.width) = 1, (images.shape[1] if images.dim() == 5 else 0), images.shape[-2:]
        else:
            raise ValueError('windows: images must be uint8 (N, [F,] H, W, 3) or float32 (N, [F,] 3, H, W), got '
                             f'{images.dtype} {tuple(images.shape)}')
        self.height, self.width = int(self.height), int(self.width)
        n, lead = int(images.shape[0]), tuple(images.shape[:images.dim() - 3])
        if n < 1 or not (1 <= self.height <= MAX_FRAME and 1 <= self.width <= MAX_FRAME):
            raise ValueError(f'windows: need at least one frame of 1..{MAX_FRAME} pixels a side, got {tuple(images.shape)}')
        if masks is not None and (masks.dtype != torch.uint16 or tuple(masks.shape) != lead + (self.height, self.width)):
            raise ValueError(f'windows: masks must be uint16 {lead + (self.height, self.width)}, got {masks.dtype} {tuple(masks.shape)}')
        if n_gt.dtype != torch.uint8 or tuple(n_gt.shape) != (n,):
            raise ValueError(f'windows: n_gt must be uint8 ({n},), got {n_gt.dtype} {tuple(n_gt.shape)}')
        self.n_gt_host = n_gt.detach().cpu().numpy().copy()
        if int(self.n_gt_host.max()) > MAX_SLOTS:
            raise ValueError(f'resident: at most {MAX_SLOTS} masks per image, got {int(self.n_gt_host.max())}')
        if masks is None and int(self.n_gt_host.max()) > 0:
            raise ValueError('windows: n_gt counts masks but there are none')
        self.planes = max(1, int(self.n_gt_host.max()))
        self.device = torch.device(device) if device is not None else images.device
        self.images = images.to(self.device).contiguous()
        self.masks = None if masks is None else masks.to(self.device).contiguous()
        self.n_gt = n_gt.to(self.device).contiguous()

    def __len__(self):
        return int(self.images.shape[0])

    # ---- construction ----
    @classmethod
    def from_resident(cls, store):
        """a ``ResidentDataset``'s tensors as a frame store (S x S frames), without copying"""
        if not isinstance(store, ResidentDataset):
            raise ValueError(f'windows: from_resident takes a ResidentDataset; got {type(store).__name__}')
        return cls(store.images, store.masks, store.n_gt, device=store.device)

    @classmethod
    def from_clevr(cls, ds, device, log=None):
        """Ingest the PNGs of a ``data.CLEVR`` uncropped and unresized: uint8 frames, the colour-coded masks as bit-words in
        ``data.clevr_separate_masks``' order (``resident.separate_masks_fast`` / ``pack_words``' layout).  Every frame must have one shape;
        more than 16 masks in an image are refused."""
        from PIL import Image
        if not isinstance(ds, CLEVR) or len(ds) < 1:
            raise ValueError('windows: from_clevr takes a non-empty data.CLEVR')
        images, masks, n_gt = [], [], []
        for i, path in enumerate(ds.img_paths):
            img = np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'))[:, :, :3]).astype(np.uint8)
            if images and img.shape != images[0].shape:
                raise ValueError(f'windows: every frame must have one shape, got {images[0].shape} and {img.shape} ({path})')
            images.append(img)
            mask_path = os.path.join(ds.root, 'masks', os.path.split(path)[-1])
            words, count = None, 0
            if os.path.exists(mask_path):
                mask_img = np.asarray(Image.open(mask_path).convert('RGB'))
                if mask_img.shape[:2] != img.shape[:2]:
                    raise ValueError(f'windows: a mask must have its image\'s size, got {mask_img.shape[:2]} for {img.shape[:2]} ({mask_path})')
                labels, count = separate_masks_fast(mask_img)
                if count > MAX_SLOTS:
                    raise ValueError(f'resident: at most {MAX_SLOTS} masks per image, got {count} ({mask_path})')
                words = np.where(labels > 0, np.left_shift(1, np.maximum(labels - 1, 0)), 0).astype(np.uint16)
            masks.append(words)
            n_gt.append(count)
            if log is not None and ((i + 1) % 1000 == 0 or i + 1 == len(ds)):
                log(f'windows: ingested {i + 1} / {len(ds)}')
        out_masks = None
        if any(m is not None for m in masks):
            out_masks = np.stack([m if m is not None else np.zeros(images[0].shape[:2], dtype=np.uint16) for m in masks])
        out_images = np.stack(images)
        check_fits(out_images.nbytes + (0 if out_masks is None else out_masks.nbytes), device)
        return cls(out_images, out_masks, np.asarray(n_gt, dtype=np.uint8), device=device)

    # the file format, the size and the clip entries are ResidentDataset's (same attributes): one .npz of plain arrays, no pickle
    save = ResidentDataset.save
    load = classmethod(ResidentDataset.load.__func__)
    nbytes = ResidentDataset.nbytes
    entry_index = ResidentDataset.entry_index

    # ---- batches ----
    def _launch(self, idx, size, entries, dev_rows):
        """the launch of one batch: host indices (validated here - the kernel trusts them), device entries and validated device rows"""
        n = len(self)
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= n:
            raise ValueError(f'windows: index out of range [0, {n}): {lo if lo < 0 else hi}')
        counts = self.n_gt_host[idx.numpy()]
        B, S, F = idx.numel(), size, self.frames
        if entries.numel() != B * max(F, 1) or tuple(dev_rows.shape) != (entries.numel(), 8):
            raise ValueError('windows: the device index list and window rows do not belong to this batch')
        lead = (B, F) if F else (B,)
        x = torch.empty(lead + (3, S, S), dtype=torch.float32, device=self.device)
        G = max(1, int(counts.max()))
        gt = torch.empty(lead + (G, S, S), dtype=torch.uint8, device=self.device) if self.masks is not None and counts.max() > 0 else None
        _lib.call('iodine_batch_window', self.device, entries, int(entries.numel()), self.images, self.image_kind,
                  self.masks if gt is not None else None, self.height, self.width, dev_rows, S, G, x, gt)
        return x, gt, counts

    def window(self, index, size, policy, seed=0, epoch=0):
        """One batch: ``index`` (a host sequence or tensor of B integers) -> ``(x, gt, n_gt_host)`` as ``ResidentDataset.gather`` returns them
        - ``x`` float32 ``(B, 3, size, size)`` (clips: ``(B, F, 3, size, size)``, all frames of a clip through their item's window), ``gt``
        uint8 ``(B, G, size, size)`` or None, ``n_gt_host`` uint8 ``(B,)`` numpy - every item through the window ``policy`` gives it for
        ``(seed, epoch, index)``.  ``policy`` may also be a float32 ``(B, 8)`` array of windows.  Indices and windows are validated on the
        host before the launch.  One launch, no synchronisation."""
        if self.device.type != 'cuda':
            raise RuntimeError('windows: window needs the store on a ROCm device (no CPU fallback)')
        idx = torch.as_tensor(index.detach().cpu() if isinstance(index, torch.Tensor) else np.asarray(index))
        if idx.dim() != 1 or idx.numel() < 1 or idx.dtype in (torch.bool, torch.float16, torch.float32, torch.float64, torch.bfloat16):
            raise ValueError(f'windows: index must be a non-empty 1-D sequence of integers, got {idx.dtype} {tuple(idx.shape)}')
        idx = idx.to(torch.int64)
        size = _check_size(size, self.height, self.width)
        rows = policy.rows(idx.numpy(), self.height, self.width, size, seed, epoch) if hasattr(policy, 'rows') else np.asarray(policy)
        rows = check_rows(rows, self.height, self.width, size)
        if rows.shape[0] != idx.numel():
            raise ValueError(f'windows: {idx.numel()} indices but {rows.shape[0]} window rows')
        per = max(self.frames, 1)
        dev_rows = torch.from_numpy(np.ascontiguousarray(np.repeat(rows, per, axis=0))).to(self.device)
        return self._launch(idx, size, self.entry_index(idx).to(self.device), dev_rows)

    def batches(self, batch_size, size, policy, shuffle=True, seed=0, epoch=0, rank=0, world_size=1, drop_last=False):
        """The batches of an epoch, ``(x, gt, n_gt_host)`` each (``window``), as an object that can be iterated epoch after epoch
        (``set_epoch``, which ``engine.train`` calls): the order is ``resident.epoch_order`` / ``shard_order``, the epoch's window rows are
        computed once on the host and uploaded once next to the index list."""
        return FrameBatches(self, batch_size, size, policy, shuffle, seed, epoch, rank, world_size, drop_last)
