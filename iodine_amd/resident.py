"""Device-resident datasets: the whole data set in device memory, a batch assembled there by one launch.

The data sets of the reference are small as bytes (CLEVR6 at 128 x 128 uint8: 2.4 GB) and slow to produce on the host (PIL, ``np.unique``,
``pack_gt`` per item).  ``ResidentDataset`` keeps them on one ROCm device:

* ``images``: uint8 ``(N, S, S, 3)``, HWC as decoded, or float32 ``(N, 3, S, S)`` for sources that are not 8-bit (the synthetic scenes);
  clips carry a frame axis after ``N``.
* ``masks``: uint16 ``(N, S, S)`` (frame axis for clips) or None.  Bit ``g`` of a word is set where the pixel lies inside ground-truth
  mask ``g``: one word per pixel whatever the number of masks, and overlapping masks stay exact.  At most ``MAX_SLOTS`` = 16 per image.
* ``n_gt``: uint8 ``(N,)`` on the device, ``n_gt_host`` its host copy; 0 = an unlabelled image.  ``planes`` = max(1, largest n_gt).

``gather(index)`` is ``iodine_batch_gather`` (include/iodine_hip.h): ``x`` float32 ``(B, 3, S, S)`` with the bits of ``ToTensor`` and ``gt``
uint8 ``(B, G, S, S)`` in ``pack_gt``'s layout, G = max(1, largest n_gt of the batch).  ``batches(...)`` iterates an epoch: the permutation is
the stable argsort of ``iodine_randn(seed, stream_id=epoch)``, computed on the device, the same on every rank, and copied to the host once
per epoch - the only synchronisation; the host then knows every batch's indices and hence its ``n_gt``.  ``synthetic(...)`` fills a store
with the bits of ``synth.make_images`` without the host (``iodine_synth_scenes``).  There is no CPU path for the gather or the generator; a
store may be held on the CPU (ingest, save, load), but batches come from a ROCm device only."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .data import CLEVR, CLEVR_BACKGROUND, center_crop_box
from .objects import MAX_SLOTS

KINDS = {'uniform': 0, 'blobs': 1}
MAX_WORKERS = 16


# ---- bit-words ----------------------------------------------------------------------------------------------------------------------
def pack_words(planes) -> np.ndarray:
    """``(G, ...)`` masks (non-zero = inside) -> uint16 words ``(...)``, bit g from plane g.  More than ``MAX_SLOTS`` planes are refused."""
    m = np.asarray(planes)
    if m.shape[0] > MAX_SLOTS:
        raise ValueError(f'resident: at most {MAX_SLOTS} masks per image, got {m.shape[0]}')
    words = np.zeros(m.shape[1:], dtype=np.uint16)
    for g in range(m.shape[0]):
        words |= (m[g] != 0).astype(np.uint16) << np.uint16(g)
    return words


def unpack_words(words, planes: int) -> np.ndarray:
    """uint16 words ``(..., S, S)`` -> uint8 0/1 planes ``(..., planes, S, S)``: what the gather kernel writes."""
    w = np.asarray(words, dtype=np.uint16)
    out = [((w >> np.uint16(g)) & np.uint16(1)).astype(np.uint8) for g in range(planes)]
    return np.stack(out, axis=-3)


def separate_masks_fast(mask_img: np.ndarray):
    """``data.clevr_separate_masks`` without the row-wise ``np.unique``: colours packed to one int32, ``(labels (H, W) int32, count)`` with
    label j + 1 on the pixels of that function's plane j (its order: colours sorted lexicographically = by packed value) and 0 on the
    background colour."""
    m = np.ascontiguousarray(mask_img[:, :, :3]).astype(np.int32)
    packed = (m[:, :, 0] << 16) | (m[:, :, 1] << 8) | m[:, :, 2]
    colours, inverse = np.unique(packed.reshape(-1), return_inverse=True)
    bg = (CLEVR_BACKGROUND[0] << 16) | (CLEVR_BACKGROUND[1] << 8) | CLEVR_BACKGROUND[2]
    label_of = np.zeros(len(colours), dtype=np.int32)
    keep = colours != bg
    label_of[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return label_of[inverse.reshape(-1)].reshape(packed.shape), int(keep.sum())


def planes_from_labels(labels: np.ndarray, count: int) -> np.ndarray:
    """the boolean planes ``(count, H, W)`` of a label map (``separate_masks_fast``)"""
    return np.stack([labels == j + 1 for j in range(count)], axis=0) if count else np.zeros((0,) + labels.shape, dtype=bool)


class _FastCLEVR(torch.utils.data.Dataset):
    """``data.CLEVR`` items as the store keeps them - (uint8 HWC image, uint16 words or None, n_gt) - without the float image and the
    per-plane loops: the label map goes through the crop and the NEAREST resize once (a nearest resize picks one source pixel per
    destination pixel whatever its value, so the planes of the resized map are the resized planes)."""

    def __init__(self, ds, crop=192, size=128):
        self.ds, self.crop, self.size = ds, crop, size

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, index):
        from PIL import Image
        path = self.ds.img_paths[index]
        img = np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'))[:, :, :3]).astype(np.uint8)
        box = center_crop_box(img.shape[0], img.shape[1], self.crop)
        u8 = np.asarray(Image.fromarray(img).crop(box).resize((self.size, self.size), Image.BILINEAR), dtype=np.uint8).copy()
        mask_path = os.path.join(self.ds.root, 'masks', os.path.split(path)[-1])
        if not os.path.exists(mask_path):
            return u8, None, 0
        mask_img = np.asarray(Image.open(mask_path).convert('RGB'))
        labels, count = separate_masks_fast(mask_img)
        if count > MAX_SLOTS:
            raise ValueError(f'resident: at most {MAX_SLOTS} masks per image, got {count} ({mask_path})')
        box = center_crop_box(mask_img.shape[0], mask_img.shape[1], self.crop)
        lab = np.asarray(Image.fromarray(labels.astype(np.int32)).crop(box).resize((self.size, self.size), Image.NEAREST)).astype(np.int64)
        words = np.where(lab > 0, np.left_shift(1, np.maximum(lab - 1, 0)), 0).astype(np.uint16)
        return u8, words, count


def _as_u8(x: torch.Tensor):
    """uint8 q with q / 255 == x bit for bit, or None"""
    q = torch.round(x * 255.0)
    if not bool(((q >= 0) & (q <= 255)).all()):
        return None
    q8 = q.to(torch.uint8)
    back = q8.float().div_(255.0)
    return q8 if torch.equal(back.view(torch.int32), x.contiguous().view(torch.int32)) else None


def _item_arrays(item):
    """one item of CLEVR / MultiDSprites / SyntheticScenes / SyntheticClips -> (float32 image (.., 3, S, S), words (.., S, S) or None, n_gt)"""
    img, mask = item[0], item[1]
    x = torch.as_tensor(np.asarray(img)) if not isinstance(img, torch.Tensor) else img
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or x.shape[-3] != 3 or x.shape[-1] != x.shape[-2]:
        raise ValueError(f'resident: an image must be float32 (3, S, S) or a clip (F, 3, S, S), got {x.dtype} {tuple(x.shape)}')
    if mask is None:
        return x, None, 0
    m = np.asarray(mask.detach().cpu() if isinstance(mask, torch.Tensor) else mask)
    want = x.dim()                                                           # (G, S, S) for a still, (F, G, S, S) for a clip
    if m.ndim != want or m.shape[-2:] != tuple(x.shape[-2:]) or (want == 4 and m.shape[0] != x.shape[0]):
        raise ValueError(f'resident: masks must be (G, S, S) for an image and (F, G, S, S) for a clip, got {m.shape} for {tuple(x.shape)}')
    g = m.shape[-3]
    if g == 0:
        return x, None, 0
    return x, pack_words(np.moveaxis(m, -3, 0)), g


def _collate(batch):
    return batch


def ingest(ds, workers: int = 0, log=None, crop: int = 192, size: int = 128):
    """A map-style data set -> host arrays ``{'images', 'masks' (or None), 'n_gt'}`` in the store's formats, through a ``DataLoader`` with at
    most 16 workers.  Images stay uint8 while ``round(x * 255) / 255`` reproduces every element of every image bitwise; the first image that
    does not turns the whole store float32 (the images before it are converted back, which is exact).  A ``data.CLEVR`` is read through
    ``_FastCLEVR`` (``crop`` / ``size``: the arguments of ``data.clevr_image`` / ``clevr_masks``, whose defaults ``data.CLEVR`` uses)."""
    fast = isinstance(ds, CLEVR)
    src = _FastCLEVR(ds, crop, size) if fast else ds
    n = len(src)
    if n < 1:
        raise ValueError('resident: the data set is empty')
    workers = max(0, min(int(workers), MAX_WORKERS))
    loader = torch.utils.data.DataLoader(src, batch_size=16, shuffle=False, num_workers=workers, collate_fn=_collate)
    images, masks, n_gt, as_u8 = [], [], [], True
    for chunk in loader:
        for item in chunk:
            if fast:
                u8, words, count = item
                images.append(np.asarray(u8))
            else:
                x, words, count = _item_arrays(item)
                q = _as_u8(x) if as_u8 else None
                if as_u8 and q is None:                                      # not 8-bit: everything so far goes back to float32, exactly
                    images = [torch.from_numpy(a).movedim(-1, -3).float().div_(255.0).numpy() for a in images]
                    as_u8 = False
                images.append(q.movedim(-3, -1).contiguous().numpy() if as_u8 else x.contiguous().numpy())
            masks.append(None if words is None else np.asarray(words))
            n_gt.append(count)
        if log is not None:
            log(f'resident: ingested {len(images)} / {n}')
    shapes = {a.shape for a in images}
    if len(shapes) != 1:
        raise ValueError(f'resident: every item must have one shape, got {sorted(shapes)}')
    out_images = np.stack(images)
    out_masks = None
    if any(m is not None for m in masks):
        mshape = out_images.shape[1:-1] if as_u8 or fast else out_images.shape[1:-3] + out_images.shape[-2:]
        out_masks = np.stack([m if m is not None else np.zeros(mshape, dtype=np.uint16) for m in masks])
    return {'images': out_images, 'masks': out_masks, 'n_gt': np.asarray(n_gt, dtype=np.uint8)}


# ---- epoch order --------------------------------------------------------------------------------------------------------------------
def epoch_order(n: int, seed: int, epoch: int, device) -> torch.Tensor:
    """The permutation of epoch ``epoch``: the stable argsort of the n normals ``iodine_randn(seed, stream_id=epoch)``, computed on ``device``
    and returned on the host (int64) - one copy, the epoch's only synchronisation.  A function of (n, seed, epoch) alone, so every rank gets
    the same list."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('resident: the epoch order is drawn on a ROCm device (no CPU fallback)')
    keys = torch.empty((n,), dtype=torch.float32, device=device)
    _lib.call('iodine_randn', device, keys, n, int(seed), int(epoch))
    return torch.argsort(keys, stable=True).cpu()


def shard_order(order, rank: int = 0, world_size: int = 1):
    """The entries of ``order`` rank ``rank`` of ``world_size`` takes: the list is padded by wrapping round to a multiple of ``world_size``
    and every ``world_size``-th entry from ``rank`` on is kept, like ``DistributedSampler``."""
    if not 0 <= rank < world_size:
        raise ValueError(f'resident: rank must be in [0, {world_size}), got {rank}')
    order = torch.as_tensor(np.asarray(order)).to(torch.int64).reshape(-1)
    n = order.numel()
    total = -(-n // world_size) * world_size
    if total > n:
        order = torch.cat([order] + [order] * ((total - n + n - 1) // n))[:total]
    return order[rank::world_size]


class ResidentBatches:
    """What ``ResidentDataset.batches`` returns: iterable once per epoch, any number of epochs, yielding ``(x, gt, n_gt_host)``.  It carries
    the attributes of a ``DataLoader`` that ``engine.train`` / ``engine.evaluate`` look at - ``dataset`` (the store) and ``sampler`` with
    ``set_epoch`` (itself)."""

    def __init__(self, store, batch_size, shuffle, seed, epoch, rank, world_size, drop_last):
        if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
            raise ValueError(f'resident: batch_size must be an integer >= 1; got {batch_size!r}')
        if world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f'resident: need 0 <= rank < world_size; got rank {rank}, world_size {world_size}')
        self.dataset, self.batch_size, self.shuffle, self.seed, self.epoch = store, int(batch_size), bool(shuffle), int(seed), int(epoch)
        self.rank, self.world_size, self.drop_last = int(rank), int(world_size), bool(drop_last)
        self.sampler = self

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def order(self):
        """this rank's indices for the current epoch (host, int64)"""
        n = len(self.dataset)
        full = epoch_order(n, self.seed, self.epoch, self.dataset.device) if self.shuffle else torch.arange(n, dtype=torch.int64)
        return shard_order(full, self.rank, self.world_size)

    def __len__(self):
        n = -(-len(self.dataset) // self.world_size)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        mine = self.order()
        entries = self.dataset.entry_index(mine).to(self.dataset.device)     # the epoch's list goes to the device once, a batch is a slice
        per = max(self.dataset.frames, 1)
        stop = mine.numel() - (mine.numel() % self.batch_size if self.drop_last else 0)
        for lo in range(0, stop, self.batch_size):
            yield self.dataset.gather(mine[lo:lo + self.batch_size], _entries=entries[lo * per:(lo + self.batch_size) * per])


class ResidentDataset:
    """See the module text.  Build one with ``from_dataset``, ``synthetic`` or ``load``."""

    def __init__(self, images, masks, n_gt, device=None):
        images, n_gt = torch.as_tensor(images), torch.as_tensor(n_gt)
        masks = None if masks is None else torch.as_tensor(masks)
        if images.dtype == torch.uint8 and images.dim() in (4, 5) and images.shape[-1] == 3 and images.shape[-2] == images.shape[-3]:
            self.image_kind, self.frames, self.size = 0, (images.shape[1] if images.dim() == 5 else 0), int(images.shape[-2])
        elif images.dtype == torch.float32 and images.dim() in (4, 5) and images.shape[-3] == 3 and images.shape[-1] == images.shape[-2]:
            self.image_kind, self.frames, self.size = 1, (images.shape[1] if images.dim() == 5 else 0), int(images.shape[-1])
        else:
            raise ValueError('resident: images must be uint8 (N, [F,] S, S, 3) or float32 (N, [F,] 3, S, S), got '
                             f'{images.dtype} {tuple(images.shape)}')
        n, lead = int(images.shape[0]), tuple(images.shape[:images.dim() - 3])
        if n < 1 or not 1 <= self.size <= 4096:
            raise ValueError(f'resident: need at least one image and a size in 1..4096, got {tuple(images.shape)}')
        if masks is not None and (masks.dtype != torch.uint16 or tuple(masks.shape) != lead + (self.size, self.size)):
            raise ValueError(f'resident: masks must be uint16 {lead + (self.size, self.size)}, got {masks.dtype} {tuple(masks.shape)}')
        if n_gt.dtype != torch.uint8 or tuple(n_gt.shape) != (n,):
            raise ValueError(f'resident: n_gt must be uint8 ({n},), got {n_gt.dtype} {tuple(n_gt.shape)}')
        self.n_gt_host = n_gt.detach().cpu().numpy().copy()
        if int(self.n_gt_host.max()) > MAX_SLOTS:
            raise ValueError(f'resident: at most {MAX_SLOTS} masks per image, got {int(self.n_gt_host.max())}')
        if masks is None and int(self.n_gt_host.max()) > 0:
            raise ValueError('resident: n_gt counts masks but there are none')
        self.planes = max(1, int(self.n_gt_host.max()))
        self.device = torch.device(device) if device is not None else images.device
        self.images = images.to(self.device).contiguous()
        self.masks = None if masks is None else masks.to(self.device).contiguous()
        self.n_gt = n_gt.to(self.device).contiguous()

    def __len__(self):
        return int(self.images.shape[0])

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.images, self.masks, self.n_gt) if t is not None)

    # ---- construction ----
    @classmethod
    def from_dataset(cls, ds, device, workers=0, log=None):
        """Ingest any map-style data set with the item format of ``data.CLEVR``, ``data.MultiDSprites`` or ``engine.SyntheticScenes`` /
        ``SyntheticClips`` (``ingest``) and put it on ``device``.  ``workers`` > 0 starts that many loader processes (at most 16) the way any
        ``DataLoader`` does - by fork where that is the platform's default, so ingest before other work has opened the device, or keep 0."""
        a = ingest(ds, workers=workers, log=log)
        check_fits(sum(v.nbytes for v in a.values() if v is not None), device)
        return cls(a['images'], a['masks'], a['n_gt'], device=device)

    @classmethod
    def synthetic(cls, n, size, seed=0, kind='blobs', max_objects=6, frames=0, device='cuda', first_index=0):
        """A float32 store filled on the device with the bits of ``synth.make_images``: item i is ``engine.SyntheticScenes(.., size,
        seed)[first_index + i]`` - ``make_images(1, size, seed=seed + first_index + i, kind, max_objects)`` - and, for ``frames`` > 0, the
        clip ``engine.SyntheticClips`` rolls from it; masks and counts likewise (``kind='uniform'`` has none)."""
        images, masks, n_gt = synth_scenes(n, size, seed=int(seed) + int(first_index), kind=kind, max_objects=max_objects, frames=frames,
                                           device=device)
        return cls(images, masks, n_gt)

    def save(self, path):
        """one .npz of plain arrays (no pickle); ``load`` gives the same bits back"""
        arrays = {'images': self.images.cpu().numpy(), 'n_gt': self.n_gt_host}
        if self.masks is not None:
            arrays['masks'] = self.masks.cpu().numpy()
        with open(path, 'wb') as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, device):
        with np.load(path, allow_pickle=False) as z:
            images, n_gt = z['images'], z['n_gt']
            masks = z['masks'] if 'masks' in z.files else None
        check_fits(images.nbytes + n_gt.nbytes + (0 if masks is None else masks.nbytes), device)
        return cls(images, masks, n_gt, device=device)

    # ---- batches ----
    def entry_index(self, index):
        """host int64 indices -> the store entries the gather kernel reads: the indices themselves, or n F + f for the F frames of clip n"""
        idx = torch.as_tensor(index).to(torch.int64).reshape(-1)
        if not self.frames:
            return idx
        return (idx[:, None] * self.frames + torch.arange(self.frames, dtype=torch.int64)[None, :]).reshape(-1)

    def gather(self, index, _entries=None):
        """One batch: ``index`` (a host sequence or tensor of B integers) -> ``(x, gt, n_gt_host)`` with ``x`` float32 ``(B, 3, S, S)`` (clips:
        ``(B, F, 3, S, S)``) and ``gt`` uint8 ``(B, G, S, S)`` (``(B, F, G, S, S)``) on the device, G = max(1, largest n_gt of the batch), rows
        beyond an image's n_gt zero - ``pack_gt``'s output - or None where no image of the batch has a mask; ``n_gt_host`` uint8 ``(B,)``
        numpy.  An index outside [0, N) is a ``ValueError`` before any launch.  One launch, no synchronisation."""
        if self.device.type != 'cuda':
            raise RuntimeError('resident: gather needs the store on a ROCm device (no CPU fallback)')
        idx = torch.as_tensor(index.detach().cpu() if isinstance(index, torch.Tensor) else np.asarray(index))
        if idx.dim() != 1 or idx.numel() < 1 or idx.dtype in (torch.bool, torch.float16, torch.float32, torch.float64, torch.bfloat16):
            raise ValueError(f'resident: index must be a non-empty 1-D sequence of integers, got {idx.dtype} {tuple(idx.shape)}')
        idx = idx.to(torch.int64)
        n = len(self)
        lo, hi = int(idx.min()), int(idx.max())                              # (always, the epoch's own lists included: the kernel trusts them)
        if lo < 0 or hi >= n:
            raise ValueError(f'resident: index out of range [0, {n}): {lo if lo < 0 else hi}')
        counts = self.n_gt_host[idx.numpy()]
        B, S, F = idx.numel(), self.size, self.frames
        dev_idx = _entries if _entries is not None else self.entry_index(idx).to(self.device)
        if dev_idx.dtype != torch.int64 or dev_idx.device != self.device or dev_idx.numel() != B * max(F, 1):
            raise ValueError('resident: the device index list does not belong to this batch')
        lead = (B, F) if F else (B,)
        x = torch.empty(lead + (3, S, S), dtype=torch.float32, device=self.device)
        G = max(1, int(counts.max()))
        gt = torch.empty(lead + (G, S, S), dtype=torch.uint8, device=self.device) if self.masks is not None and counts.max() > 0 else None
        _lib.call('iodine_batch_gather', self.device, dev_idx, int(dev_idx.numel()), self.images, self.image_kind,
                  self.masks if gt is not None else None, S, G, x, gt)
        return x, gt, counts

    def batches(self, batch_size, shuffle=True, seed=0, epoch=0, rank=0, world_size=1, drop_last=False):
        """The batches of an epoch, ``(x, gt, n_gt_host)`` each (``gather``), as an object that can be iterated epoch after epoch
        (``set_epoch``, which ``engine.train`` calls).  ``shuffle``: the order is ``epoch_order(N, seed, epoch)`` - one device sort and one
        copy to the host per epoch; without it 0..N-1 and no synchronisation at all.  Rank ``rank`` of ``world_size`` takes ``shard_order``
        of it.  ``drop_last`` drops a final short batch."""
        return ResidentBatches(self, batch_size, shuffle, seed, epoch, rank, world_size, drop_last)


def synth_scenes(n, size, seed=0, kind='blobs', max_objects=6, frames=0, device='cuda', seed_step=1, stream=0, stream_step=0):
    """``iodine_synth_scenes``: ``(images float32 (n, [F,] 3, S, S), masks uint16 (n, [F,] S, S) or None, n_gt uint8 (n,))`` on ``device``.
    Item i draws from ``uniform01(seed + i seed_step, stream + i stream_step)``: the defaults are ``SyntheticScenes``' items (seed + i, stream
    0); ``seed_step=0, stream=first, stream_step=1`` is ``synth.make_images(n, size, seed, first_index=first)``."""
    if kind not in KINDS:
        raise ValueError(f"resident: kind must be 'uniform' or 'blobs'; got {kind!r}")
    if int(n) < 1 or not 1 <= int(size) <= 1024 or not 1 <= int(max_objects) <= MAX_SLOTS or int(frames) < 0:
        raise ValueError(f'resident: need n >= 1, size in 1..1024, max_objects in 1..{MAX_SLOTS} and frames >= 0; got n = {n}, size = {size}, '
                         f'max_objects = {max_objects}, frames = {frames}')
    if min(int(seed), int(seed_step), int(stream), int(stream_step)) < 0:
        raise ValueError('resident: seeds and streams must be >= 0')
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('resident: synthetic scenes are generated on a ROCm device (no CPU fallback)')
    n, S, F = int(n), int(size), int(frames)
    lead = (n, F) if F else (n,)
    check_fits(n * max(F, 1) * S * S * 14, device)
    images = torch.empty(lead + (3, S, S), dtype=torch.float32, device=device)
    blobs = kind == 'blobs'
    masks = torch.empty(lead + (S, S), dtype=torch.uint16, device=device) if blobs else None
    n_gt = torch.zeros((n,), dtype=torch.uint8, device=device)
    _lib.call('iodine_synth_scenes', device, n, S, int(seed), int(seed_step), int(stream), int(stream_step), KINDS[kind], int(max_objects), F,
              images, masks, n_gt)
    return images, masks, n_gt


def check_fits(nbytes, device):
    """refuse in words a store larger than the free device memory"""
    device = torch.device(device)
    if device.type != 'cuda':
        return
    free, _ = torch.cuda.mem_get_info(device)
    if nbytes > free:
        raise RuntimeError(f'resident: the store needs {nbytes / 2 ** 30:.2f} GiB but {device} has {free / 2 ** 30:.2f} GiB free; '
                           'use the DataLoader path or a smaller data set')
