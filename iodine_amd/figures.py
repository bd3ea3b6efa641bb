"""Decomposition figures: image, reconstruction, segmentation and one panel per slot, rendered on the device.

``sheet`` turns the tensors ``reconstruct`` / ``decode`` / a ``trajectory`` return - ``mask (*, K, 1, S, S)``, ``mean (*, K, 3, S, S)``,
``pred (*, 3, S, S)`` and the input ``x`` - into one ``uint8 (H, W, 3)`` picture in one launch of ``iodine_render_sheet``: a row per scene
(or per refinement iteration, or per frame), a panel per entry of ``panels``.  Only the finished picture crosses to the host
(``encode_png`` / ``write_png``: 8-bit RGB PNG through ``zlib`` and ``struct``).  ``decomposition`` runs a model and draws its figure,
``trajectory_sheet`` draws the refinement figure of one image from ``model.trajectory``, ``restarts_sheet`` the chains of one image from
``model.restarts`` with matched colours, ``matched_colors`` gives slots and ground-truth
masks the same palette entries so that the ``seg`` and ``gt`` panels compare by eye, ``layout`` is the host arithmetic of the panel boxes.

Panels: ``'image'``, ``'pred'``, ``'seg'`` (palette colour of the argmax slot), ``'overlay'`` (the image blended with ``seg``, segment edges
drawn), ``'gt'``, ``'error'`` (grey ``error_gain * mean_c |x - pred|``), ``('slot_masked', k)`` = ``m_k mean_k + (1 - m_k) background``,
``('slot_mean', k)``, ``('slot_mask', k)``, and ``'slots'`` = the K panels of ``slot_mode``.  The arithmetic is fixed to the byte
(include/iodine_hip.h, iodine_render_sheet; tests/sheet_reference.py restates it in numpy).  Like the other stateless kernels there is no
CPU path."""
from __future__ import annotations

import ctypes as C
import struct
import zlib

import numpy as np
import torch

from . import _lib
from .objects import MAX_SIZE, MAX_SLOTS

# 16 slot colours, mutually distinct, and entry 16 = "none" (no slot / no ground-truth row): a dark grey
PALETTE = (
    (230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
    (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
    (48, 48, 48),
)
NONE_COLOR = 16
KINDS = {'image': 0, 'pred': 1, 'seg': 2, 'overlay': 3, 'gt': 4, 'error': 5, 'slot_masked': 6, 'slot_mean': 7, 'slot_mask': 8}
SLOT_MODES = {'masked': 'slot_masked', 'mean': 'slot_mean', 'mask': 'slot_mask'}
MAX_PANELS = 64
FORM_VECTOR_LOADS, FORM_WORD_STORES = 1, 2                   # bits of ``sheet_form``


def expand_panels(panels, K: int, slot_mode: str = 'masked'):
    """The panel list as ``[(kind name, slot)]``: ``'slots'`` becomes K panels of ``slot_mode``, a bare name gets slot 0."""
    if slot_mode not in SLOT_MODES:
        raise ValueError(f"sheet: slot_mode must be one of {tuple(SLOT_MODES)}; got {slot_mode!r}")
    if isinstance(panels, str):
        panels = (panels,)
    out = []
    for p in panels:
        if p == 'slots':
            out += [(SLOT_MODES[slot_mode], k) for k in range(K)]
            continue
        name, k = (p, 0) if isinstance(p, str) else (p[0], int(p[1]))
        if name not in KINDS:
            raise ValueError(f"sheet: unknown panel {p!r}; panels are {tuple(KINDS)}, 'slots' and (slot kind, k)")
        if KINDS[name] >= KINDS['slot_masked'] and (isinstance(p, str) or not 0 <= k < K):
            raise ValueError(f'sheet: panel {p!r} needs a slot index in 0..{K - 1}, as ({name!r}, k)')
        out.append((name, k))
    if not 1 <= len(out) <= MAX_PANELS:
        raise ValueError(f'sheet: 1..{MAX_PANELS} panels per row, got {len(out)}')
    return out


def layout(rows: int, panels, K: int, S: int, scale: int = 1, pad: int = 2):
    """``(H, W, boxes)`` of a sheet: ``boxes[r][c] = (y0, x0, side)``, panel c of row r is ``sheet[y0:y0 + side, x0:x0 + side]``.
    ``H = pad + rows (S scale + pad)``, ``W = pad + C (S scale + pad)``.  Host arithmetic only."""
    n = len(expand_panels(panels, K))
    side = S * scale
    boxes = [[(pad + r * (side + pad), pad + c * (side + pad), side) for c in range(n)] for r in range(rows)]
    return pad + rows * (side + pad), pad + n * (side + pad), boxes


def _rgb8(v, name):
    v = tuple(int(c) for c in v)
    if len(v) != 3 or any(not 0 <= c <= 255 for c in v):
        raise ValueError(f'sheet: {name} must be three integers in 0..255; got {v}')
    return v


def _prepare(mask, mean, pred, x, gt, panels, slot_mode, scale, pad, pad_value, background, alpha, edges, edge, error_gain, colors,
             gt_colors):
    """The checked arguments of one launch: ``(spec, tensors (x, pred, mask, mean, gt, colors, gt_colors), lead)``"""
    given = {'mask': mask, 'mean': mean, 'pred': pred, 'x': x, 'gt': gt, 'colors': colors, 'gt_colors': gt_colors}
    for n, t in given.items():
        if t is not None and not isinstance(t, torch.Tensor):
            raise ValueError(f'sheet: {n} must be a torch tensor')
    if not isinstance(mask, torch.Tensor):
        raise ValueError('sheet: mask must be a torch tensor')
    if mask.dim() < 4 or mask.shape[-3] != 1 or mask.shape[-1] != mask.shape[-2]:
        raise ValueError(f'sheet: mask must be (*, K, 1, S, S), got {tuple(mask.shape)}')
    lead, K, S = tuple(mask.shape[:-4]), int(mask.shape[-4]), int(mask.shape[-1])
    if not 1 <= K <= MAX_SLOTS or not 1 <= S <= MAX_SIZE:
        raise ValueError(f'sheet: K must be in 1..{MAX_SLOTS} and S in 1..{MAX_SIZE}, got K = {K}, S = {S}')
    R = 1
    for d in lead:
        R *= int(d)
    if R < 1:
        raise ValueError(f'sheet: empty leading dimensions {lead}')
    if mean is not None and tuple(mean.shape) != lead + (K, 3, S, S):
        raise ValueError(f'sheet: mean must be {lead + (K, 3, S, S)} for this mask, got {tuple(mean.shape)}')
    if pred is not None and tuple(pred.shape) != lead + (3, S, S):
        raise ValueError(f'sheet: pred must be {lead + (3, S, S)} for this mask, got {tuple(pred.shape)}')
    if x is not None:
        if tuple(x.shape) == (3, S, S):
            x = x.expand(lead + (3, S, S))
        if tuple(x.shape) != lead + (3, S, S):
            raise ValueError(f'sheet: x must be {lead + (3, S, S)} or {(3, S, S)} for this mask, got {tuple(x.shape)}')
    G = 0
    if gt is not None:
        if gt.dtype != torch.uint8:
            raise ValueError(f'sheet: gt must be uint8 0/1 (pack_gt), got {gt.dtype}')
        if gt.dim() != len(lead) + 3 or tuple(gt.shape[:-3]) != lead or tuple(gt.shape[-2:]) != (S, S):
            raise ValueError(f'sheet: gt must be {lead + ("G", S, S)} for this mask, got {tuple(gt.shape)}')
        G = int(gt.shape[-3])
        if not 1 <= G <= MAX_SLOTS:
            raise ValueError(f'sheet: G must be in 1..{MAX_SLOTS}, got {G}')
    for n, t, w in (('colors', colors, K), ('gt_colors', gt_colors, G)):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != lead + (w,)):
            raise ValueError(f'sheet: {n} must be uint8 {lead + (w,)} palette indices, got {t.dtype} {tuple(t.shape)}')
    scale, pad = int(scale), int(pad)
    if not 1 <= scale <= 8 or not 0 <= pad <= 16:
        raise ValueError(f'sheet: scale must be in 1..8 and pad in 0..16, got {scale}, {pad}')
    plist = expand_panels(panels, K, slot_mode)
    needs = {'image': ('x',), 'pred': ('pred',), 'overlay': ('x',), 'gt': ('gt',), 'error': ('x', 'pred'), 'slot_masked': ('mean',),
             'slot_mean': ('mean',)}
    have = {'x': x, 'pred': pred, 'mean': mean, 'gt': gt}
    for name, _ in plist:
        for n in needs.get(name, ()):
            if have[n] is None:
                raise ValueError(f'sheet: panel {name!r} needs {n}=')
    if mask.device.type != 'cuda' or any(t is not None and t.device != mask.device for t in given.values()):
        raise RuntimeError('sheet needs mask (and the other inputs) on one ROCm device (no CPU fallback)')
    sp = _lib.SheetSpec(rows=R, slots=K, n_gt=G, size=S, scale=scale, pad=pad, n_panels=len(plist), draw_edges=1 if edges else 0,
                        alpha=float(alpha), error_gain=float(error_gain))
    sp.background[:] = [float(c) for c in background]
    sp.pad_value[:] = _rgb8(pad_value, 'pad_value')
    sp.edge[:] = _rgb8(edge, 'edge')
    for c, (name, k) in enumerate(plist):
        sp.panel_kind[c], sp.panel_slot[c] = KINDS[name], k
    sp.palette[:] = [c for rgb in PALETTE for c in rgb]
    f32 = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    u8 = lambda t: None if t is None else t.contiguous()
    return sp, (f32(x), f32(pred), f32(mask), f32(mean), u8(gt), u8(colors), u8(gt_colors)), lead


def sheet(mask, mean=None, pred=None, x=None, gt=None, panels=('image', 'pred', 'seg', 'slots'), slot_mode='masked', scale=1, pad=2,
          pad_value=(255, 255, 255), background=(1., 1., 1.), alpha=0.5, edges=True, edge=(255, 255, 255), error_gain=4.0, colors=None,
          gt_colors=None) -> torch.Tensor:
    """``mask (*, K, 1, S, S)`` and whatever the panels read -> the sheet, ``uint8 (H, W, 3)`` on the device, one row per entry of the
    leading dimensions (flattened in order) and one panel per entry of ``panels``; see ``layout`` for the boxes.  ``x (3, S, S)`` is
    repeated over the rows.  ``scale``: integer nearest-neighbour magnification 1..8; ``pad``: 0..16 pixels of ``pad_value`` around and
    between the panels.  ``colors (*, K)`` / ``gt_colors (*, G)``: uint8 palette indices of the slots / ground-truth rows (default: the
    identity; ``matched_colors``).  One launch, no synchronisation; two calls give equal bytes."""
    sp, tensors, _ = _prepare(mask, mean, pred, x, gt, panels, slot_mode, scale, pad, pad_value, background, alpha, edges, edge,
                              error_gain, colors, gt_colors)
    L = _lib.lib()
    h, w = C.c_int(), C.c_int()
    _lib.check(L.iodine_sheet_size(C.byref(sp), C.byref(h), C.byref(w)), None, 'iodine_sheet_size')
    dev = tensors[2].device
    out = torch.empty((h.value, w.value, 3), dtype=torch.uint8, device=dev)
    return render_into(out, sp, tensors)


def render_into(out, sp, tensors):
    """One launch of ``iodine_render_sheet`` into ``out`` (uint8, H W 3 bytes, contiguous) for a prepared spec; returns ``out``."""
    _lib.call('iodine_render_sheet', out.device, C.byref(sp), *tensors, out)
    return out


def sheet_form(out, sp, tensors) -> int:
    """Which forms of the kernel ``render_into(out, sp, tensors)`` runs: ``FORM_VECTOR_LOADS | FORM_WORD_STORES`` bits.  Host only."""
    form = _lib.lib().iodine_sheet_form(C.byref(sp), *[_lib.ptr(t) for t in tensors[:5]], _lib.ptr(out))
    if form < 0:
        _lib.check(1, None, 'iodine_sheet_form')
    return form


def matched_colors(mask, gt, cost='iou'):
    """``(colors (*, K), gt_colors (*, G))`` uint8 palette indices under which the ``seg`` and ``gt`` panels of a row compare by eye:
    ground-truth row g takes palette g and so does the slot ``matching.match_masks`` assigns to it; the other slots take, in slot order,
    the lowest indices no ground-truth row of the image uses; padding rows (no pixels) take 16.  Device ops only, no synchronisation."""
    from .matching import match_masks
    m = match_masks(mask, gt, cost=cost)
    lead, G, K = tuple(m.assign.shape[:-1]), int(m.assign.shape[-1]), int(mask.shape[-4])
    dev = mask.device
    asg = m.assign.reshape(-1, G).to(torch.int64)
    real = m.stats.gt_area.reshape(-1, G) > 0
    R = asg.shape[0]
    rows_g = torch.arange(G, device=dev).expand(R, G)
    gt_colors = torch.where(real, rows_g, torch.full_like(rows_g, NONE_COLOR))
    # matched slots: scatter g to column assign[g]; unmatched rows go to a spare column K
    col = torch.full((R, K + 1), -1, dtype=torch.int64, device=dev)
    col.scatter_(1, torch.where(asg >= 0, asg, torch.full_like(asg, K)), rows_g)
    col = col[:, :K]
    used = torch.zeros((R, 16), dtype=torch.int64, device=dev)
    used[:, :G] = real.to(torch.int64)
    free = torch.sort(used, dim=1, stable=True).indices      # the unused indices first, ascending
    open_ = col < 0
    rank = (torch.cumsum(open_.to(torch.int64), 1) - 1).clamp_min(0)
    col = torch.where(open_, free.gather(1, rank), col)
    return col.to(torch.uint8).reshape(lead + (K,)), gt_colors.to(torch.uint8).reshape(lead + (G,))


def _with_gt(kw, mask, gt):
    """``gt`` as a device tensor and, unless given, the ``gt`` panel after ``pred`` and matched colours"""
    from .matching import pack_gt
    gt = pack_gt(gt, size=int(mask.shape[-1]), device=mask.device)
    if 'panels' not in kw:
        kw['panels'] = ('image', 'pred', 'gt', 'seg', 'slots')
    if 'colors' not in kw and 'gt_colors' not in kw:
        kw['colors'], kw['gt_colors'] = matched_colors(mask, gt)
    return gt


@torch.no_grad()
def decomposition(model, x, gt=None, n=8, trajectory=None, eps=None, **kw):
    """Run ``model.reconstruct`` on the first ``n`` images of ``x (B, 3, S, S)`` and return their sheet, one row per image.  ``gt``: the
    images' ground-truth masks (``pack_gt`` input or ``(B, G, S, S)`` uint8): adds the ``gt`` panel and matched colours.
    ``trajectory=b``: reconstruct image b alone with ``trajectory=True`` and return the refinement figure, one row per decode (T + 1).
    ``eps``: the normals of the call (``reconstruct``'s ``eps``); ``**kw`` goes to ``sheet``."""
    if trajectory is not None:
        b = int(trajectory)
        if not 0 <= b < x.shape[0]:
            raise ValueError(f'decomposition: trajectory must be an image index in 0..{x.shape[0] - 1}; got {trajectory!r}')
        model.reconstruct(x[b:b + 1], eps=eps, trajectory=True)
        g = None if gt is None else (gt[b:b + 1] if isinstance(gt, torch.Tensor) else [gt[b]])
        return trajectory_sheet(model.trajectory, image=0, x=x[b], gt=g, **kw)
    n = max(1, min(int(n), int(x.shape[0])))
    pred, mask, mean = model.reconstruct(x[:n], eps=eps)
    if gt is not None:
        gt = _with_gt(kw, mask, gt[:n] if isinstance(gt, torch.Tensor) else list(gt)[:n])
    return sheet(mask, mean=mean, pred=pred, x=x[:n].to(mask.device), gt=gt, **kw)


def trajectory_sheet(trajectory, image=0, x=None, gt=None, **kw):
    """The refinement figure of image ``image`` from ``model.trajectory`` (``reconstruct(x, trajectory=True)``): one row per decode, T + 1
    rows, the last the final decode.  ``x``: that image ``(3, S, S)``, or the batch ``(B, 3, S, S)``; without it the default panels drop
    ``'image'``.  ``gt``: the ground truth of that image (one entry), repeated over the rows."""
    if not isinstance(trajectory, dict) or not {'pred', 'mask', 'mean'} <= set(trajectory):
        raise ValueError('trajectory_sheet: need model.trajectory of reconstruct(x, trajectory=True)')
    B = int(trajectory['mask'].shape[1])
    b = int(image)
    if not 0 <= b < B:
        raise ValueError(f'trajectory_sheet: image must be an index in 0..{B - 1}; got {image!r}')
    pred, mask, mean = (trajectory[n][:, b] for n in ('pred', 'mask', 'mean'))
    if x is not None and x.dim() == 4:
        x = x[b]
    if gt is not None:
        from .matching import pack_gt
        if isinstance(gt, torch.Tensor) and gt.dim() == 4 and gt.shape[0] == B:
            gt = gt[b:b + 1]
        gt = pack_gt(gt, size=int(mask.shape[-1]), device=mask.device)
        if gt.shape[0] != 1:
            raise ValueError(f'trajectory_sheet: gt must be the masks of image {b} alone (or of the whole batch of {B}), got {gt.shape[0]} entries')
        gt = gt.expand((mask.shape[0],) + tuple(gt.shape[1:])).contiguous()       # the same ground truth in every row
        if 'colors' not in kw and 'gt_colors' not in kw:
            kw['colors'], kw['gt_colors'] = matched_colors(mask, gt)              # matched per row: a slot may change its object on the way
    if 'panels' not in kw:
        kw['panels'] = (('image',) if x is not None else ()) + ('pred',) + (('gt',) if gt is not None else ()) + ('seg', 'slots')
    return sheet(mask, mean=mean, pred=pred, x=None if x is None else x.to(mask.device), gt=gt, **kw)


def restarts_sheet(res, image=0, x=None, **kw):
    """The multi-stability figure of image ``image`` from ``model.restarts(x, chains=C, keep_decodes=True)``: one row per chain, C rows,
    with the slot colours following ``res.perm`` - slot i of chain c takes the palette entry of the slot of the best chain it is matched
    to, so that equal objects have equal colours down the rows.  ``x``: that image ``(3, S, S)``, or the batch ``(B, 3, S, S)``; without it
    the default panels drop ``'image'``.  The existing ``sheet``, one launch; ``**kw`` goes to it."""
    if getattr(res, 'decodes', None) is None or getattr(res, 'perm', None) is None:
        raise ValueError('restarts_sheet: need the result of model.restarts(x, consensus=True, keep_decodes=True)')
    pred, mask, mean = res.decodes
    B = int(mask.shape[1])
    b = int(image)
    if not 0 <= b < B:
        raise ValueError(f'restarts_sheet: image must be an index in 0..{B - 1}; got {image!r}')
    if x is not None and x.dim() == 4:
        x = x[b]
    if 'colors' not in kw:
        kw['colors'] = res.perm[:, b].clamp(0, NONE_COLOR).to(torch.uint8)        # (an unmatched slot, -1, would not occur: K rows, K columns)
    if 'panels' not in kw:
        kw['panels'] = (('image',) if x is not None else ()) + ('pred', 'seg', 'slots')
    return sheet(mask[:, b], mean=mean[:, b], pred=pred[:, b], x=None if x is None else x.to(mask.device), **kw)


def quantise(v: torch.Tensor) -> torch.Tensor:
    """The sheet's rule for one channel value on any float tensor: ``uint8(int(clamp(v) * 255 + 0.5))`` in float32, NaN -> 0."""
    v = v.detach().to(torch.float32)
    v = torch.where(v > 0, torch.where(v < 1, v, torch.ones_like(v)), torch.zeros_like(v))
    return (v * 255.0 + 0.5).to(torch.int32).to(torch.uint8)


def encode_png(sheet) -> bytes:
    """A ``uint8 (H, W, 3)`` tensor (any device: one copy to the host) or array as an 8-bit RGB PNG, filter type 0 on every row."""
    a = sheet.detach().cpu().numpy() if isinstance(sheet, torch.Tensor) else np.asarray(sheet)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'encode_png: need uint8 (H, W, 3) with H, W >= 1, got {a.dtype} {a.shape}')
    H, W = int(a.shape[0]), int(a.shape[1])
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)            # a filter byte (0 = none) in front of every row
    rows[:, 1:] = a.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)

    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))


def write_png(path, sheet) -> None:
    with open(path, 'wb') as f:
        f.write(encode_png(sheet))
