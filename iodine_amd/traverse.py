"""Latent traversals: the disentanglement figures of a slot model in one call.

The recipe is the reference's (notes.md, README "disentanglement"): take the ``z, mu, logvar`` of one image, rank the latent units of a
slot by their KL against N(0, 1), vary one unit at a time and decode.  Every such scene differs from the base in one latent of ONE slot,
so ``traverse`` hands the whole list to ``IODINE.edit``: the base is decoded once and each variation decodes a single slot-image.

``latent_kl`` / ``rank_dims`` / ``build_edits`` are plain torch and run anywhere; ``traverse`` needs the model on its ROCm device.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

MODES = ('set', 'add', 'sigma')


def latent_kl(post_mean: torch.Tensor, post_logvar: torch.Tensor) -> torch.Tensor:
    """KL(N(m, exp(lv)) || N(0, 1)) per latent unit, ``0.5 (exp(lv) + m^2 - 1 - lv)`` (iodine.py:653-659 before its sum); shape preserved."""
    return 0.5 * (post_logvar.exp() + post_mean * post_mean - 1.0 - post_logvar)


def rank_dims(post_mean: torch.Tensor, post_logvar: torch.Tensor, top: Optional[int] = None) -> torch.Tensor:
    """Indices ``(..., top)`` of the latent units by descending KL (``top=None``: all L).  Stable: on a tie the lowest index comes first."""
    kl = latent_kl(post_mean, post_logvar)
    L = kl.shape[-1]
    if top is None:
        top = L
    if isinstance(top, bool) or int(top) != top or not 1 <= int(top) <= L:
        raise ValueError(f'rank_dims: top must be an integer in 1..{L} (the latent width); got {top!r}')
    return torch.sort(kl, dim=-1, descending=True, stable=True).indices[..., :int(top)]


def build_edits(z_row: torch.Tensor, slots, dims, values: torch.Tensor, mode: str = 'set', posterior=None):
    """The edit list of a traversal of ONE image: ``z_row (K, L)`` -> ``(slot (E,) int64, z_new (E, L))`` with E = n_slots x n_dims x V,
    ordered by slot, then unit, then value.  ``dims (n_slots, n_dims)``: the units varied in each slot; row e of ``z_new`` is the slot's
    latent with unit d set to v (``'set'``), moved by v (``'add'``) or set to ``mu[d] + v exp(logvar[d] / 2)`` (``'sigma'``, which needs
    ``posterior = (mean, logvar)``, each (K, L))."""
    if mode not in MODES:
        raise ValueError(f'traverse: mode must be one of {MODES}; got {mode!r}')
    if z_row.dim() != 2:
        raise ValueError(f'traverse: the latents of one image must be (K, L); got {tuple(z_row.shape)}')
    K, L = z_row.shape
    slots = [int(s) for s in slots]
    dims = torch.as_tensor(dims, dtype=torch.int64).cpu()
    if dims.dim() != 2 or dims.shape[0] != len(slots) or dims.shape[1] < 1:
        raise ValueError(f'traverse: dims must be (n_slots, n_dims) = ({len(slots)}, >= 1); got {tuple(dims.shape)}')
    if any(not 0 <= s < K for s in slots):
        raise ValueError(f'traverse: slots must lie in 0..{K - 1} (z has shape (.., {K}, {L})); got {slots}')
    if int(dims.min()) < 0 or int(dims.max()) >= L:
        raise ValueError(f'traverse: dims must lie in 0..{L - 1} (z has shape (.., {K}, {L})); got {dims.tolist()}')
    values = torch.as_tensor(values, dtype=z_row.dtype).to(z_row.device).reshape(-1)
    if values.numel() < 1:
        raise ValueError('traverse: values is empty')
    if mode == 'sigma':
        if posterior is None:
            raise ValueError("traverse: mode 'sigma' moves a unit along its posterior, mu + v exp(logvar / 2): pass posterior=(mean, logvar)")
        pm, plv = (_posterior_rows(t, z_row, 'posterior') for t in posterior)
    n_s, n_d, V = len(slots), int(dims.shape[1]), int(values.numel())
    z_new = z_row[slots].reshape(n_s, 1, 1, L).repeat(1, n_d, V, 1)                 # (n_s, n_d, V, L): copies of the slot's latent
    idx = dims.to(z_row.device).reshape(n_s, n_d, 1, 1).expand(n_s, n_d, V, 1)
    v = values.reshape(1, 1, V, 1).expand(n_s, n_d, V, 1)
    if mode == 'add':
        v = z_new.gather(3, idx) + v
    elif mode == 'sigma':
        sl = torch.as_tensor(slots, device=z_row.device)
        v = pm[sl].reshape(n_s, 1, 1, L).expand(n_s, n_d, V, L).gather(3, idx) + v * (0.5 * plv[sl]).exp().reshape(n_s, 1, 1, L).expand(n_s, n_d, V, L).gather(3, idx)
    z_new.scatter_(3, idx, v)
    slot = torch.as_tensor(slots, dtype=torch.int64).reshape(n_s, 1, 1).expand(n_s, n_d, V).reshape(-1)
    return slot, z_new.reshape(n_s * n_d * V, L)


def _posterior_rows(t, z_row, name):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(z_row.shape):
        raise ValueError(f'traverse: {name} must be (mean, logvar) of shape {tuple(z_row.shape)} each; got '
                         f'{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}')
    return t.detach().to(device=z_row.device, dtype=z_row.dtype)


@dataclasses.dataclass
class Traversal:
    """``pred (n_slots, n_dims, V, 3, S, S)``: entry [i, j, v] = the scene with unit ``dims[i, j]`` of slot ``slots[i]`` at ``values[v]``;
    ``mask (n_slots, n_dims, V, K, 1, S, S)`` or None; ``base`` = (pred (3, S, S), mask (K, 1, S, S), mean (K, 3, S, S)) of the unedited image."""
    pred: torch.Tensor
    mask: Optional[torch.Tensor]
    slots: list
    dims: torch.Tensor
    values: torch.Tensor
    base: tuple

    def grid(self, i: int, transpose: bool = False) -> torch.Tensor:
        """The traversal of slot ``slots[i]`` as one image ``(3, n_dims S, V S)``: rows are units, columns are values.  ``transpose=True``:
        ``(3, V S, n_dims S)``, one column per unit with the values running down - the layout of the reference's README figures."""
        t = self.pred[i]                                         # (n_dims, V, 3, S, S)
        if transpose:
            t = t.transpose(0, 1)
        r, c, ch, S, _ = t.shape
        return t.permute(2, 0, 3, 1, 4).reshape(ch, r * S, c * S)

    def save_png(self, path, i: int, transpose: bool = False) -> None:
        """``grid(i, transpose)`` as an 8-bit RGB PNG: every channel value quantised by the rule of the decomposition sheets
        (``figures.quantise``: clamp to [0, 1], ``int(v * 255 + 0.5)``, NaN -> 0), one copy to the host."""
        from .figures import quantise, write_png
        write_png(path, quantise(self.grid(i, transpose)).permute(1, 2, 0).contiguous())


def traverse(model, z, *, image: int = 0, slots=None, dims=None, values=None, mode: str = 'set', posterior=None, top: int = 8,
             return_mask: bool = False) -> Traversal:
    """Traverse latent units of image ``image`` of the scene ``z (B, K, L)`` with ONE ``model.edit`` call.

    ``slots``: the slots to traverse (default all K); ``dims``: a list of units used for every slot, or None = the ``top`` units of each
    slot by KL (``rank_dims`` of ``posterior = (mean, logvar)``, each (B, K, L) - required then, and for mode ``'sigma'``); ``values``:
    default ``torch.linspace(-2, 2, 7)``; ``mode``: ``'set'`` z[d] = v, ``'add'`` z[d] += v, ``'sigma'`` z[d] = mu[d] + v exp(logvar[d] / 2).
    Not differentiable (see ``IODINE.edit``)."""
    if not torch.is_tensor(z) or z.dim() != 3:
        raise ValueError(f'traverse: z must be (B, K, L); got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}')
    B, K, L = z.shape
    if isinstance(image, bool) or int(image) != image or not 0 <= int(image) < B:
        raise ValueError(f'traverse: image must be an index in 0..{B - 1} (z has shape {tuple(z.shape)}); got {image!r}')
    image = int(image)
    slots = list(range(K)) if slots is None else [int(s) for s in slots]
    if not slots:
        raise ValueError('traverse: slots is empty')
    post_row = None
    if posterior is not None:
        if len(posterior) != 2 or any(not torch.is_tensor(t) or tuple(t.shape) != tuple(z.shape) for t in posterior):
            raise ValueError(f'traverse: posterior must be (mean, logvar) of shape {tuple(z.shape)} each')
        post_row = tuple(t.detach()[image] for t in posterior)
    if dims is None:
        if post_row is None:
            raise ValueError('traverse: dims=None ranks the units of each slot by KL and needs posterior=(mean, logvar); or pass dims')
        if any(not 0 <= s < K for s in slots):
            raise ValueError(f'traverse: slots must lie in 0..{K - 1}; got {slots}')
        dims_t = rank_dims(post_row[0], post_row[1], top)[slots].cpu()
    else:
        dims_t = torch.as_tensor(list(dims), dtype=torch.int64).reshape(1, -1).repeat(len(slots), 1)
    values = torch.linspace(-2.0, 2.0, 7) if values is None else torch.as_tensor(values, dtype=torch.float32).reshape(-1)
    zd = z.detach().to(torch.float32)
    slot, z_new = build_edits(zd[image], slots, dims_t, values, mode, post_row)
    E = int(slot.numel())
    out = model.edit(zd, [image] * E, slot.tolist(), z_new, return_mask=return_mask, return_base=True)
    n_s, n_d, V = len(slots), int(dims_t.shape[1]), int(values.numel())
    S = out.pred.shape[-1]
    return Traversal(pred=out.pred.reshape(n_s, n_d, V, 3, S, S),
                     mask=out.mask.reshape(n_s, n_d, V, K, 1, S, S) if return_mask else None,
                     slots=slots, dims=dims_t, values=values, base=tuple(t[image] for t in out.base))
