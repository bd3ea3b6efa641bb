"""Host-only argument checks of the ``IODINE`` entry points: plain functions of what they need, run before any device work.  Their
error texts are part of the interface (tests match on them)."""
import math
import numbers

import torch

from . import _lib


def all_tensors(values, message):
    """ValueError(message) unless every entry of ``values`` is a torch tensor"""
    if any(not isinstance(t, torch.Tensor) for t in values):
        raise ValueError(message)


def one_device(tensors, message):
    """RuntimeError(message) unless the tensors share one ROCm device (the stateless kernels have no CPU path)"""
    if tensors[0].device.type != 'cuda' or any(t.device != tensors[0].device for t in tensors[1:]):
        raise RuntimeError(message)


def lead_count(lead, message):
    """The product of the leading dimensions ``lead``, ValueError(message) when it is < 1"""
    n = math.prod(int(d) for d in lead)
    if n < 1:
        raise ValueError(message)
    return n


def run_shape(K, T):
    """(K, T) of the call that is starting - ``model.K`` / ``model.n_iters``, read like the reference reads them on every call
    (iodine.py:81-83,123-126,279,312) -, checked on the host before any device work."""
    if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= 16:
        raise ValueError(f'IODINE: the slot count (model.K) must be an integer in 1..16 - the per-pixel kernels keep every slot of '
                         f'a pixel in registers, instantiated for K <= 16; got {K!r}')
    if isinstance(T, bool) or int(T) != T or int(T) < 1:
        raise ValueError(f'IODINE: the iteration count (model.n_iters) must be an integer >= 1; got {T!r}')
    return int(K), int(T)


def _number(v, name, rule, ok):
    # a Python or numpy real number, or a tensor / array with one element - what a schedule usually produces
    if torch.is_tensor(v) and v.numel() == 1 and not v.is_complex():
        v = v.detach().item()
    elif not isinstance(v, numbers.Real) and getattr(v, 'size', None) == 1 and hasattr(v, 'item'):
        v = v.item()
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f'IODINE: model.{name} must be a finite number {rule}, given as a real number or a one-element '
                         f'tensor; got {v!r} of type {type(v).__name__}')
    if not math.isfinite(v) or not ok(v):
        raise ValueError(f'IODINE: model.{name} must be a finite number {rule}; got {v!r}')
    return float(v)


_ITER_WEIGHTS = "IODINE: model.iter_weights must be None, 'linspace', 'uniform', 'last' or a sequence of T + 1 numbers; "


def read_objective(sigma, beta, iter_weights, T):
    """(sigma, beta, weights) of the call that is starting at ``T`` iterations, from ``model.sigma`` / ``beta`` / ``iter_weights``, which
    are read like K / n_iters; weights: () = the default (i+1)/(T+1), else T + 1 floats.  ValueError for anything the library would refuse.  Every entry point reads all three "at call time", so explicit
    ``iter_weights`` of the training length make encode / reconstruct / elbo at ANOTHER ``n_iters`` raise the length error although
    inference never uses the weights, and a named weighting sends its table for the T of an inference call too - set
    ``iter_weights = None`` (or a name) around evaluation at another iteration count."""
    sigma = _number(sigma, 'sigma', '> 0 (the likelihood scale)', lambda v: v > 0)
    beta = _number(beta, 'beta', '>= 0 (the weight of the KL term)', lambda v: v >= 0)
    w = iter_weights
    if w is None or (isinstance(w, str) and w == 'linspace'):
        return sigma, beta, ()
    if isinstance(w, str):
        if w == 'uniform':
            return sigma, beta, (1.0 / (T + 1),) * (T + 1)
        if w == 'last':
            return sigma, beta, (0.0,) * T + (1.0,)
        raise ValueError(_ITER_WEIGHTS + f'got {w!r}')
    if torch.is_tensor(w):
        w = w.detach().reshape(-1).tolist()
    try:
        w = tuple(w)
    except TypeError:
        raise ValueError(_ITER_WEIGHTS + f'got {w!r}') from None
    if len(w) != T + 1:
        raise ValueError(f'IODINE: model.iter_weights has {len(w)} entries, but a call at n_iters = {T} makes {T + 1} ELBO '
                         f'evaluations and takes {T + 1} weights (or one of the names, which follow n_iters)')
    w = tuple(_number(v, 'iter_weights[%d]' % i, '>= 0', lambda v: v >= 0) for i, v in enumerate(w))
    if not any(_lib.as_float32(v) > 0 for v in w):
        raise ValueError(f'IODINE: model.iter_weights are all zero (as float32) - no evaluation would carry any loss; got {w!r}')
    return sigma, beta, w


def check_x(x, channels, size):
    if x.dim() != 4 or x.shape[1] != channels or x.shape[2] != size or x.shape[3] != size:
        raise RuntimeError(f'expected images of shape (B, {channels}, {size}, {size}), got {tuple(x.shape)}')
    return x.detach().to(torch.float32).contiguous()


def check_frames(x, E, what, c, s, n_iters):
    """``x`` of a call that makes ``E`` ELBO evaluations -> (x, frames): images (B, C, S, S) -> frames 0; a clip (B, E, C, S, S),
    batch first, one frame per evaluation -> frames E.  Any other frame count is refused - never clamped or repeated."""
    if x.dim() != 5:
        return check_x(x, c, s), 0
    if tuple(x.shape[1:]) != (E, c, s, s):
        raise RuntimeError(f'{what} at n_iters = {n_iters} makes {E} ELBO evaluations: expected a clip of shape '
                           f'(B, {E}, {c}, {s}, {s}), one frame per evaluation, or images (B, {c}, {s}, {s}); got {tuple(x.shape)}')
    return x.detach().to(torch.float32).contiguous(), E


def check_weights(weights, x, img_size, what):
    """``weights=`` of a call on ``x`` (as given: images (B, C, S, S) or a clip (B, E, C, S, S)) -> None, or contiguous float32 on
    x's device: (B, S, S), or (B, E, S, S) for one weight image per frame.  Accepted: (B, 1, S, S) / (B, S, S), with a clip also
    (B, E, 1, S, S) / (B, E, S, S) - a 4-D (B, 1, S, S) weight goes to every frame.  Refused before any device work, like
    ``check_frames``; the values (finite, >= 0) are the caller's contract.  Weights are data: detached."""
    if weights is None:
        return None
    if not torch.is_tensor(weights):
        raise RuntimeError(f'IODINE.{what}: weights must be a tensor of per-pixel weights (bool, uint8 or a float dtype), or None; got '
                           f'{type(weights).__name__}')
    if not (weights.dtype in (torch.bool, torch.uint8) or weights.is_floating_point()):
        raise RuntimeError(f'IODINE.{what}: weights must have dtype bool, uint8 or a float dtype; got {weights.dtype}')
    B, s = x.shape[0], img_size
    E = x.shape[1] if x.dim() == 5 else None
    got = tuple(weights.shape)
    per_frame = False
    if got in ((B, 1, s, s), (B, s, s)):
        pass
    elif E is not None and got in ((B, E, 1, s, s), (B, E, s, s)):
        per_frame = True
    else:
        if weights.dim() == 5 and E is None:
            raise RuntimeError(f'IODINE.{what}: weights of shape {got} hold one weight image per frame, but x {tuple(x.shape)} is a '
                               f'batch of single images: expected weights ({B}, 1, {s}, {s}) or ({B}, {s}, {s})')
        clip = f', or ({B}, {E}, 1, {s}, {s}) / ({B}, {E}, {s}, {s}) - one weight image per frame' if E is not None else ''
        raise RuntimeError(f'IODINE.{what}: weights must have shape ({B}, 1, {s}, {s}) or ({B}, {s}, {s}){clip}, matching x '
                           f'{tuple(x.shape)}; got {got}')
    w = weights.detach().to(device=x.device, dtype=torch.float32)
    return w.reshape((B, E, s, s) if per_frame else (B, s, s)).contiguous()


def check_state(state, B, K, L, H, device, train=False):
    """``state=``: (post_mean, post_logvar (B, K, L), h, c (B, K, H = MLP_UNITS)) as refinement_state returns it -> float32 contiguous on
    ``device``, detached.  ``train`` (``forward``): h / c may also come as the reference's (B * K, H) (``lstm_hidden``, iodine.py:37),
    and nothing is detached - tensors that require grad stay connected to the caller's graph."""
    if state is None:
        return None
    if not isinstance(state, (tuple, list)) or len(state) != 4 or any(not torch.is_tensor(t) for t in state):
        raise RuntimeError('state must be the tuple (post_mean, post_logvar, h, c) that model.refinement_state() returns')
    want = ((B, K, L), (B, K, L), (B, K, H), (B, K, H))
    got = tuple(tuple(t.shape) for t in state)
    if train:
        if not (got[:2] == want[:2] and all(g in ((B, K, H), (B * K, H)) for g in got[2:])):
            raise RuntimeError(f'state does not match this call: (B, K) = ({B}, {K}) needs post_mean, post_logvar of shape {(B, K, L)} and '
                               f'h, c of shape {(B, K, H)} (or {(B * K, H)}, as model.lstm_hidden); got {got}')
        return tuple(t.to(device=device, dtype=torch.float32).reshape(shp).contiguous() for t, shp in zip(state, want))
    if got != want:
        raise RuntimeError(f'state does not match this call: (B, K) = ({B}, {K}) needs tensors of shapes {want}, got {got}')
    return tuple(t.detach().to(device=device, dtype=torch.float32).contiguous() for t in state)


def check_attach_frames(attach_frames, T):
    """``attach_frames`` of ``forward`` -> None (off) or the sorted tuple of evaluation indices.  Host only."""
    if attach_frames is None or attach_frames is False:
        return None
    if attach_frames is True:
        return tuple(range(T + 1))
    try:
        vals = list(attach_frames)
    except TypeError:
        raise ValueError(f'IODINE.forward: attach_frames must be None, a bool or an iterable of evaluation indices in 0..{T}; got '
                         f'{attach_frames!r}') from None
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= T:
            raise ValueError(f'IODINE.forward: attach_frames holds {v!r}; a forward of {T} iterations makes the ELBO evaluations 0..{T}')
    if len(set(vals)) != len(vals):
        raise ValueError(f'IODINE.forward: attach_frames names an evaluation twice: {vals!r}')
    return tuple(sorted(vals))


def int_list(v, name, E=None):
    """An int sequence or integer tensor of edits -> list of Python ints (host values: the library checks them before any launch)."""
    if torch.is_tensor(v):
        if v.dim() != 1 or v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f'IODINE.edit: {name} must be a 1-D integer tensor or a sequence of ints; got {v.dtype} of shape {tuple(v.shape)}')
        v = v.detach().cpu().tolist()
    else:
        try:
            v = list(v)
        except TypeError:
            raise ValueError(f'IODINE.edit: {name} must be a sequence of ints or a 1-D integer tensor; got {type(v).__name__}') from None
        if any(isinstance(i, bool) or int(i) != i for i in v):
            raise ValueError(f'IODINE.edit: {name} must hold integers; got {v!r}')
        v = [int(i) for i in v]
    if E is not None and len(v) != E:
        raise ValueError(f'IODINE.edit: {name} has {len(v)} entries, but there are {E} edits (one entry per edit)')
    return v
