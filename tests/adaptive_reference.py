"""numpy float64 definition of the adaptive stopping rule (include/iodine_hip.h: iodine_adaptive_ctl, iodine_adaptive_select,
iodine_reconstruct_adaptive), shared by tests/test_adaptive_cpu.py and tests/test_gpu_adaptive.py.

``ll[i, b]``, ``kl[i, b]``: the fp32 per-image terms of ELBO evaluation i (what ``trajectory['ll']`` / ``['kl']`` hold);
``s_i(b) = double(ll) - beta * double(kl)``; R = ``check_every``.  Decisions are taken after t in {R, 2R, ..}, t < max_iters, updates.  After
t updates image b stops when ``t >= budget[b]`` (with a budget), or when ``t >= max(min_iters, 2)`` and

    s_{t-1} - s_{t-2} < tol + rtol * |s_{t-2}|

evaluated in fp64 in that order: one multiply, one add, one subtract, one compare (numpy has no fused multiply-add).  A non-finite value on
either side makes the comparison false - the image continues.  At t = max_iters every remaining image stops."""
import numpy as np


def score(ll, kl, beta):
    return np.asarray(ll, np.float32).astype(np.float64) - np.float64(beta) * np.asarray(kl, np.float32).astype(np.float64)


def stops(s_prev, s_last, tol, rtol):
    """the comparison alone, elementwise (NaN -> False)"""
    s_prev, s_last = np.asarray(s_prev, np.float64), np.asarray(s_last, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return (s_last - s_prev) < (np.float64(tol) + np.float64(rtol) * np.abs(s_prev))


def decide(t, s, max_iters, min_iters=2, check_every=1, tol=-np.inf, rtol=0.0, budget=None):
    """bool (B): which images stop after t updates, given ``s (>= t, B)`` (rows 0 .. t-1 are read).  Every image at t >= max_iters; none
    at a t that is no multiple of check_every."""
    s = np.asarray(s, np.float64)
    B = s.shape[1]
    if t >= max_iters:
        return np.ones(B, bool)
    if t % check_every != 0:
        return np.zeros(B, bool)
    out = np.zeros(B, bool)
    if budget is not None:
        out |= t >= np.asarray(budget)
    if t >= max(min_iters, 2):
        out |= stops(s[t - 2], s[t - 1], tol, rtol)
    return out


def iterations(ll, kl, beta, max_iters, min_iters=2, check_every=1, tol=-np.inf, rtol=0.0, budget=None):
    """``iters (B)`` int32 and ``active`` (list: the batch each round ran at) from a fixed ``max_iters``-iteration trajectory ``ll``,
    ``kl (max_iters, B)`` - images are independent of the batch they sit in, so an image's scores up to its stop are those of the fixed run."""
    s = score(ll, kl, beta)
    B = s.shape[1]
    iters = np.zeros(B, np.int32)
    alive = np.ones(B, bool)
    active = []
    t = 0
    while t < max_iters and alive.any():
        active.append(int(alive.sum()))
        t = min(t + check_every, max_iters)
        stop = decide(t, s, max_iters, min_iters, check_every, tol, rtol, budget) & alive
        iters[stop] = t
        alive &= ~stop
    n_rounds = -(-max_iters // check_every)
    return iters, active + [0] * (n_rounds - len(active))


def select(terms, idx, t, B, ll, kl, iters, max_iters, min_iters, check_every, tol, rtol, beta, budget=None):
    """iodine_adaptive_select in numpy: ``terms (R, n, 2)`` fp32, ``idx (n)`` original indices or None; the traces ``ll``, ``kl (max_iters,
    B)`` and ``iters (B)`` are updated in place.  Returns (idx_out, pos_out, stop_idx, stop_pos), each in position order."""
    terms = np.asarray(terms, np.float32)
    R, n = terms.shape[:2]
    idx = np.arange(n) if idx is None else np.asarray(idx)
    for r in range(R):
        ll[t - R + r, idx] = terms[r, :, 0]
        kl[t - R + r, idx] = terms[r, :, 1]
    s = np.full((t, B), np.nan)
    for i in (t - 2, t - 1):
        if i >= 0:
            s[i, idx] = score(ll[i, idx], kl[i, idx], beta)
    stop = decide(t, s, max_iters, min_iters, check_every, tol, rtol, budget)[idx]
    pos = np.arange(n)
    iters[idx[stop]] = t
    return idx[~stop].astype(np.int32), pos[~stop].astype(np.int32), idx[stop].astype(np.int32), pos[stop].astype(np.int32)


def move(entries):
    """iodine_adaptive_move in numpy: (src, dst, src_index, dst_index, rows) with 2-D arrays; dst is updated in place"""
    for src, dst, si, di, rows in entries:
        r = np.arange(rows)
        dst[r if di is None else np.asarray(di)[:rows]] = src[r if si is None else np.asarray(si)[:rows]]
