"""numpy definition of ``iodine_chain_score`` and ``iodine_chain_consensus`` (include/iodine_hip.h), shared by tests/test_restarts_cpu.py and
tests/test_gpu_restarts.py: float64 for ``ll`` and ``mask_mean``, integers for everything else.  Written from the header alone - plain loops
over chains and slots, no trick the kernels use."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


def pixel_ll(x, mask, mean, sigma, joint):
    """LL_p of one decode: x (B,3,S,S), mask (B,K,1,S,S), mean (B,K,3,S,S) -> (B,S,S) float64.
    l_kc = -(x_c - mu_kc)^2 / (2 sigma^2) - ln sigma - ln(2 pi) / 2; per channel: sum_c logsumexp_k(log(m_k + 1e-12) + l_kc); joint:
    logsumexp_k(log(m_k + 1e-12) + sum_c l_kc).  The maximum is subtracted inside the logsumexp."""
    x, mask, mean, sigma = np.asarray(x, np.float64), np.asarray(mask, np.float64), np.asarray(mean, np.float64), float(sigma)
    l = -(x[:, None] - mean) ** 2 / (2.0 * sigma * sigma) - np.log(sigma) - 0.5 * LOG_2PI          # (B,K,3,S,S)
    a = np.log(mask + 1e-12) + (l.sum(2, keepdims=True) if joint else l)                            # (B,K,1 or 3,S,S)
    top = a.max(1, keepdims=True)
    lse = top[:, 0] + np.log(np.exp(a - top).sum(1))                                                # (B,1 or 3,S,S)
    return lse.sum(1)


def chain_score(x, w, mask, mean, sigma, joint):
    """x (B,3,S,S), w (B,S,S) or None, mask (C,B,K,1,S,S), mean (C,B,K,3,S,S) -> ll (C,B) float64, scale (C,B) = sum_p |w_p LL_p|,
    seg (C,B,S,S) uint8.  seg: `v > best` from slot 0 upwards from -inf: the lowest index wins a tie and a NaN never wins."""
    mask = np.asarray(mask)
    C, B, K = mask.shape[:3]
    S = mask.shape[-1]
    wt = np.ones((B, S, S)) if w is None else np.asarray(w, np.float64)
    ll, scale = np.zeros((C, B)), np.zeros((C, B))
    seg = np.zeros((C, B, S, S), np.uint8)
    for c in range(C):
        t = wt * pixel_ll(x, mask[c], mean[c], sigma, joint)
        ll[c], scale[c] = t.sum((1, 2)), np.abs(t).sum((1, 2))
        best = np.full((B, S, S), -np.inf, mask.dtype)
        for k in range(K):
            v = mask[c, :, k, 0]
            with np.errstate(invalid='ignore'):
                win = v > best
            best = np.where(win, v, best)
            seg[c] = np.where(win, k, seg[c])
    return ll, scale, seg


def top_two_gap(mask):
    """the smallest difference between the largest and the second largest mask value of a pixel (inf for K = 1): > 0 means no ties"""
    m = np.sort(np.asarray(mask, np.float64), axis=-4)
    return np.inf if m.shape[-4] < 2 else float((m[..., -1, :, :, :] - m[..., -2, :, :, :]).min())


def relabel(seg, perm):
    """t (C,B,P) int64: perm[c, b, seg[c, b, p]], or -1 where the label is >= K or the perm entry outside 0..K-1"""
    seg, perm = np.asarray(seg), np.asarray(perm)
    C, B = seg.shape[:2]
    K = perm.shape[2]
    lab = seg.reshape(C, B, -1).astype(np.int64)
    t = np.full(lab.shape, -1, np.int64)
    for c in range(C):
        for b in range(B):
            ok = lab[c, b] < K
            v = perm[c, b][np.where(ok, lab[c, b], 0)].astype(np.int64)
            t[c, b] = np.where(ok & (v >= 0) & (v < K), v, -1)
    return t


def chain_consensus(seg, perm, ref=None, mask=None):
    """seg (C,B,S,S) uint8, perm (C,B,K) int, ref (B) int or None, mask (C,B,K,1,S,S) or None -> dict(votes (B,K,P) int64, consensus (B,P)
    uint8, agreement (B,P) float32 = float32(top) / float32(C), match (C,B) float32 = float32(count / P), mask_mean (B,K,P) float64)."""
    seg, perm = np.asarray(seg), np.asarray(perm)
    C, B = seg.shape[:2]
    K = perm.shape[2]
    P = seg.shape[2] * seg.shape[3]
    t = relabel(seg, perm)
    votes = np.zeros((B, K, P), np.int64)
    for j in range(K):
        votes[:, j] = (t == j).sum(0)
    top = np.zeros((B, P), np.int64)
    cons = np.zeros((B, P), np.uint8)
    for j in range(K):                                       # `v > best` from 0 upwards from a best of 0
        win = votes[:, j] > top
        top = np.where(win, votes[:, j], top)
        cons = np.where(win, j, cons).astype(np.uint8)
    out = dict(votes=votes, consensus=cons, agreement=top.astype(np.float32) / np.float32(C), relabelled=t)
    if ref is not None:
        match = np.zeros((C, B), np.float32)
        for b in range(B):
            r = int(ref[b])
            if 0 <= r < C:
                for c in range(C):
                    match[c, b] = np.float32(float(((t[c, b] >= 0) & (t[c, b] == t[r, b])).sum()) / float(P))
        out['match'] = match
    if mask is not None:
        m = np.asarray(mask, np.float64).reshape(C, B, K, P)
        mm = np.zeros((B, K, P))
        for c in range(C):
            for b in range(B):
                for i in range(K):
                    j = int(perm[c, b, i])
                    if 0 <= j < K:
                        mm[b, j] += m[c, b, i]
        out['mask_mean'] = mm / C
    return out
