"""One driver for calls on more images than one library call takes (``IODINE.max_batch``): the images are independent, so the batch
runs as balanced chunks and the per-chunk results are merged by a rule per field.  Sums run left to right, chunk 0 first."""
import torch

# merge rules: concatenate on axis 0 / 1, share-weighted sum, sum of values that carry their share already (``scaled``), chunk 0
CAT0, CAT1, SHARE, SUM, FIRST = 'cat0', 'cat1', 'share', 'sum', 'first'


def split(B, cap):
    """Balanced split of B images into ceil(B / cap) runs, each with its share of the batch: [(start, stop, (stop - start) / B), ...]."""
    n = -(-B // cap)
    base, extra = divmod(B, n)
    out, s = [], 0
    for i in range(n):
        e = s + base + (1 if i < extra else 0)
        out.append((s, e, (e - s) / float(B)))
        s = e
    return out


def cut(t, s, e, axis=0):
    """``t[s:e]`` along ``axis``; None stays None."""
    return None if t is None else t[(slice(None),) * axis + (slice(s, e),)]


def merge(parts, rules, shares=None):
    """Per-chunk tuples or dicts of optional tensors -> one of the same kind, field by field after ``rules`` (same layout).  A field
    that chunk 0 left None stays None; SHARE weighs chunk i by ``shares[i]``."""
    def one(key, rule):
        vals = [p[key] for p in parts]
        if rule == FIRST or vals[0] is None:
            return vals[0]
        if rule == SHARE:
            return sum(v * w for v, w in zip(vals, shares))
        if rule == SUM:
            return sum(vals[1:], vals[0])
        return torch.cat(vals, 0 if rule == CAT0 else 1)
    if isinstance(rules, dict):
        return {k: one(k, r) for k, r in rules.items()}
    return tuple(one(j, r) for j, r in enumerate(rules))


def scaled(w, *ts):
    """The optional tensors ``ts`` times ``w``, a chunk's share of the batch mean as a device scalar - what a SUM rule then adds up."""
    return tuple(None if t is None else t * w for t in ts)
