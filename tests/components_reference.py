"""Numpy restatement of ``iodine_seg_components`` (include/iodine_hip.h) and the pattern list its tests run, shared by
test_components_cpu.py and test_gpu_components.py.  ``partition`` is a breadth-first flood fill from every unvisited valid pixel in raster
order - obviously the rule, not fast -; everything after it is array arithmetic on its result.  Results are cached and must not be
written to."""
import functools
from collections import deque

import numpy as np

INVALID = 255
N4 = ((0, -1), (0, 1), (-1, 0), (1, 0))                 # (d_row, d_col)
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def partition(seg, slots, connectivity):
    """seg (S, S) uint8 -> comp (S, S) int32 (index of the pixel's component in order of first(c), -1 where seg >= slots),
    first (C,), area (C,), slot (C,)"""
    S = seg.shape[0]
    W = S + 2                                            # a frame of INVALID pixels stands in for the bounds checks (slots <= 16 < INVALID)
    assert slots <= INVALID
    flat = np.pad(np.asarray(seg, np.uint8), 1, constant_values=INVALID).reshape(-1).tolist()
    comp = [-1] * (W * W)
    first, area, slot = [], [], []
    steps = [dr * W + dc for dr, dc in (N4 if connectivity == 4 else N8)]
    for r0 in range(S):
        for c0 in range(S):
            p0 = (r0 + 1) * W + c0 + 1
            v = flat[p0]
            if v >= slots or comp[p0] >= 0:
                continue
            c = len(first)
            comp[p0] = c
            todo, n = deque([p0]), 0
            while todo:
                q = todo.popleft()
                n += 1
                for step in steps:
                    r = q + step
                    if flat[r] == v and comp[r] < 0:
                        comp[r] = c
                        todo.append(r)
            first.append(r0 * S + c0)
            area.append(n)
            slot.append(v)
    comp = np.array(comp, np.int32).reshape(W, W)[1:-1, 1:-1]
    return np.ascontiguousarray(comp), np.array(first, np.int64), np.array(area, np.int64), np.array(slot, np.int64)


def components(seg, slots, connectivity=4, min_area=1, max_components=64, parts=None):
    """One map (S, S) uint8 -> dict(labels, area_map (S, S) int32, count (4,), per_slot (slots, 4), table (M, 8) int32, clean (S, S)
    uint8), every output of the entry point for one image.  ``parts``: ``partition(seg, slots, connectivity)`` where the caller has it."""
    seg = np.asarray(seg, np.uint8)
    S, M = seg.shape[0], max_components
    comp, first, area, slot = parts if parts is not None else partition(seg, slots, connectivity)
    C = len(first)
    valid = comp >= 0
    kept = area >= min_area
    ident = np.where(kept, np.cumsum(kept) - 1, -1)                       # in order of first(c) by construction of partition
    cc = np.where(valid, comp, 0)
    labels = np.where(valid, ident[cc] if C else -1, -1).astype(np.int32)
    area_map = np.where(valid, area[cc] if C else 0, 0).astype(np.int32)
    count = np.array([kept.sum(), (~kept).sum(), area[~kept].sum(), (~valid).sum()], np.int32)
    per_slot = np.zeros((slots, 4), np.int32)
    for s in range(slots):
        mine = slot == s
        per_slot[s] = [(mine & kept).sum(), (mine & ~kept).sum(), area[mine].max() if mine.any() else 0, area[mine & ~kept].sum()]
    table = np.full((M, 8), -1, np.int32)
    row, col = np.divmod(np.arange(S * S), S)
    flat = labels.reshape(-1)
    for i in range(min(M, int(kept.sum()))):
        at = flat == i
        c = int(np.flatnonzero(ident == i)[0])
        table[i] = [slot[c], area[c], col[at].sum(), row[at].sum(), col[at].min(), row[at].min(), col[at].max(), row[at].max()]
    # clean: every (small c, kept d) pair across a 4-neighbour edge; per c the largest area(d), then the smallest first(d)
    clean = seg.copy()
    pairs = []
    for a, b in ((comp[:, :-1], comp[:, 1:]), (comp[:-1, :], comp[1:, :])):
        for c, d in ((a, b), (b, a)):
            c, d = c.reshape(-1), d.reshape(-1)
            ok = (c >= 0) & (d >= 0)
            ok[ok] = ~kept[c[ok]] & kept[d[ok]]
            pairs.append(np.stack([c[ok], d[ok]], 1))
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    if len(pairs):
        order = np.lexsort((first[pairs[:, 1]], -area[pairs[:, 1]], pairs[:, 0]))
        pairs = pairs[order]
        lead = np.ones(len(pairs), bool)
        lead[1:] = pairs[1:, 0] != pairs[:-1, 0]
        take = np.full(C, -1, np.int64)
        take[pairs[lead, 0]] = slot[pairs[lead, 1]]
        moved = valid & (take[cc] >= 0)
        clean[moved] = take[cc][moved].astype(np.uint8)
    return dict(labels=labels, area_map=area_map, count=count, per_slot=per_slot, table=table, clean=clean)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The pattern list: name -> f(S) -> (S, S) uint8 with values below 16 (or INVALID).  TILE is the tile edge of the global-memory form.
# ---------------------------------------------------------------------------------------------------------------------------------------
TILE = 64


def _one_label(S):
    return np.full((S, S), 3, np.uint8)


def _checkerboard(S):
    r, c = np.indices((S, S))
    return ((r + c) & 1).astype(np.uint8)


def _serpentine(S):
    """a one-pixel-wide path of label 1 through the whole image: full even rows, joined alternately at the right and left end"""
    m = np.zeros((S, S), np.uint8)
    m[0::2] = 1
    m[1::4, S - 1] = 1
    m[3::4, 0] = 1
    return m


def _rings(S):
    r, c = np.indices((S, S))
    return (np.minimum(np.minimum(r, c), np.minimum(S - 1 - r, S - 1 - c)) % 3).astype(np.uint8)


def _corner_blocks(S):
    """two blocks of label 1 that touch at one corner only: one component under 8, two under 4"""
    m = np.zeros((S, S), np.uint8)
    h = S // 2
    m[:h, :h] = 1
    m[h:, h:] = 1
    return m


def _tile_crosser(S):
    """label 2: one column and one row through every tile of the global form plus a staircase diagonal, so one component crosses every
    tile border (the diagonal alone joins corner to corner under 8); label 5 elsewhere, cut into many pieces"""
    m = np.full((S, S), 5, np.uint8)
    m[:, TILE // 2::TILE] = 2
    m[TILE // 2::TILE, :] = 2
    i = np.arange(S)
    m[i, i] = 2
    return m


def _random16(S, seed=5):
    return np.random.default_rng(seed + S).integers(0, 16, (S, S)).astype(np.uint8)


def _random16_invalid(S):
    m = _random16(S)
    m[np.random.default_rng(77 + S).random((S, S)) < 0.1] = INVALID
    return m


def _specks(S):
    """two large regions (labels 0 and 1) with single pixels and 2 x 2 specks of other labels.  From S = 16 up also TIE_SPECK: one pixel
    whose only kept 4-neighbours at min_area 2 and 9 are two 3 x 3 blocks of area 9 (its other two neighbours are single pixels), so the
    tie rule decides - the upper block, label 10 -, and a pixel enclosed by a ring of area 8, which stays as it is at min_area 9"""
    m = np.zeros((S, S), np.uint8)
    if S >= 16:
        m[:, S // 2:] = 1
        m[2, S // 2 - 1] = 7                               # single pixel on the border of the two regions
        m[5:7, 3:5] = 4                                    # 2 x 2 speck inside label 0
        m[9:12, 2:5] = 6                                   # 3 x 3 ring of label 6 (area 8) ...
        m[10, 3] = 9                                       # ... enclosing one pixel: no kept 4-neighbour at min_area 9
        m[12, S - 2] = 3
        c = S - 5
        m[1:4, c:c + 3] = 10
        m[5:8, c:c + 3] = 11
        m[4, c:c + 3] = (13, 12, 14)                       # TIE_SPECK is the 12
    else:
        m[S // 2, S // 2] = 2
        if S >= 3:
            m[0, S - 1] = 1
    return m


PATTERNS = {
    'one_label': _one_label, 'checkerboard': _checkerboard, 'serpentine': _serpentine, 'rings': _rings, 'corner_blocks': _corner_blocks,
    'tile_crosser': _tile_crosser, 'random16': _random16, 'random16_invalid': _random16_invalid, 'specks': _specks,
}
SLOTS = 16


@functools.lru_cache(maxsize=None)
def pattern(name, S):
    m = PATTERNS[name](S)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _partition_cached(name, S, connectivity):
    return partition(pattern(name, S), SLOTS, connectivity)


@functools.lru_cache(maxsize=None)
def expected(name, S, connectivity, min_area, max_components):
    """``components`` of ``pattern(name, S)`` at SLOTS slots (cached: read only)"""
    out = components(pattern(name, S), SLOTS, connectivity, min_area, max_components, _partition_cached(name, S, connectivity))
    for v in out.values():
        v.setflags(write=False)
    return out
