"""Time of ``iodine_amd.objects.components`` on the device against the route a user has without it: ``seg.cpu()`` and one
``scipy.ndimage.label`` per slot (where scipy is absent, the flood fill of tests/components_reference.py - the column says which).

    python tools/components_time.py [--reps 30] [--inner 10] [--warmup 3] [--host-reps 5] [--out FILE.json] [--md FILE.md]

Shapes (B, K, S) = (32, 7, 128) - CLEVR's -, (32, 6, 64) and one 1024 x 1024 map with 7 labels.  Two kinds of map: "smooth" is the
ground-truth layout of the synthetic scenes (``resident.synth_scenes``, the topmost object's index per pixel, 0 for the background);
"speckled" is the same with every tenth pixel replaced by a uniform random label - what an argmax map looks like along object borders.

Device columns: HIP events around ``inner`` back-to-back calls, divided by ``inner`` (a call is several short launches and one scratch
allocation from torch's pool: the gaps are part of what a user pays); median (min .. max) of ``reps`` samples after ``warmup`` samples.
"plain" returns labels, count, per_slot and a 64-row table; "full" adds ``area_map`` and ``clean`` at ``min_area`` 9.  Host columns: a host
clock around the whole route starting from the device tensor, so the copy and its synchronise are inside; ``host-reps`` samples.  "host
entry" is ``components`` on the CPU copy (``iodine_seg_components_host``, image by image).  Before anything is timed the device labels are
checked against the host entry's, and against scipy's partition where scipy is there.  Prints one JSON line; ``--md`` also writes the table
kept as profiles/components_timing.md."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iodine_amd.objects import components                              # noqa: E402
from iodine_amd.resident import synth_scenes                           # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

SHAPES = ((32, 7, 128), (32, 6, 64), (1, 7, 1024))
FULL = dict(min_area=9, area_map=True, clean=True)


def make_maps(B, K, S, dev):
    """(smooth, speckled) uint8 (B, S, S) on the device with labels in 0..K-1"""
    _, masks, _ = synth_scenes(B, S, seed=11, kind='blobs', max_objects=K - 1, device=dev)
    words = masks.view(torch.int16).to(torch.int32) & 0xFFFF
    bit = torch.arange(16, device=dev, dtype=torch.int32).view(1, 16, 1, 1)
    top = (((words.unsqueeze(1) >> bit) & 1) * (bit + 1)).amax(1)        # 0: no object; g + 1: the highest mask g that covers the pixel
    smooth = top.clamp_max(K - 1).to(torch.uint8)
    g = torch.Generator(device='cpu').manual_seed(5)
    noise = torch.randint(0, K, (B, S, S), generator=g, dtype=torch.uint8).to(dev)
    hit = (torch.rand((B, S, S), generator=g) < 0.1).to(dev)
    return smooth, torch.where(hit, noise, smooth)


def label_route(seg_dev, K):
    """today's route: copy, then label slot by slot -> list over images of list over slots of (labels, n)"""
    seg = seg_dev.cpu().numpy()
    out = []
    for b in range(seg.shape[0]):
        if ndimage is not None:
            out.append([ndimage.label(seg[b] == k) for k in range(K)])
        else:
            out.append(reference_partition(seg[b], K))
    return out


def reference_partition(seg, K):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import components_reference as R
    return R.partition(seg, K, 4)


def check(seg, K):
    dev_out = components(seg, K)
    host_out = components(seg.cpu(), K)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(dev_out[:4], host_out[:4])), 'device and host entry differ'
    if ndimage is not None:
        lab = dev_out.labels[0].cpu().numpy()
        sg = seg[0].cpu().numpy()
        for k in range(K):
            at = sg == k
            ref, n = ndimage.label(at)
            pairs = np.unique(np.stack([ref[at], lab[at]], 1), axis=0)  # (scipy's number, ours) wherever they meet, sorted by scipy's
            assert len(pairs) == n == len(np.unique(lab[at])), 'partition differs from scipy'
            assert np.all(np.diff(pairs[:, 1]) > 0), 'numbering order differs from scipy'


def device_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def stats(v):
    v = sorted(v)
    return [round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)]


def measure(B, K, S, kind, seg, args):
    check(seg, K)
    dev_runs = {'plain': lambda: components(seg, K), 'full': lambda: components(seg, K, **FULL)}
    times = {k: [] for k in dev_runs}
    for r in range(args.warmup + args.reps):
        for k, fn in dev_runs.items():
            t = device_ms(fn, args.inner)
            if r >= args.warmup:
                times[k].append(t)
    host_runs = {'label_route': lambda: label_route(seg, K), 'host_entry': lambda: components(seg.cpu(), K, **FULL)}
    for k, fn in host_runs.items():
        fn()                                                             # warm-up: imports, allocator, page faults
        times[k] = [host_ms(fn) for _ in range(args.host_reps)]
    row = dict(shape=[B, K, S], map=kind, kept=int(components(seg, K, **FULL).count[:, 0].sum()),
               components=int(components(seg, K).count[:, 0].sum()))
    row.update({k + '_ms': stats(v) for k, v in times.items()})
    row['label_route_over_plain'] = round(row['label_route_ms'][0] / row['plain_ms'][0], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=5)
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('components_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = []
    for B, K, S in SHAPES:
        for kind, seg in zip(('smooth', 'speckled'), make_maps(B, K, S, dev)):
            rows.append(measure(B, K, S, kind, seg, args))
    route = 'scipy.ndimage.label per slot' if ndimage is not None else 'flood fill of tests/components_reference.py (no scipy)'
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, inner=args.inner, warmup=args.warmup, host_reps=args.host_reps,
               label_route=route, rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        cell = lambda v: '{:.4f} ({:.4f} .. {:.4f})'.format(*v)
        with open(args.md, 'w') as f:
            f.write('# components: the device call against copy + label per slot\n\n')
            f.write(f'`python tools/components_time.py --reps {args.reps} --inner {args.inner} --warmup {args.warmup} --host-reps '
                    f'{args.host_reps}` on {out["device"]}.  ms per call, median (min .. max).  Device columns: HIP events around {args.inner} '
                    f'back-to-back calls, {args.reps} samples after {args.warmup} warm-up samples; "plain" = labels, count, per_slot and a 64-row '
                    'table, "full" = plus area_map and clean at min_area 9.  Host columns: host clock around the whole route from the device '
                    f'tensor (copy and synchronise inside), {args.host_reps} samples after one warm-up run; label route = seg.cpu() + {route}, '
                    'host entry = components() on the CPU copy (full).  "components" counts all of the batch at min_area 1, "kept" at 9.\n\n')
            f.write('| (B, K, S) | map | components | kept at 9 | device plain ms | device full ms | label route ms | host entry ms | '
                    'label route / device plain |\n|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| ({}, {}, {}) | {} | {} | {} | {} | {} | {} | {} | {:.1f} |\n'.format(
                    *r['shape'], r['map'], r['components'], r['kept'], cell(r['plain_ms']), cell(r['full_ms']), cell(r['label_route_ms']),
                    cell(r['host_entry_ms']), r['label_route_over_plain']))


if __name__ == '__main__':
    main()
