"""Time of ``iodine_amd.objects.slot_table`` (table + segmentation map, one launch) against the same table computed with eager torch ops on
the same device, HIP events after warm-up.

    python tools/slot_table_time.py [--reps 50] [--inner 20] [--warmup 5] [--copies 6] [--out FILE.json] [--md FILE.md]

Shapes (B, K, S) = (32, 7, 128) - the benchmarked CLEVR config - and (32, 6, 64).  One sample is the time of ``inner`` back-to-back calls
between two events divided by ``inner`` (a single call is a few tens of microseconds: launch gaps are part of what a user pays, the event
resolution is not); the two contenders alternate sample by sample in one process, the figure is the median of ``reps`` samples.  Every
call reads one of ``copies`` distinct input sets in turn: with 6 sets of 59 MB the inputs of a call were last touched more than one 256 MB
Infinity Cache ago ("cold"); ``hot`` is the same with a single set, which stays cache resident.  The eager composite is the yardstick:
argmax, one_hot and a dozen reductions, checked against the op's table before anything is timed.  Prints one JSON line; ``--md`` also
writes the table kept as profiles/slot_table_timing.md, with the achieved fraction of 8 TB/s on the algorithmic bytes (16 B K P in,
56 B K + B P out)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd.objects import slot_table                              # noqa: E402

SHAPES = ((32, 7, 128), (32, 6, 64))
PEAK_BPS = 8e12


def eager_table(mask, mean):
    """the table and map of iodine_slot_table with torch ops (float32 on the device)"""
    B, K, _, S, _ = mask.shape
    m = mask[:, :, 0]
    seg = m.argmax(1)
    hard = torch.nn.functional.one_hot(seg, K).permute(0, 3, 1, 2)
    col = torch.arange(S, device=m.device, dtype=torch.float32).view(1, 1, 1, S)
    row = torch.arange(S, device=m.device, dtype=torch.float32).view(1, 1, S, 1)
    area = m.sum((-1, -2))
    safe = area.clamp_min(1e-30)
    harea = hard.sum((-1, -2)).to(torch.float32)
    hsafe = harea.clamp_min(1.0)
    hf = hard.to(torch.float32)
    some = harea > 0
    neg = torch.full_like(harea, -1.0)
    hb = hard.bool()
    big, small = torch.full_like(m, float(S)), torch.full_like(m, -1.0)
    cols = [area, harea, (m * col).sum((-1, -2)) / safe, (m * row).sum((-1, -2)) / safe,
            torch.where(some, (hf * col).sum((-1, -2)) / hsafe, neg), torch.where(some, (hf * row).sum((-1, -2)) / hsafe, neg),
            torch.where(some, torch.where(hb, col, big).amin((-1, -2)), neg), torch.where(some, torch.where(hb, row, big).amin((-1, -2)), neg),
            torch.where(some, torch.where(hb, col, small).amax((-1, -2)), neg), torch.where(some, torch.where(hb, row, small).amax((-1, -2)), neg)]
    rgb = (m[:, :, None] * mean).sum((-1, -2)) / safe[..., None]
    cols += [rgb[..., 0], rgb[..., 1], rgb[..., 2], m.amax((-1, -2))]
    return torch.stack(cols, -1), seg.to(torch.uint8)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(B, K, S, copies, reps, inner, warmup, dev):
    g = torch.Generator().manual_seed(7)
    sets = []
    for _ in range(copies):
        mask = torch.softmax(4.0 * torch.randn(B, K, 1, S, S, generator=g), dim=1).to(dev)
        mean = torch.sigmoid(torch.randn(B, K, 3, S, S, generator=g)).to(dev)
        sets.append((mask, mean))
    # the yardstick computes the same thing
    t_op, s_op = slot_table(*sets[0], segmentation=True)
    t_eg, s_eg = eager_table(*sets[0])
    assert torch.equal(s_op, s_eg), 'segmentation maps differ'
    rel = float(((t_op - t_eg).abs() / t_eg.abs().clamp_min(1e-6)).max())
    assert rel < 1e-3, f'eager composite and op disagree: {rel}'
    runs = {'op': lambda i: slot_table(*sets[i % copies], segmentation=True), 'eager': lambda i: eager_table(*sets[i % copies])}
    times = {k: [] for k in runs}
    for r in range(warmup + reps):
        for k, fn in runs.items():
            t = timed(fn, inner)
            if r >= warmup:
                times[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    P = S * S
    nbytes = 16 * B * K * P + 56 * B * K + B * P
    out = {k + '_ms_median': round(med(v), 5) for k, v in times.items()}
    out.update({k + '_ms_min': round(min(v), 5) for k, v in times.items()})
    out.update({k + '_ms_max': round(max(v), 5) for k, v in times.items()})
    out.update(shape=[B, K, S], copies=copies, algorithmic_bytes=nbytes, max_rel_diff_vs_eager=rel,
               speedup_median=round(med(times['eager']) / med(times['op']), 2),
               op_fraction_of_8TBps=round(nbytes / (med(times['op']) * 1e-3) / PEAK_BPS, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--copies', type=int, default=6)
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('slot_table_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = []
    for B, K, S in SHAPES:
        for label, copies in (('cold', args.copies), ('hot', 1)):
            r = measure(B, K, S, copies, args.reps, args.inner, args.warmup, dev)
            r['inputs'] = label
            rows.append(r)
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, inner=args.inner, warmup=args.warmup, rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        with open(args.md, 'w') as f:
            f.write('# slot_table: one launch against the eager torch composite\n\n')
            f.write(f'`python tools/slot_table_time.py --reps {args.reps} --inner {args.inner} --warmup {args.warmup} --copies {args.copies}` on '
                    f'{out["device"]}.  ms per call: median (min .. max) of {args.reps} samples of {args.inner} back-to-back calls, HIP events, the two '
                    'contenders alternating; "cold" rotates over input sets larger than the Infinity Cache, "hot" re-reads one set.  '
                    'The fraction is algorithmic bytes (16 B K P in, 56 B K + B P out) over the op\'s median time over 8 TB/s.\n\n')
            f.write('| (B, K, S) | inputs | op ms | eager ms | eager / op | algorithmic MB | op fraction of 8 TB/s |\n|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| ({}, {}, {}) | {} | {:.4f} ({:.4f} .. {:.4f}) | {:.4f} ({:.4f} .. {:.4f}) | {:.1f} | {:.2f} | {:.3f} |\n'.format(
                    *r['shape'], r['inputs'], r['op_ms_median'], r['op_ms_min'], r['op_ms_max'], r['eager_ms_median'], r['eager_ms_min'],
                    r['eager_ms_max'], r['speedup_median'], r['algorithmic_bytes'] / 1e6, r['op_fraction_of_8TBps']))


if __name__ == '__main__':
    main()
