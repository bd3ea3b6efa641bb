"""Time of one decomposition sheet (``iodine_amd.figures.sheet``, one launch of ``iodine_render_sheet``) against the same sheet composed
from torch ops on the same device, and against the device-to-host copy of the float planes the sheet replaces.  HIP events after warm-up.

    python tools/sheet_time.py [--reps 50] [--inner 20] [--warmup 5] [--copies 4] [--out FILE.json] [--md FILE.md] [--commit HASH]

An 8-scene sheet with the default panels (image, pred, seg, K slot panels), and with the error panel behind them (an odd panel count makes
the width a multiple of 4 at pad 2: the word-store form of the kernel), at the CLEVR shapes (K = 7, S = 128, scale 1 and 2) and at the
dSprites shapes (K = 4, S = 64, scale 1 and 2).  One sample is the time of ``inner`` back-to-back calls between two events divided by
``inner``; the contenders alternate sample by sample in one process and the figure is the median of ``reps`` samples.  Every call reads one
of ``copies`` distinct input sets in turn.  The composite - argmax, palette gather, the slot blend, ``repeat_interleave``, ``cat`` and the
quantisation - is checked against the op before anything is timed.  ``op`` is ``figures.sheet`` as a user calls it, ``launch`` one
``iodine_render_sheet`` call on a spec prepared beforehand: the difference is Python per call.  ``planes d2h`` is the copy of mask, mean, pred and x
into pinned host memory: what a user pays before the first line of numpy when the figure is made on the host; ``sheet d2h`` the copy of
the finished sheet.  Prints one JSON line; ``--md`` also writes the table kept as profiles/sheet_timing.md with the achieved fraction of
8 TB/s on the algorithmic bytes: the planes the default panels read (mask K times for seg and once per slot, mean once per slot, x, pred:
``4 (5 K + 6) S^2`` per row) plus the sheet's ``3 H W``."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import figures                                        # noqa: E402

SHAPES = ((8, 7, 128, 1), (8, 7, 128, 2), (8, 4, 64, 1), (8, 4, 64, 2))   # (rows, K, S, scale)
DEFAULT = ('image', 'pred', 'seg', 'slots')
WIDE = DEFAULT + ('error',)                                            # an odd panel count: W % 4 == 0 at pad 2, the word-store form
PEAK_BPS = 8e12
PAD = 2


def _q(v):
    v = torch.where(v > 0, torch.where(v < 1, v, torch.ones_like(v)), torch.zeros_like(v))
    return (v * 255.0 + 0.5).to(torch.int32).to(torch.uint8)


def eager_sheet(mask, mean, pred, x, scale, pal, error=False):
    """the default sheet (``error``: with the error panel behind it) with torch ops: (H, W, 3) uint8"""
    Rr, K, _, S, _ = mask.shape
    m = mask[:, :, 0]
    seg = pal[m.argmax(1)]                                             # (R, S, S, 3)
    hwc = lambda t: _q(t).permute(0, 2, 3, 1)
    panels = [hwc(x), hwc(pred), seg]
    blend = mask * mean + (1.0 - mask) * 1.0                           # (R, K, 3, S, S), background 1
    panels += [hwc(blend[:, k]) for k in range(K)]
    if error:
        d = (x - pred).abs()
        e = _q(4.0 * ((d[:, 0] + d[:, 1]) + d[:, 2]) / 3.0)
        panels.append(torch.stack([e, e, e], -1))
    if scale > 1:
        panels = [p.repeat_interleave(scale, 1).repeat_interleave(scale, 2) for p in panels]
    side = S * scale
    white = lambda h, w: torch.full((Rr, h, w, 3), 255, dtype=torch.uint8, device=mask.device)
    cols = [white(side, PAD)]
    for p in panels:
        cols += [p, white(side, PAD)]
    rows = torch.cat(cols, 2)                                          # (R, side, W, 3)
    W = rows.shape[2]
    rows = torch.cat([rows, white(PAD, W)], 1)                         # every row with the padding below it
    return torch.cat([white(PAD, W)[0], rows.reshape(-1, W, 3)], 0)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(Rr, K, S, scale, copies, reps, inner, warmup, dev, panels=DEFAULT):
    g = torch.Generator().manual_seed(7)
    pal = torch.tensor(figures.PALETTE, dtype=torch.uint8, device=dev)
    sets = []
    for _ in range(copies):
        mask = torch.softmax(4.0 * torch.randn(Rr, K, 1, S, S, generator=g), dim=1).to(dev)
        mean = torch.sigmoid(torch.randn(Rr, K, 3, S, S, generator=g)).to(dev)
        pred, x = torch.rand(Rr, 3, S, S, generator=g).to(dev), torch.rand(Rr, 3, S, S, generator=g).to(dev)
        sets.append((mask, mean, pred, x))
    op = lambda i: figures.sheet(*sets[i % copies], panels=panels, scale=scale, pad=PAD)
    eager = lambda i: eager_sheet(*sets[i % copies], scale, pal, error=panels is WIDE)
    a, b = op(0), eager(0)
    # the launch alone: spec and tensors prepared once per input set, one ctypes call per sample element, the same output buffer
    prepared = [figures._prepare(m, mu, p, xx, None, panels, 'masked', scale, PAD, (255, 255, 255), (1., 1., 1.), 0.5, True, (255, 255, 255),
                                 4.0, None, None)[:2] for m, mu, p, xx in sets]
    buf = torch.empty_like(a)
    launch = lambda i: figures.render_into(buf, *prepared[i % copies])
    assert torch.equal(launch(0), a)
    form = figures.sheet_form(buf, *prepared[0])
    # torch may contract m * mu + (1 - m) into a fused multiply-add inside one of its kernels; the op never does.  Count, do not assume.
    differ = int((a != b).sum())
    assert a.shape == b.shape and differ <= a.numel() // 1000 and int((a.int() - b.int()).abs().max()) <= 1, 'composite and op disagree'
    host = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in sets[0]]
    host_sheet = torch.empty(a.shape, dtype=torch.uint8).pin_memory()

    def planes_d2h(i):
        for h, t in zip(host, sets[i % copies]):
            h.copy_(t, non_blocking=True)

    runs = {'op': op, 'launch': launch, 'eager': eager, 'planes_d2h': planes_d2h, 'sheet_d2h': lambda i: host_sheet.copy_(a, non_blocking=True)}
    times = {k: [] for k in runs}
    for r in range(warmup + reps):
        for k, fn in runs.items():
            t = timed(fn, inner)
            if r >= warmup:
                times[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    H, W = int(a.shape[0]), int(a.shape[1])
    nbytes = 4 * (5 * K + 6 + (6 if panels is WIDE else 0)) * S * S * Rr + 3 * H * W
    out = {k + '_ms_median': round(med(v), 5) for k, v in times.items()}
    out.update({k + '_ms_min': round(min(v), 5) for k, v in times.items()})
    out.update({k + '_ms_max': round(max(v), 5) for k, v in times.items()})
    out.update(shape=[Rr, K, S, scale], sheet=[H, W], panels=len(figures.expand_panels(panels, K)), form=form, copies=copies, algorithmic_bytes=nbytes, bytes_differing_from_eager=differ,
               plane_bytes=sum(t.numel() * 4 for t in sets[0]), sheet_bytes=3 * H * W,
               eager_over_op=round(med(times['eager']) / med(times['op']), 2),
               op_fraction_of_8TBps=round(nbytes / (med(times['op']) * 1e-3) / PEAK_BPS, 4),
               launch_fraction_of_8TBps=round(nbytes / (med(times['launch']) * 1e-3) / PEAK_BPS, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--copies', type=int, default=4)
    ap.add_argument('--out')
    ap.add_argument('--md')
    ap.add_argument('--commit', default='(working tree)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sheet_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = [measure(*s, args.copies, args.reps, args.inner, args.warmup, dev, panels=p) for s in SHAPES for p in (DEFAULT, WIDE)]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, inner=args.inner, warmup=args.warmup, commit=args.commit, rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        with open(args.md, 'w') as f:
            f.write('# Decomposition sheet: one launch against the torch composite and against copying the planes\n\n')
            f.write(f'`python tools/sheet_time.py --reps {args.reps} --inner {args.inner} --warmup {args.warmup} --copies {args.copies}` on '
                    f'{out["device"]}, tree {args.commit}.  ms per call: median (min .. max) of {args.reps} samples of {args.inner} back-to-back '
                    'calls, HIP events, the contenders alternating.  Default panels (image, pred, seg, K slots), or those and the error panel - an odd '
                    'panel count, whose width is a multiple of 4: the word-store form -, 8 rows, pad 2.  "op" is `figures.sheet`, "launch" one '
                    '`iodine_render_sheet` call on a spec prepared beforehand; form: bit 0 = 16-byte loads, bit 1 = word stores.  "planes d2h" '
                    'copies mask, mean, pred and x to pinned host memory, "sheet d2h" the finished sheet.  The fraction is algorithmic bytes '
                    '(4 (5 K + 6) S^2 per row read, 24 S^2 more with the error panel, 3 H W written) over the median time over 8 TB/s.\n\n')
            f.write('| (R, K, S, scale) | panels | form | sheet H x W | op ms | launch ms | torch composite ms | composite / op | planes d2h ms | sheet d2h ms | '
                    'plane MB | sheet MB | op fraction of 8 TB/s | launch fraction |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| ({}, {}, {}, {}) | {} | {} | {} x {} | {:.4f} ({:.4f} .. {:.4f}) | {:.4f} ({:.4f} .. {:.4f}) | {:.4f} ({:.4f} .. {:.4f}) | {:.1f} | {:.4f} | {:.4f} | '
                        '{:.2f} | {:.2f} | {:.4f} | {:.4f} |\n'.format(
                    *r['shape'], r['panels'], r['form'], *r['sheet'], r['op_ms_median'], r['op_ms_min'], r['op_ms_max'], r['launch_ms_median'],
                    r['launch_ms_min'], r['launch_ms_max'], r['eager_ms_median'], r['eager_ms_min'], r['eager_ms_max'], r['eager_over_op'],
                    r['planes_d2h_ms_median'], r['sheet_d2h_ms_median'], r['plane_bytes'] / 1e6, r['sheet_bytes'] / 1e6, r['op_fraction_of_8TBps'],
                    r['launch_fraction_of_8TBps']))


if __name__ == '__main__':
    main()
