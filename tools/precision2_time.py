"""Time of ``reconstruct`` and of a training step at conv_precision 2 against conv_precision 1 of the same build, HIP events after warm-up.

    python tools/precision2_time.py [--reps 7] [--warmup 2] [--commit ID] [--out FILE.json] [--md FILE.md]

Two configurations: cfg3 (the CLEVR architecture, K = 7, B = 32) and cfg2 (the dSprites architecture, K = 6, B = 32); synthetic weights and
images (the time depends on neither).  One module per precision, both alive in one process; a sample of the timing is one whole call
between two events, the two precisions alternate sample by sample, and the figure is the median of ``reps`` samples with their minimum
and maximum beside it (the spread).  A separate pass under the library's event profiler (option profile 1: the ``conv_tile_*`` launches
only; after the timed loops, since the brackets idle the GPU) gives the time per ``conv_tile_fwd`` / ``conv_tile_dgrad`` launch of a
``reconstruct``, again alternating and once per repeat.  The verdict lines say whether precision 2 beats precision 1 by more than the
spread (max - min) of precision 1's own repeats: per launch of either category and per ``reconstruct``."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE                                           # noqa: E402
from iodine_amd.model import clevr6_arch, dsprites_arch                 # noqa: E402

CONFIGS = (('cfg3', clevr6_arch, 7, 32), ('cfg2', dsprites_arch, 6, 32))
PRECISIONS = (1, 2)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    s = sorted(v)
    return dict(median=round(s[len(s) // 2], 5), min=round(s[0], 5), max=round(s[-1], 5))


def measure(name, make_arch, K, B, reps, warmup, dev):
    arch = make_arch()
    models = {}
    for p in PRECISIONS:
        torch.manual_seed(0)
        m = IODINE(arch).to(dev)
        m.K = K
        m.set_option('conv_precision', p)
        models[p] = m
    Si = int(arch.IMG_SIZE)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, 3, Si, Si, generator=g).to(dev)

    def reconstruct(m):
        m.eval()
        with torch.no_grad():
            m.reconstruct(x)

    def train_step(m):
        m.train()
        m.zero_grad(set_to_none=True)
        m(x).backward()

    out = dict(config=name, K=K, B=B, S=Si, T=int(arch.ITERS))
    for what, fn in (('reconstruct', reconstruct), ('train_step', train_step)):
        times = {p: [] for p in PRECISIONS}
        for r in range(warmup + reps):
            for p in PRECISIONS:
                t = timed(lambda: fn(models[p]))
                if r >= warmup:
                    times[p].append(t)
        for p in PRECISIONS:
            out[f'{what}_ms_p{p}'] = stats(times[p])
        torch.cuda.synchronize()
    # per launch of the weight-stationary kernel, in a pass of its own
    per = {(p, c): [] for p in PRECISIONS for c in ('conv_tile_fwd', 'conv_tile_dgrad')}
    for p in PRECISIONS:
        models[p].set_option('profile', 1)
        reconstruct(models[p])
        for c in ('conv_tile_fwd', 'conv_tile_dgrad'):
            models[p].profile_read(c)
    for r in range(reps):
        for p in PRECISIONS:
            reconstruct(models[p])
            for c in ('conv_tile_fwd', 'conv_tile_dgrad'):
                ms, n = models[p].profile_read(c)
                per[(p, c)].append(ms / max(n, 1))
                out[f'{c}_launches_per_reconstruct'] = n
    for p in PRECISIONS:
        models[p].set_option('profile', 0)
    for (p, c), v in per.items():
        out[f'{c}_ms_per_launch_p{p}'] = stats(v)
    verdict = {}
    for key in ('conv_tile_fwd_ms_per_launch', 'conv_tile_dgrad_ms_per_launch', 'reconstruct_ms', 'train_step_ms'):
        a, b = out[key + '_p1'], out[key + '_p2']
        verdict[key] = dict(gain=round(a['median'] - b['median'], 5), spread_p1=round(a['max'] - a['min'], 5), ratio=round(a['median'] / b['median'], 3),
                            beats_spread=bool(a['median'] - b['median'] > a['max'] - a['min']))
    out['verdict'] = verdict
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('precision2_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = [measure(n, a, K, B, args.reps, args.warmup, dev) for n, a, K, B in CONFIGS]
    out = dict(device=torch.cuda.get_device_name(0), commit=args.commit, reps=args.reps, warmup=args.warmup, rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        fmt = lambda s: '{:.4f} ({:.4f} .. {:.4f})'.format(s['median'], s['min'], s['max'])
        with open(args.md, 'w') as f:
            f.write(f'Device: {out["device"]}; source: {args.commit}; median (min .. max) of {args.reps} alternating repeats after {args.warmup} warm-up rounds, ms.\n\n')
            f.write('| config | quantity | conv_precision 1 | conv_precision 2 | 1 / 2 | gain > spread of 1 |\n|---|---|---|---|---|---|\n')
            for r in rows:
                for key, label in (('reconstruct_ms', 'reconstruct'), ('train_step_ms', 'training step'),
                                   ('conv_tile_fwd_ms_per_launch', 'conv_tile_fwd per launch'), ('conv_tile_dgrad_ms_per_launch', 'conv_tile_dgrad per launch')):
                    v = r['verdict'][key]
                    f.write('| {} (B {}, K {}) | {} | {} | {} | {:.3f} | {} |\n'.format(r['config'], r['B'], r['K'], label, fmt(r[key + '_p1']), fmt(r[key + '_p2']),
                                                                                      v['ratio'], 'yes' if v['beats_spread'] else 'NO'))


if __name__ == '__main__':
    main()
