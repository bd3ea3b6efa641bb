"""Time of ``IODINE.reconstruct_adaptive`` against the fixed ``reconstruct``, HIP events after warm-up.

    python tools/adaptive_time.py [--reps 9] [--warmup 3] [--out FILE.json] [--md FILE.md] [--only NAME] [--trace-c]

Configurations, in one process: the dSprites architecture at B = 32 (K = 6) and the CLEVR architecture at B = 8 and B = 32 (K = 7), each
with max_iters in {5, 10}; synthetic weights, uniform images, fixed noise (the time depends on none of them - the budget decides who stops).
Timed, each call as one window between two events on the current stream (the adaptive call ends in work the second event waits for), the
routes alternating sample by sample, the figure the median of ``reps`` samples with the min .. max spread beside it:

* (a) *fixed*: ``reconstruct(x, eps)`` at ``n_iters = max_iters`` - the yardstick, whose path this feature does not touch;
* (b) *adaptive, nothing stops*: ``tol = -inf`` at ``check_every = 1`` and at ``check_every = max_iters`` - the pure overhead of the rounds
  (per round: one select launch, one 8-byte read-back with a stream synchronise, no move while nothing has stopped);
* (c) *adaptive, half the batch on a budget of 2*: ``budget = 2`` for the even images, ``max_iters`` for the odd ones, ``check_every = 1``;
  its ideal share of (a)'s loop is ``sum(iters) / (B max_iters)``.

``--trace-c`` runs (c) of one configuration (``--only``, default the first) a few times and nothing else: the window for a kernel trace taken
from outside (``rocprofv3 --kernel-trace --stats -- python tools/adaptive_time.py --trace-c``), no counters in that run."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE                                           # noqa: E402
from iodine_amd.model import clevr6_arch, dsprites_arch                 # noqa: E402

CONFIGS = (('dsprites_b32', dsprites_arch, 6, 32), ('clevr_b8', clevr6_arch, 7, 8), ('clevr_b32', clevr6_arch, 7, 32))
MAX_ITERS = (5, 10)
INF = float('inf')


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def routes(model, x, eps, M, dev):
    B = x.shape[0]
    budget = torch.where(torch.arange(B, device=dev) % 2 == 0, 2, M).to(torch.int32)

    def fixed():
        model.n_iters = M
        return model.reconstruct(x, eps)
    return budget, {
        'fixed': fixed,
        'never_r1': lambda: model.reconstruct_adaptive(x, tol=-INF, max_iters=M, check_every=1, eps=eps),
        'never_rmax': lambda: model.reconstruct_adaptive(x, tol=-INF, max_iters=M, check_every=M, eps=eps),
        'half_budget2': lambda: model.reconstruct_adaptive(x, max_iters=M, budget=budget, check_every=1, eps=eps),
    }


def setup(make_arch, K, B, M, dev):
    arch = make_arch()
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    model.K = K
    L, S = int(arch.DIM_LATENT), int(arch.IMG_SIZE)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    eps = torch.randn(M + 1, B, K, L, generator=g).to(dev)
    return model, x, eps


def measure(name, make_arch, K, B, M, reps, warmup, dev):
    model, x, eps = setup(make_arch, K, B, M, dev)
    budget, runs = routes(model, x, eps, M, dev)
    # what is timed computes what it should: nothing stopping is the fixed call, bit for bit; the budget is met
    pred = runs['fixed']()[0]
    same = all(bool(torch.equal(runs[k]().pred, pred)) for k in ('never_r1', 'never_rmax'))
    res = runs['half_budget2']()
    iters = res.iters.tolist()
    times = {k: [] for k in runs}
    for r in range(warmup + reps):
        for k, fn in runs.items():
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {k + '_ms_median': round(med(v), 4) for k, v in times.items()}
    out.update({k + '_ms_min': round(min(v), 4) for k, v in times.items()})
    out.update({k + '_ms_max': round(max(v), 4) for k, v in times.items()})
    a = med(times['fixed'])
    out.update(config=name, K=K, B=B, max_iters=M, never_equals_fixed=same, budget_iters_ok=iters == budget.tolist(), active=res.active,
               fixed_spread_rel=round((max(times['fixed']) - min(times['fixed'])) / a, 4),
               never_r1_over_fixed=round(med(times['never_r1']) / a, 4), never_rmax_over_fixed=round(med(times['never_rmax']) / a, 4),
               half_over_fixed=round(med(times['half_budget2']) / a, 4), half_ideal=round(sum(iters) / float(B * M), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', help='one configuration by name')
    ap.add_argument('--trace-c', action='store_true', help='run (c) of one configuration at max_iters 10 five times and nothing else')
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('adaptive_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    configs = [c for c in CONFIGS if args.only in (None, c[0])]
    if not configs:
        raise SystemExit(f'--only: one of {[c[0] for c in CONFIGS]}')
    if args.trace_c:
        name, make_arch, K, B = configs[0]
        model, x, eps = setup(make_arch, K, B, 10, dev)
        run = routes(model, x, eps, 10, dev)[1]['half_budget2']
        for _ in range(5):
            res = run()
        torch.cuda.synchronize()
        print(json.dumps(dict(config=name, B=B, max_iters=10, calls=5, active=res.active)))
        return
    rows = [measure(n, a, K, B, M, args.reps, args.warmup, dev) for n, a, K, B in configs for M in MAX_ITERS]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        cell = lambda r, k: '{:.2f} ({:.2f} .. {:.2f})'.format(r[k + '_ms_median'], r[k + '_ms_min'], r[k + '_ms_max'])
        with open(args.md, 'w') as f:
            f.write('| config | B | max_iters | (a) fixed ms | (b) never, R = 1 ms | (b) never, R = max ms | (b) / (a), R = 1 | (b) / (a), R = max | '
                    '(c) half at budget 2 ms | (c) / (a) | ideal |\n|---|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| {} | {} | {} | {} | {} | {} | {:.4f} | {:.4f} | {} | {:.4f} | {:.4f} |\n'.format(
                    r['config'], r['B'], r['max_iters'], cell(r, 'fixed'), cell(r, 'never_r1'), cell(r, 'never_rmax'), r['never_r1_over_fixed'],
                    r['never_rmax_over_fixed'], cell(r, 'half_budget2'), r['half_over_fixed'], r['half_ideal']))


if __name__ == '__main__':
    main()
