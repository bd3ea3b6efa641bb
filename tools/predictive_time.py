"""Time of ``IODINE.predictive(x, samples=16)`` against the route that existed before it, HIP events after warm-up.

    python tools/predictive_time.py [--reps 7] [--warmup 2] [--samples 16] [--out FILE.json] [--md FILE.md]

Two configurations: the dSprites architecture at B = 32, K = 6 and the CLEVR architecture at B = 8, K = 7; synthetic weights, a random
posterior with logvar around -1 (the time depends on neither).  *predictive*: one call - per chunk one sampling launch, one decoder pass,
one accumulate launch - plus the float64 host arithmetic of the bounds.  *by hand*: the S samples materialised in torch, ``decode`` on the
(S B, K, L) latents (chunked by ``max_batch()``), ``mean`` / ``var`` / arg-max counts of the NCHW outputs in torch, then S ``elbo`` calls with
``likelihood_maps`` on and the per-image sum of the map - which decodes every sample a second time and writes and re-reads every sample's
planes.  One sample of the timing is one whole route between two events; the two routes alternate sample by sample in one process and the
figure is the median of ``reps`` samples.  Peak memory: ``torch.cuda.max_memory_allocated`` over one run of the route on a fresh module, workspace included.
Before anything is timed the outputs of the two routes are compared (votes: ``torch.argmax`` does not promise the lowest index on an exact
tie, so pixels whose counts differ are reported with and without such a tie).  A separate pass under the library's event profiler (option profile 2,
after the timed loops: the brackets idle the GPU) gives the time of the accumulate launches (category "predictive"); their algorithmic
bytes are S B K P 16 for the decoder output plus, once per launch, the packed image (16 B per pixel) and the state in and out ((2 K + 6)
floats and K ints per pixel each way; the formula holds up to K = 8, where the state stays in registers for the launch)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE                                           # noqa: E402
from iodine_amd.model import clevr6_arch, dsprites_arch                 # noqa: E402

CONFIGS = (('dsprites', dsprites_arch, 6, 32), ('clevr', clevr6_arch, 7, 8))
PEAK_BPS = 8e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated())


def measure(name, make_arch, K, B, S, reps, warmup, dev):
    arch = make_arch()

    def make_model():
        torch.manual_seed(0)
        m = IODINE(arch).to(dev)
        m.K = K
        return m
    model = make_model()
    L, Si = int(arch.DIM_LATENT), int(arch.IMG_SIZE)
    g = torch.Generator().manual_seed(11)
    pm = torch.randn(B, K, L, generator=g).to(dev)
    plv = (0.5 * torch.randn(B, K, L, generator=g) - 1.0).to(dev)
    eps = torch.randn(S, B, K, L, generator=g).to(dev)
    x = torch.rand(B, 3, Si, Si, generator=g).to(dev)

    def new_route(model=model):
        return model.predictive(x, samples=S, posterior=(pm, plv), eps=eps)

    def old_route(model=model, ties=False):
        z = pm[None] + torch.exp(0.5 * plv)[None] * eps
        pred, mask, _ = model.decode(z.reshape(S * B, K, L))
        pred, mask = pred.reshape(S, B, 3, Si, Si), mask.reshape(S, B, K, 1, Si, Si)
        out = dict(pred_mean=pred.mean(0), pred_var=pred.var(0, unbiased=False), mask_mean=mask.mean(0), mask_var=mask.var(0, unbiased=False))
        win = mask[:, :, :, 0].argmax(2)
        out['votes'] = torch.stack([(win == k).sum(0) for k in range(K)], 1).to(torch.int32)
        if ties:                                                            # (only for the comparison before the timed loops)
            top2 = mask[:, :, :, 0].topk(2, dim=2).values
            out['tie'] = (top2[:, :, 0] == top2[:, :, 1]).any(0)           # pixels where some sample's two largest masks are equal
        del pred, mask
        model.posterior.mean, model.posterior.logvar, model.likelihood_maps = pm, plv, True
        try:
            out['ll'] = torch.stack([(model.elbo(x, eps=eps[s]), model.log_likelihood.sum((1, 2, 3)))[1] for s in range(S)])
        finally:
            model.posterior.mean = model.posterior.logvar = None
            model.likelihood_maps = False
        return out

    a, b = new_route(), old_route(ties=True)
    check = dict(pred_mean_max_diff=float((a.pred_mean - b['pred_mean']).abs().max()), pred_var_max_diff=float((a.pred_var - b['pred_var']).abs().max()),
                 mask_mean_max_diff=float((a.mask_mean - b['mask_mean']).abs().max()), votes_differ_pixels=int((a.votes != b['votes']).any(1).sum()),
                 votes_differ_pixels_without_a_tie=int(((a.votes != b['votes']).any(1) & ~b['tie']).sum()),
                 ll_max_rel_diff=float(((a.ll - b['ll']).abs() / b['ll'].abs()).max()))
    del a, b
    runs = {'predictive': new_route, 'by_hand': old_route}
    times = {k: [] for k in runs}
    for r in range(warmup + reps):
        for k, fn in runs.items():
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    # peak memory of one run of each route on a module of its own (a module keeps the largest workspace it ever needed)
    peaks = {}
    for k, fn in runs.items():
        fresh = make_model()
        peaks[k] = peak_bytes(lambda: fn(fresh))
        del fresh
        torch.cuda.empty_cache()
    # the accumulate launches alone, in a pass of their own
    model.set_option('profile', 2)
    new_route()
    model.profile_read('predictive')
    for _ in range(3):
        new_route()
    acc_ms, acc_n = model.profile_read('predictive')
    model.set_option('profile', 0)
    med = lambda v: sorted(v)[len(v) // 2]
    P = Si * Si
    launches = acc_n // 3
    # decoder output per pixel and sample; per launch the packed image once and the state in and out (K <= 8: registers for the launch)
    nbytes = S * B * P * 16 * K + launches * B * P * (16 + 2 * (2 * K + 6) * 4 + 2 * K * 4)
    out = {k + '_ms_median': round(med(v), 4) for k, v in times.items()}
    out.update({k + '_ms_min': round(min(v), 4) for k, v in times.items()})
    out.update({k + '_ms_max': round(max(v), 4) for k, v in times.items()})
    out.update({k + '_peak_bytes': v for k, v in peaks.items()})
    out.update(config=name, K=K, B=B, L=L, S=Si, samples=S, max_batch=model.max_batch(K=K), by_hand_over_predictive=round(med(times['by_hand']) / med(times['predictive']), 2),
               accumulate_ms_per_call=round(acc_ms / 3, 4), accumulate_launches_per_call=launches, accumulate_algorithmic_bytes=nbytes,
               accumulate_bytes_per_s=round(nbytes / (acc_ms / 3 * 1e-3), 1) if acc_ms > 0 else None,
               accumulate_fraction_of_8TBps=round(nbytes / (acc_ms / 3 * 1e-3) / PEAK_BPS, 4) if acc_ms > 0 else None, **check)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('predictive_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = [measure(n, a, K, B, args.samples, args.reps, args.warmup, dev) for n, a, K, B in CONFIGS]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        with open(args.md, 'w') as f:
            f.write('| config | B | K | samples | predictive ms | by hand ms | by hand / predictive | peak MB predictive | peak MB by hand |\n|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| {} | {} | {} | {} | {:.2f} ({:.2f} .. {:.2f}) | {:.2f} ({:.2f} .. {:.2f}) | {:.2f} | {:.0f} | {:.0f} |\n'.format(
                    r['config'], r['B'], r['K'], r['samples'], r['predictive_ms_median'], r['predictive_ms_min'], r['predictive_ms_max'],
                    r['by_hand_ms_median'], r['by_hand_ms_min'], r['by_hand_ms_max'], r['by_hand_over_predictive'],
                    r['predictive_peak_bytes'] / 1e6, r['by_hand_peak_bytes'] / 1e6))
            f.write('\n| config | accumulate ms per call | launches | algorithmic MB | algorithmic bytes / s | fraction of 8 TB/s |\n|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| {} | {:.4f} | {} | {:.1f} | {} | {} |\n'.format(r['config'], r['accumulate_ms_per_call'], r['accumulate_launches_per_call'],
                                                                          r['accumulate_algorithmic_bytes'] / 1e6, r['accumulate_bytes_per_s'],
                                                                          r['accumulate_fraction_of_8TBps']))


if __name__ == '__main__':
    main()
