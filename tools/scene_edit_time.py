"""Time of a latent traversal through ``iodine_amd.traverse`` (one ``IODINE.edit`` call: the scene decoded once, one slot-image per
variation) against ``model.decode`` on the same E fully materialised scenes (chunked by ``max_batch()`` - the only route before
``edit`` existed, and the yardstick), HIP events after warm-up.

    python tools/scene_edit_time.py [--reps 7] [--warmup 2] [--out FILE.json] [--md FILE.md]

Two configurations, each one scene (B = 1) and every latent unit of ONE slot at 7 values: the CLEVR architecture at K = 7 (64 units,
E = 448) and the dSprites architecture at K = 6 (16 units, E = 112); synthetic weights, random z (the time does not depend on either).
One sample is one whole call between two events; the two routes alternate sample by sample in one process and the figure is the median
of ``reps`` samples.  Both routes return pred only to the caller's view of the problem - the decode route cannot avoid writing mask and
mean as well, which is part of what it costs.  Before anything is timed the two preds are compared (a replace edit promises the bits of
the decode).  A separate pass under the library's event profiler (option profile 2, after the timed loops: the brackets idle the GPU)
gives the time of the per-pixel rendering launches (category "scene_edit"); their algorithmic bytes are E P (16 K + 12): K float4 read
and three floats of pred written per pixel and edit.  The register counts in the note are the compiler's (-Rpass-analysis=kernel-resource-usage)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE, synth                                    # noqa: E402
from iodine_amd.model import clevr6_arch, dsprites_arch                 # noqa: E402
from iodine_amd.traverse import build_edits, traverse                   # noqa: E402

CONFIGS = (('clevr', clevr6_arch, 7), ('dsprites', dsprites_arch, 6))
N_VALUES = 7
PEAK_BPS = 8e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, make_arch, K, reps, warmup, dev):
    arch = make_arch()
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    L, S = int(arch.DIM_LATENT), int(arch.IMG_SIZE)
    g = torch.Generator().manual_seed(11)
    z = torch.randn(1, K, L, generator=g).to(dev)
    values = torch.linspace(-2.0, 2.0, N_VALUES)
    dims = list(range(L))
    slot, z_new = build_edits(z[0], [0], [dims], values, 'set')
    E = int(slot.numel())
    ze = z.repeat(E, 1, 1)
    ze[:, 0] = z_new                                                   # the E scenes, fully materialised

    def new_route():
        return traverse(model, z, image=0, slots=[0], dims=dims, values=values, mode='set').pred

    def old_route():
        return model.decode(ze)[0]

    a, b = new_route().reshape(E, 3, S, S), old_route()
    same = bool(torch.equal(a, b))
    max_diff = float((a - b).abs().max())
    del a, b
    runs = {'edit': new_route, 'decode': old_route}
    times = {k: [] for k in runs}
    for r in range(warmup + reps):
        for k, fn in runs.items():
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    # the rendering launches alone, in a pass of their own
    model.set_option('profile', 2)
    new_route()
    model.profile_read('scene_edit')
    for _ in range(3):
        new_route()
    comp_ms, comp_n = model.profile_read('scene_edit')
    model.set_option('profile', 0)
    med = lambda v: sorted(v)[len(v) // 2]
    P = S * S
    nbytes = E * P * (16 * K + 12)
    out = {k + '_ms_median': round(med(v), 4) for k, v in times.items()}
    out.update({k + '_ms_min': round(min(v), 4) for k, v in times.items()})
    out.update({k + '_ms_max': round(max(v), 4) for k, v in times.items()})
    out.update(config=name, K=K, L=L, S=S, edits=E, max_batch=model.max_batch(K=K), bitwise_equal=same, max_abs_diff=max_diff,
               decode_over_edit=round(med(times['decode']) / med(times['edit']), 2), flop_ratio=round(E * K / (K + E), 2),
               render_ms_per_call=round(comp_ms / 3, 4), render_launches_per_call=comp_n // 3, render_algorithmic_bytes=nbytes,
               render_fraction_of_8TBps=round(nbytes / (comp_ms / 3 * 1e-3) / PEAK_BPS, 4) if comp_ms > 0 else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_edit_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = [measure(n, a, K, args.reps, args.warmup, dev) for n, a, K in CONFIGS]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        with open(args.md, 'w') as f:
            f.write('| config | K | E | edit ms | decode ms | decode / edit | FLOP ratio E K / (K + E) | pred bitwise equal |\n|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| {} | {} | {} | {:.2f} ({:.2f} .. {:.2f}) | {:.2f} ({:.2f} .. {:.2f}) | {:.2f} | {:.2f} | {} |\n'.format(
                    r['config'], r['K'], r['edits'], r['edit_ms_median'], r['edit_ms_min'], r['edit_ms_max'], r['decode_ms_median'],
                    r['decode_ms_min'], r['decode_ms_max'], r['decode_over_edit'], r['flop_ratio'], r['bitwise_equal']))
            f.write('\n| config | rendering ms per call | launches | algorithmic MB | fraction of 8 TB/s |\n|---|---|---|---|---|\n')
            for r in rows:
                f.write('| {} | {:.4f} | {} | {:.1f} | {} |\n'.format(r['config'], r['render_ms_per_call'], r['render_launches_per_call'],
                                                                     r['render_algorithmic_bytes'] / 1e6, r['render_fraction_of_8TBps']))


if __name__ == '__main__':
    main()
