"""Time of one training step with an image that requires grad, with weights that require grad and with ``model.likelihood_maps``, HIP events
after warm-up.

    python tools/input_grad_step_time.py [--config dsprites] [--batch 8] [--iters 5] [--steps 20] [--warmup 3] [--out FILE]

Prints one JSON line: ms per step (forward + backward, single images, no optimizer step) of
    plain            x and weights are data, loss.backward()
    x_grad           x requires grad: one more per-pixel kernel per evaluation (option input_grad 1), one read-back of (B, 3, S, S) per step
    w_grad           weights= of ones that require grad (option input_grad 2), one read-back of (B, S, S); its own yardstick is plain_w, the
                     same step with the same weights as data
    maps             model.likelihood_maps = True: one per-pixel launch per step writing (B, 3, S, S) + (B, K, 3, S, S)
and, from the kernel categories (option profile 2, a separate pass), the mean time per launch of pixel_input_grad next to pixel_sigma_grad's
slot pixel_pass1.  The modes alternate step by step in one process.  IODINE_HIP_LIB selects another build of the library for the plain
step (an older build knows none of this: pass --plain-only)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE, synth                                   # noqa: E402
from iodine_amd.model import clevr6_arch, dsprites_arch                # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', choices=['clevr6', 'dsprites'], default='dsprites')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    arch = (clevr6_arch if args.config == 'clevr6' else dsprites_arch)(iters=args.iters)
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    model.manual_seed(1)
    S = arch.IMG_SIZE
    x = torch.from_numpy(synth.make_images(args.batch, S, seed=2, kind='blobs')[0]).to(dev)
    ones = torch.ones(args.batch, 1, S, S, device=dev)

    def step(x_grad=False, w=None, w_grad=False, maps=False):
        def run():
            model.likelihood_maps = maps
            model.zero_grad(set_to_none=True)
            xi = x.detach().requires_grad_(x_grad)
            if w is None:
                model(xi).backward()
            else:
                model(xi, weights=w.detach().requires_grad_(w_grad)).backward()
        return run

    runs = {'plain': step()}
    if not args.plain_only:
        runs.update(x_grad=step(x_grad=True), plain_w=step(w=ones), w_grad=step(w=ones, w_grad=True), maps=step(maps=True))
    times = {k: [] for k in runs}
    for i in range(args.warmup + args.steps):
        for k, fn in runs.items():
            t = timed(fn)
            if i >= args.warmup:
                times[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    out = dict(config=args.config, batch=args.batch, iters=args.iters, steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), lib=os.environ.get('IODINE_HIP_LIB', 'in-tree'),
               ms_median={k: round(med(v), 3) for k, v in times.items()}, ms_min={k: round(min(v), 3) for k, v in times.items()},
               ms_max={k: round(max(v), 3) for k, v in times.items()})
    if not args.plain_only:
        # the kernels by themselves: event-bracketed launches, a pass of its own (the brackets cost time: not part of the figures above)
        model.set_option('profile', 2)
        for cat in ('pixel_input_grad', 'pixel_pass1'):
            model.profile_read(cat)
        for _ in range(3):
            runs['x_grad']()
        torch.cuda.synchronize()
        us = {}
        for cat in ('pixel_input_grad', 'pixel_pass1'):
            tot, n = model.profile_read(cat)
            us[cat] = round(1000.0 * tot / max(n, 1), 2)
        model.set_option('profile', 0)
        K, P = arch.SLOTS, S * S
        bytes_x = args.batch * P * (16 * K + 16 + 12 + 12)                 # decoder output + packed image in, three planes read + written
        out['us_per_launch'] = us
        out['input_grad_GBps'] = round(bytes_x / (us['pixel_input_grad'] * 1e-6) / 1e9, 1) if us['pixel_input_grad'] > 0 else None
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
