"""Time of one training step with a differentiable ``model.sigma`` and with ``model.stable_encoding``, HIP events after warm-up.

    python tools/sigma_grad_step_time.py [--config dsprites] [--batch 8] [--iters 5] [--steps 20] [--warmup 3] [--out FILE]

Prints one JSON line: ms per step (forward + backward, single images, no optimizer step) of
    plain            model.sigma a float, loss.backward()
    sigma_grad       model.sigma a device tensor that requires grad: one more per-pixel kernel and a one-block reduction per evaluation,
                     one small read-back and three torch ops per step
    stable_encoding  model.stable_encoding = True, sigma a float
The modes alternate step by step in one process.  IODINE_HIP_LIB selects another build of the library for the plain step (an older build
knows neither option: pass --plain-only)."""
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
    x = torch.from_numpy(synth.make_images(args.batch, arch.IMG_SIZE, seed=2, kind='blobs')[0]).to(dev)
    sigma = torch.tensor(float(arch.SIGMA), device=dev, requires_grad=True)

    def step(s, stable):
        def run():
            model.sigma, model.stable_encoding = s, stable
            model.zero_grad(set_to_none=True)
            sigma.grad = None
            model(x).backward()
        return run

    runs = {'plain': step(float(arch.SIGMA), False)}
    if not args.plain_only:
        runs.update(sigma_grad=step(sigma, False), stable_encoding=step(float(arch.SIGMA), True))
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
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
