"""Time of a training step and of ``reconstruct`` under ``model.likelihood = 'per_channel'`` and ``'joint'``, HIP events after warm-up.

    python tools/joint_likelihood_time.py [--config clevr6|dsprites] [--batch 32] [--steps 10] [--warmup 3] [--out FILE]

Prints one JSON line: ms per training step (forward + backward, no optimizer step) and per ``reconstruct`` in both modes - the modes
alternate step by step in one process - and, from a second pass with option ``profile`` 2 (HIP events around every launch, not part of
the timed steps), the time per launch of ``pixel_pass1`` and of ``pixel_pass2`` / ``refine_l0f`` (whichever the shape takes) per mode.
IODINE_HIP_LIB selects another build of the library (an older build does not know the option: pass --default-only)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE, synth                                   # noqa: E402
from iodine_amd.model import clevr6_arch, dsprites_arch                # noqa: E402

CATEGORIES = ('pixel_pass1', 'pixel_pass2', 'refine_l0f')


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', choices=['clevr6', 'dsprites'], default='clevr6')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--default-only', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    arch = (clevr6_arch if args.config == 'clevr6' else dsprites_arch)()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    x = torch.from_numpy(synth.make_images(args.batch, arch.IMG_SIZE, seed=0, kind='uniform')).to(dev)
    eps = torch.from_numpy(synth.make_eps(arch.ITERS, args.batch, arch.SLOTS, arch.DIM_LATENT, seed=1)).to(dev)
    modes = ('per_channel',) if args.default_only else ('per_channel', 'joint')

    def train(mode):
        def run():
            if not args.default_only:
                model.likelihood = mode
            model.zero_grad(set_to_none=True)
            model(x, eps).backward()
        return run

    def infer(mode):
        def run():
            if not args.default_only:
                model.likelihood = mode
            with torch.no_grad():
                model.reconstruct(x, eps)
        return run

    runs = {(kind, mode): fn(mode) for kind, fn in (('train', train), ('reconstruct', infer)) for mode in modes}
    times = {k: [] for k in runs}
    for i in range(args.warmup + args.steps):
        for k, fn in runs.items():
            t = timed(fn)
            if i >= args.warmup:
                times[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    # per-launch times: every launch bracketed by events, a pass of its own
    model.set_option('profile', 2)
    launch = {}
    for mode in modes:
        for c in CATEGORIES:
            model.profile_read(c)
        for _ in range(3):
            runs[('train', mode)]()
        torch.cuda.synchronize()
        launch[mode] = {}
        for c in CATEGORIES:
            tot, cnt = model.profile_read(c)
            if cnt:
                launch[mode][c] = dict(us_per_launch=round(1e3 * tot / cnt, 2), launches=cnt)
    model.set_option('profile', 0)
    out = dict(config=args.config, batch=args.batch, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               lib=os.environ.get('IODINE_HIP_LIB', 'in-tree'),
               ms_median={f'{k[0]}/{k[1]}': round(med(v), 3) for k, v in times.items()},
               ms_min={f'{k[0]}/{k[1]}': round(min(v), 3) for k, v in times.items()},
               ms_max={f'{k[0]}/{k[1]}': round(max(v), 3) for k, v in times.items()}, training_step_launches=launch)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
