"""Time of one training step with per-frame auxiliary losses (``forward(x, attach_frames=...)``), HIP events after warm-up.

    python tools/frame_aux_step_time.py [--config dsprites] [--batch 8] [--iters 5] [--steps 10] [--warmup 3] [--out FILE]

Prints one JSON line: ms per step (forward + backward, single images, no optimizer step) of
    plain         loss.backward()
    attach_state  attach_state=True, (loss + <W, model.mask>).backward()
    frame_T       attach_frames=[T], the same cotangent on frames['mask'][0]
    all_frames    attach_frames=True, a mask cotangent on every one of the T + 1 evaluations
The modes alternate step by step in one process."""
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
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    arch = (clevr6_arch if args.config == 'clevr6' else dsprites_arch)(iters=args.iters)
    T = args.iters
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    model.manual_seed(1)
    x = torch.from_numpy(synth.make_images(args.batch, arch.IMG_SIZE, seed=2, kind='blobs')[0]).to(dev)
    W = torch.randn((T + 1, args.batch, model.K, 1, arch.IMG_SIZE, arch.IMG_SIZE), device=dev)

    def plain():
        model.zero_grad(set_to_none=True)
        model(x).backward()

    def attach_state():
        model.zero_grad(set_to_none=True)
        loss = model(x, attach_state=True)
        (loss + (W[T] * model.mask).sum()).backward()

    def frame_T():
        model.zero_grad(set_to_none=True)
        loss = model(x, attach_frames=[T])
        (loss + (W[T] * model.frames['mask'][0]).sum()).backward()

    def all_frames():
        model.zero_grad(set_to_none=True)
        loss = model(x, attach_frames=True)
        (loss + (W * model.frames['mask']).sum()).backward()

    runs = {'plain': plain, 'attach_state': attach_state, 'frame_T': frame_T, 'all_frames': all_frames}
    times = {k: [] for k in runs}
    for i in range(args.warmup + args.steps):
        for k, fn in runs.items():
            t = timed(fn)
            if i >= args.warmup:
                times[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    out = dict(config=args.config, batch=args.batch, iters=T, steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0),
               ms_median={k: round(med(v), 3) for k, v in times.items()}, ms_min={k: round(min(v), 3) for k, v in times.items()},
               ms_max={k: round(max(v), 3) for k, v in times.items()})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
