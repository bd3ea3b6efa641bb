"""Time of one clip training step (iodine_amd.engine.clip_backward) under truncated and exact BPTT, HIP events after warm-up.

    python tools/clip_step_time.py [--config dsprites] [--batch 8] [--frames 11] [--iters 5] [--steps 10] [--warmup 3] [--out FILE]

Prints one JSON line: ms per clip step (forward(s) + backward(s) of every chunk, no optimizer step) for both modes, next to the plain
single-chunk step (one forward + backward at the same T) the chunks are made of.  The two modes alternate step by step in one process."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE, synth                                   # noqa: E402
from iodine_amd.engine import clip_backward, clip_chunks               # noqa: E402
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
    ap.add_argument('--frames', type=int, default=11)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    arch = (clevr6_arch if args.config == 'clevr6' else dsprites_arch)(iters=args.iters)
    chunks = clip_chunks(args.frames, args.iters)
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    model.manual_seed(1)
    x = torch.from_numpy(synth.make_images(args.batch, arch.IMG_SIZE, seed=2, kind='blobs')[0]).to(dev)
    clip = torch.stack([torch.roll(x, shifts=(f, 2 * f), dims=(-2, -1)) for f in range(args.frames)], 1).contiguous()
    first = clip[:, :args.iters + 1].contiguous()

    def plain():
        model.zero_grad(set_to_none=True)
        model(first).backward()

    def step(bptt):
        model.zero_grad(set_to_none=True)
        clip_backward(model, clip, bptt=bptt)

    runs = {'single_chunk': plain, 'truncated': lambda: step('truncated'), 'exact': lambda: step('exact')}
    times = {k: [] for k in runs}
    for i in range(args.warmup + args.steps):
        for k, fn in runs.items():
            t = timed(fn)
            if i >= args.warmup:
                times[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    out = dict(config=args.config, batch=args.batch, frames=args.frames, iters=args.iters, chunks=len(chunks), steps=args.steps,
               warmup=args.warmup, device=torch.cuda.get_device_name(0),
               ms_median={k: round(med(v), 3) for k, v in times.items()}, ms_min={k: round(min(v), 3) for k, v in times.items()},
               ms_max={k: round(max(v), 3) for k, v in times.items()})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
