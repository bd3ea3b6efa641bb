"""Windowed batches (iodine_amd.windows, iodine_batch_window) timed on one GPU, in one call:

    python tools/window_time.py [--batch 32] [--items 1024] [--steps 20] [--warm-steps 3] [--out FILE.json] [--md FILE.md]

Per batch of CLEVR-sized windows (240 x 320 uint8 frames with masks of six objects, crop 192 -> 128):
* ``iodine_batch_window`` with the centre window and with ``Augment`` windows (random scale, aspect, position, flip, gain);
* (a) ``iodine_batch_gather`` on a store resized beforehand - what a run without windows launches, the floor;
* (b) the centre-crop transform from torch ops on the device: index, crop, ``F.interpolate(..., antialias=True)``, ``flip``, and
  nearest-exact on the unpacked planes.
HIP events over back-to-back launches with a fresh random index list (and window rows) per launch; median (min .. max) of the samples.
Then the dSprites training step (64 x 64, ``engine.train``, host clock, synchronised) fed by ``ResidentDataset.batches`` and by
``FrameStore.from_resident(store).batches(..., Augment(...))``, alternating, two rounds each.  Prints one JSON line; ``--md`` writes
profiles/window_timing.md."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iodine_amd import _lib, engine                                       # noqa: E402
from iodine_amd.resident import ResidentDataset                            # noqa: E402
from iodine_amd.windows import Augment, Center, FrameStore                 # noqa: E402

PEAK_BPS = 8e12
H, W, CROP, S, G = 240, 320, 192, 128, 6
AUGMENT = dict(scale=(0.7, 1.0), ratio=(0.8, 1.25), translate=8, flip=True, gain=0.1)


def med(v):
    return sorted(v)[len(v) // 2]


def make_frames(n, dev):
    """n CLEVR-sized frames on the device: noise images, six rectangles per frame as mask words"""
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8, device=dev)
    words = torch.zeros((n, H, W), dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    for o in range(G):
        y, x, h, w = rng.integers(30, H - 90), rng.integers(70, W - 130), rng.integers(20, 60), rng.integers(20, 60)
        words[:, y:y + h, x:x + w] = 1 << o                                  # (painter's order; the same boxes in every frame)
    return FrameStore(images, words.to(torch.int16).view(torch.uint16), torch.full((n,), G, dtype=torch.uint8), device=dev)


def resized_store(frames, batch):
    """the centre windows of every frame frozen into a ResidentDataset, as ingestion at one size would"""
    xs, ms = [], []
    for lo in range(0, len(frames), batch):
        idx = list(range(lo, min(lo + batch, len(frames))))
        x, gt, _ = frames.window(idx, S, Center(CROP))
        xs.append((x * 255.0).round().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
        w = torch.zeros(gt.shape[:1] + gt.shape[2:], dtype=torch.int32, device=gt.device)
        for g in range(gt.shape[1]):
            w |= gt[:, g].to(torch.int32) << g
        ms.append(w.to(torch.int16).view(torch.uint16))
    return ResidentDataset(torch.cat(xs), torch.cat(ms), frames.n_gt)


def timed(launch, reps, inner):
    """ms per call of ``launch(i)``, i = 0..inner-1 back to back between two events: (median, min, max) over reps after 3 warm-ups"""
    times = []
    for r in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(inner):
            launch(i)
        b.record(); b.synchronize()
        if r >= 3:
            times.append(a.elapsed_time(b) / inner)
    return dict(ms_median=round(med(times), 5), ms_min=round(min(times), 5), ms_max=round(max(times), 5))


def torch_centre(frames, idx, flip):
    """(b): the centre-crop transform from torch ops - one fixed box for the batch (a box per item would need a loop over items)"""
    top, left = (H - CROP) // 2, (W - CROP) // 2
    img = frames.images[idx][:, top:top + CROP, left:left + CROP].permute(0, 3, 1, 2).float().div_(255.0)
    x = F.interpolate(img, size=(S, S), mode='bilinear', antialias=True, align_corners=False).clamp_(0, 1)
    x = torch.where(flip[:, None, None, None], x.flip(-1), x)
    w = frames.masks.view(torch.int16)[idx][:, top:top + CROP, left:left + CROP].to(torch.int32)
    planes = torch.stack([(w >> g) & 1 for g in range(G)], dim=1).float()
    gt = F.interpolate(planes, size=(S, S), mode='nearest-exact').to(torch.uint8)
    return x, torch.where(flip[:, None, None, None], gt.flip(-1), gt)


def launches(frames, small, batch, reps, inner, dev):
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream()
    g = torch.Generator().manual_seed(0)
    host_idx = [torch.randint(0, len(frames), (batch,), generator=g) for _ in range(inner)]
    idx = [i.to(dev) for i in host_idx]
    x = torch.empty((batch, 3, S, S), dtype=torch.float32, device=dev)
    gt = torch.empty((batch, G, S, S), dtype=torch.uint8, device=dev)
    rows = {'centre': Center(CROP), 'augment': Augment(crop=CROP, **AUGMENT)}
    out = {}
    for name, policy in rows.items():
        dev_rows = [torch.from_numpy(policy.rows(i.numpy(), H, W, S, seed=1, epoch=k)).to(dev) for k, i in enumerate(host_idx)]
        out['window_' + name] = timed(lambda i: L.iodine_batch_window(st, p(idx[i]), batch, p(frames.images), 0, p(frames.masks), H, W,
                                                                       p(dev_rows[i]), S, G, p(x), p(gt)), reps, inner)
    out['gather_resized'] = timed(lambda i: L.iodine_batch_gather(st, p(idx[i]), batch, p(small.images), 0, p(small.masks), S, G, p(x), p(gt)),
                                  reps, inner)
    flips = [torch.rand((batch,), generator=g).lt(0.5).to(dev) for _ in range(inner)]
    out['torch_centre'] = timed(lambda i: torch_centre(frames, idx[i], flips[i]), reps, max(1, inner // 5))
    window_bytes = batch * (CROP * CROP * 3 + S * S * 2 + S * S * (12 + G))
    gather_bytes = batch * S * S * (3 + 2 + 12 + G)
    for k, v in out.items():
        v['bytes'] = gather_bytes if k == 'gather_resized' else window_bytes
        v['ms_at_8TBps'] = round(v['bytes'] / PEAK_BPS * 1e3, 5)
    tx, tgt = torch_centre(frames, idx[0], flips[0])                         # how far the torch transform is from the rule, for the record
    r = torch.from_numpy(Center(CROP).rows(host_idx[0].numpy(), H, W, S))
    r[:, 4] = flips[0].cpu().float()
    wx, wgt, _ = frames.window(host_idx[0], S, r.numpy())
    out['torch_vs_window'] = dict(image_max_abs=float((tx - wx).abs().max()), mask_pixels_differing=int((tgt != wgt).sum()))
    return out


def step_times(args, dev):
    from iodine_amd import IODINE
    from iodine_amd.model import dsprites_arch
    from iodine_amd.optim import make_optimizer
    arch = dsprites_arch()
    size = int(arch.IMG_SIZE)
    store = ResidentDataset.synthetic(args.step_items, size, device=dev)
    sources = {'resident': lambda: store.batches(args.batch, shuffle=True),
               'augment': lambda: FrameStore.from_resident(store).batches(args.batch, size, Augment(**AUGMENT), shuffle=True)}
    quiet = lambda *a: None
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    opt = make_optimizer(model, base_lr=3e-4)
    engine.train(model, opt, sources['resident'](), dev, args.warm_steps, print_every=10 ** 9, log=quiet)
    engine.train(model, opt, sources['augment'](), dev, args.warm_steps, print_every=10 ** 9, log=quiet)
    out = {k: [] for k in sources}
    for _ in range(args.rounds):                                             # alternating: A B A B on the same model
        for k, make in sources.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            engine.train(model, opt, make(), dev, args.steps, print_every=10 ** 9, log=quiet)
            torch.cuda.synchronize()
            out[k].append(round((time.perf_counter() - t) * 1e3 / args.steps, 3))
    return dict(size=size, batch=args.batch, steps=args.steps, items=args.step_items, step_ms=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--items', type=int, default=1024, help='240 x 320 frames of the store the launches are timed on')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warm-steps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--step-items', type=int, default=512, help='synthetic 64 x 64 scenes of the training-step comparison')
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('window_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    frames = make_frames(args.items, dev)
    small = resized_store(frames, args.batch)
    out = dict(device=torch.cuda.get_device_name(0), frames_mib=round(frames.nbytes() / 2 ** 20, 1), resized_mib=round(small.nbytes() / 2 ** 20, 1),
               launches=launches(frames, small, args.batch, args.reps, args.inner, dev), train=step_times(args, dev),
               args={k: v for k, v in vars(args).items() if k not in ('out', 'md')})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        write_md(args.md, out)


def write_md(path, out):
    a, la, tr = out['args'], out['launches'], out['train']
    names = {'window_centre': '`iodine_batch_window`, centre window 192 -> 128', 'window_augment': '`iodine_batch_window`, `Augment` windows',
             'gather_resized': '(a) `iodine_batch_gather`, store resized beforehand', 'torch_centre': '(b) torch ops, centre crop + flip'}
    with open(path, 'w') as f:
        f.write('# Windowed batches: the window launch against the plain gather and against torch ops\n\n')
        f.write(f'`python tools/window_time.py --batch {a["batch"]} --items {a["items"]} --steps {a["steps"]} --warm-steps {a["warm_steps"]}` on one '
                f'MI355X (the name torch reports is "{out["device"]}").  Everything below comes from that one call.\n\n')
        f.write(f'Store: {a["items"]} frames of {H} x {W} uint8 with mask words, {out["frames_mib"]} MiB; the same frames resized beforehand to '
                f'{S} x {S}: {out["resized_mib"]} MiB.  Batch {a["batch"]}, {G} mask planes.  Median (min .. max) of {a["reps"]} samples of '
                f'{a["inner"]} back-to-back launches between HIP events ((b): {max(1, a["inner"] // 5)} calls per sample), a fresh random index '
                'list and fresh window rows per launch; the outputs are the same two buffers every launch.  Bytes are the algorithm\'s: the '
                'crop\'s pixels and one mask word per output pixel read, 12 + planes per output pixel written; `Augment` windows are smaller '
                'than the crop on average, so their row overstates them.\n\n')
        f.write('| path | ms per batch | MB per batch | ms at 8 TB/s |\n|---|---|---|---|\n')
        for k in ('window_centre', 'window_augment', 'gather_resized', 'torch_centre'):
            v = la[k]
            f.write('| {} | {:.4f} ({:.4f} .. {:.4f}) | {:.2f} | {:.4f} |\n'.format(names[k], v['ms_median'], v['ms_min'], v['ms_max'], v['bytes'] / 1e6,
                                                                                   v['ms_at_8TBps']))
        wc, ga, tc = la['window_centre'], la['gather_resized'], la['torch_centre']
        f.write('\nThe window launch takes {:.1f}x the plain gather and {:.1f}x less than the torch ops.  Neither launch is near its bytes at 8 TB/s '
                '({:.0f}x and {:.0f}x away): a batch is too few bytes to keep the memory system busy, the gather sits at the cost of a back-to-back '
                'launch and the window launch on top of that pays the latency of its dependent steps - tap tables, horizontal pass of up to {} '
                'source rows per block, vertical pass - on one or two blocks per CU.\n'.format(
                    wc['ms_median'] / ga['ms_median'], tc['ms_median'] / wc['ms_median'], wc['ms_median'] / wc['ms_at_8TBps'],
                    ga['ms_median'] / ga['ms_at_8TBps'], 8 * CROP // S + 2 * (CROP // S + 1) + 1))
        tv = la['torch_vs_window']
        f.write('\nThe torch transform is not the rule bit for bit: on one batch its image differs from the window launch by at most '
                '{:.2e} and {} mask bytes differ.  It also cuts one box for the whole batch; a box per item would need a loop over the '
                'items.\n'.format(tv['image_max_abs'], tv['mask_pixels_differing']))
        f.write('\nThe dSprites training step ({0} x {0}, batch {1}, `engine.train`, host clock around {2} steps, synchronised, after {3} warm-up '
                'steps of each source), fed by `ResidentDataset.batches` and by `FrameStore.from_resident(store).batches(..., Augment(flip, '
                'scale 0.7:1, ratio 0.8:1.25, translate 8, gain 0.1))`, alternating on one model:\n\n'.format(tr['size'], tr['batch'], tr['steps'],
                                                                                                           a['warm_steps']))
        f.write('| source | step ms, per round |\n|---|---|\n')
        for k, v in tr['step_ms'].items():
            f.write('| {} | {} |\n'.format(k, ', '.join(f'{t:.2f}' for t in v)))
        d = [b - a_ for a_, b in zip(tr['step_ms']['resident'], tr['step_ms']['augment'])]
        f.write('\nDifference per round: {} ms of a step ({} of it).  What the augmented source adds is the window launch in place of the gather '
                '(microseconds, above) and, once per epoch of {} batches, the window rows computed on the host and one more upload; the two were '
                'not separated, and with two rounds the spread of a round is known no better than the table shows.\n'.format(
                    ', '.join(f'{x:+.2f}' for x in d), ', '.join(f'{100 * x / a_:+.1f} %' for x, a_ in zip(d, tr['step_ms']['resident'])),
                    -(-tr['items'] // tr['batch'])))
        f.write('\nNot measured: real CLEVR files, several GPUs, kernel time from a profiler trace, other batch sizes.\n')


if __name__ == '__main__':
    main()
