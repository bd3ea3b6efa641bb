"""Input side of a training step: the DataLoader path against the device-resident store (iodine_amd.resident), in one call on one GPU.

    python tools/resident_time.py [--batch 32] [--steps 10] [--warm-steps 3] [--epochs 20] [--out FILE.json] [--md FILE.md]

For the dSprites (64 x 64) and CLEVR (128 x 128) architectures at batch 32:
* batches per second of ``make_dataloader``'s loader with 0 and 16 workers - a batch counts when it is where a training step needs it: ``x`` on
  the device and, for labelled data, ``pack_gt`` done - and of ``ResidentDataset.batches``;
* wall time per training step of ``engine.train`` fed by each (host clock around ``train``, synchronised; warm-up steps first);
* the gather launch alone (HIP events over back-to-back launches) against its algorithmic bytes at 8 TB/s.
Sources: the engine's default ``SyntheticScenes`` at both sizes, and for CLEVR a generated folder in the data set's format (320 x 240 PNG
frames, six objects and their colour-coded masks) read through ``data.CLEVR`` - there the loader pays PIL, the colour separation and
``pack_gt`` per item.  Worker processes are spawned, not forked (they must not inherit the GPU), persist across epochs, and the timed epoch
is the second one, so their start-up is not in the figures.  Also re-measures, on this machine's CPU, the two host costs per image.
Prints one JSON line; ``--md`` writes profiles/resident_timing.md."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iodine_amd import _lib, data, engine, synth                       # noqa: E402
from iodine_amd.matching import pack_gt                                 # noqa: E402
from iodine_amd.resident import ResidentDataset                         # noqa: E402

PEAK_BPS = 8e12
OBJECT_COLOURS = [(200, 30, 30), (30, 200, 30), (30, 30, 200), (200, 200, 30), (30, 200, 200), (200, 30, 200)]


def med(v):
    return sorted(v)[len(v) // 2]


def clevr_frame(rng, h=240, w=320):
    """one (image, colour-coded mask) pair in CLEVR's format: six rectangles on the (64, 64, 64) background"""
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = np.empty((h, w, 3), dtype=np.uint8)
    mask[:] = data.CLEVR_BACKGROUND
    for c in OBJECT_COLOURS:
        y, x = int(rng.integers(30, h - 90)), int(rng.integers(70, w - 130))
        mask[y:y + int(rng.integers(20, 60)), x:x + int(rng.integers(20, 60))] = c
    return img, mask


def write_clevr_folder(root, n, seed=0):
    from PIL import Image
    os.makedirs(os.path.join(root, 'images')), os.makedirs(os.path.join(root, 'masks'))
    rng = np.random.default_rng(seed)
    for i in range(n):
        img, mask = clevr_frame(rng)
        Image.fromarray(img).save(os.path.join(root, 'images', f'{i:05d}.png'))
        Image.fromarray(mask).save(os.path.join(root, 'masks', f'{i:05d}.png'))


def host_costs():
    """the two per-image host costs, one core, median of repeats (ms)"""
    img, mask = clevr_frame(np.random.default_rng(1))
    a, b = [], []
    for _ in range(7):
        t = time.perf_counter(); data.clevr_image(img); data.clevr_masks(mask); a.append((time.perf_counter() - t) * 1e3)
    for _ in range(30):
        t = time.perf_counter(); synth.make_images(1, 128, kind='blobs'); b.append((time.perf_counter() - t) * 1e3)
    return dict(clevr_image_plus_masks_320x240_ms=round(med(a), 2), make_images_blobs_128_ms=round(med(b), 3), torch_threads=torch.get_num_threads())


def loader(ds, batch, workers):
    kw = dict(multiprocessing_context='spawn', persistent_workers=True) if workers else {}
    return torch.utils.data.DataLoader(ds, batch_size=batch, collate_fn=data.collate_fn, shuffle=True, num_workers=workers, **kw)


def consume(batches, dev, size):
    """what a step needs of every batch; returns the number of batches"""
    n = 0
    for d in batches:
        x = d[0].to(dev)
        if d[1] is not None and not torch.is_tensor(d[1]):
            pack_gt(d[1], size, dev)
        n += 1
    torch.cuda.synchronize()
    return n


def batch_rate(make, dev, size, epochs):
    src = make()
    consume(src, dev, size)                                                  # first epoch: workers start, code objects load
    t = time.perf_counter()
    n = sum(consume(src, dev, size) for _ in range(epochs))
    return n / (time.perf_counter() - t), src


def step_time(src, arch, dev, steps, warm):
    from iodine_amd import IODINE
    from iodine_amd.optim import make_optimizer
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    opt = make_optimizer(model, base_lr=3e-4)
    quiet = lambda *a: None
    engine.train(model, opt, src, dev, warm, print_every=10 ** 9, log=quiet)
    torch.cuda.synchronize()
    t = time.perf_counter()
    engine.train(model, opt, src, dev, steps, print_every=10 ** 9, log=quiet)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def gather_launch(store, batch, reps, inner, dev):
    """ms per launch (median, min, max) with a fresh random index list per launch, and the algorithmic bytes"""
    L, S = _lib.lib(), store.size
    g = torch.Generator().manual_seed(0)
    idx = [torch.randint(0, len(store), (batch,), generator=g).to(dev) for _ in range(inner)]
    G = store.planes
    x = torch.empty((batch, 3, S, S), dtype=torch.float32, device=dev)
    gt = torch.empty((batch, G, S, S), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = []
    for r in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(inner):
            L.iodine_batch_gather(st, _lib.ptr(idx[i]), batch, _lib.ptr(store.images), store.image_kind, _lib.ptr(store.masks), S, G,
                                  _lib.ptr(x), _lib.ptr(gt))
        b.record(); b.synchronize()
        if r >= 3:
            times.append(a.elapsed_time(b) / inner)
    nbytes = batch * S * S * ((3 if store.image_kind == 0 else 12) + 2 + 12 + G)
    return dict(ms_median=round(med(times), 5), ms_min=round(min(times), 5), ms_max=round(max(times), 5), bytes=nbytes, planes=G,
                store_mib=round(store.nbytes() / 2 ** 20, 1), fraction_of_8TBps=round(nbytes / (med(times) * 1e-3) / PEAK_BPS, 4))


def as_uint8_store(store):
    """the same scenes quantised to 8 bits: a uint8 HWC store of the size a decoded data set has"""
    u8 = (store.images * 255.0).round().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return ResidentDataset(u8, store.masks, store.n_gt)


def measure(name, arch, ds_of, n_items, args, dev, tag):
    S, B = int(arch.IMG_SIZE), args.batch
    ds = ds_of(n_items)
    row = dict(config=name, source=tag, size=S, batch=B, items=n_items)
    t = time.perf_counter()
    # (ingestion in this process: forked workers would inherit the GPU this process has open)
    store = ResidentDataset.from_dataset(ds, dev) if tag != 'SyntheticScenes' else ResidentDataset.synthetic(n_items, S, device=dev)
    torch.cuda.synchronize()
    row['build_store_s'] = time.perf_counter() - t
    row['store'] = 'uint8' if store.image_kind == 0 else 'float32'
    srcs = {}
    for w in (0, 16):
        row[f'loader_w{w}_batches_per_s'], srcs[f'loader_w{w}'] = batch_rate(lambda: loader(ds, B, w), dev, S, 1)
    row['resident_batches_per_s'], srcs['resident'] = batch_rate(lambda: store.batches(B, shuffle=True), dev, S, args.epochs)
    for k, src in srcs.items():
        slow = k == 'loader_w0' and tag != 'SyntheticScenes'
        row[k + '_step_ms'] = step_time(src, arch, dev, max(2, args.steps // 3) if slow else args.steps, 1 if slow else args.warm_steps)
    for k in list(row):
        if isinstance(row[k], float):
            row[k] = round(row[k], 3)
    del srcs
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warm-steps', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--items', type=int, default=512, help='synthetic scenes per data set')
    ap.add_argument('--clevr-items', type=int, default=512, help='frames of the generated CLEVR folder (16 batches of 32: one per worker)')
    ap.add_argument('--gather-items', type=int, default=4096, help='scenes of the store the gather launch is timed on (128 x 128)')
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resident_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    from iodine_amd.model import clevr6_arch, dsprites_arch
    dev = torch.device('cuda', 0)
    host = host_costs()
    rows = [measure('dsprites', dsprites_arch(), lambda n: engine.SyntheticScenes(n, 64), args.items, args, dev, 'SyntheticScenes'),
            measure('clevr6', clevr6_arch(), lambda n: engine.SyntheticScenes(n, 128), args.items, args, dev, 'SyntheticScenes')]
    with tempfile.TemporaryDirectory() as tmp:
        write_clevr_folder(tmp, args.clevr_items)
        rows.append(measure('clevr6', clevr6_arch(), lambda n: data.CLEVR(tmp), args.clevr_items, args, dev, 'CLEVR folder'))
    big = ResidentDataset.synthetic(args.gather_items, 128, device=dev)
    gathers = [dict(store='float32 (N, 3, 128, 128)', **gather_launch(big, args.batch, 20, 50, dev)),
               dict(store='uint8 (N, 128, 128, 3)', **gather_launch(as_uint8_store(big), args.batch, 20, 50, dev))]
    small = ResidentDataset.synthetic(args.gather_items, 64, device=dev)
    gathers.append(dict(store='float32 (N, 3, 64, 64)', **gather_launch(small, args.batch, 20, 50, dev)))
    gathers.append(dict(store='float32 (N, 3, 128, 128), batch 256', **gather_launch(big, 256, 20, 50, dev)))   # enough bytes to leave the launch floor
    out = dict(device=torch.cuda.get_device_name(0), host=host, rows=rows, gather=gathers,
               args={k: v for k, v in vars(args).items() if k not in ('out', 'md')})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        write_md(args.md, out)


def write_md(path, out):
    a = out['args']
    with open(path, 'w') as f:
        f.write('# Device-resident data set against the DataLoader path\n\n')
        f.write(f'`python tools/resident_time.py --batch {a["batch"]} --steps {a["steps"]} --warm-steps {a["warm_steps"]} --epochs {a["epochs"]}` on one '
                f'MI355X (the name torch reports is "{out["device"]}"), {out["host"]["torch_threads"]} torch threads in the training process.  '
                'Everything below comes from that one call.\n\n')
        f.write('Batches per second: a batch counts when `x` is on the device and, for labelled data, `pack_gt` is done.  Loader figures are '
                'one whole epoch (the second: spawned, persistent workers are up); resident figures are '
                f'{a["epochs"]} epochs, each with its device sort and one copy of the permutation to the host.  Step time: host clock around '
                f'`engine.train` for {a["steps"]} steps after {a["warm_steps"]} warm-up steps (the CLEVR folder with 0 workers: {max(2, a["steps"] // 3)} '
                'after 1), synchronised, no mask loss.  One run each; the spread was not measured.\n\n')
        f.write('| architecture | source | items | store | loader 0 workers, batches/s | loader 16 workers, batches/s | resident, batches/s | '
                'step ms, loader 0 | step ms, loader 16 | step ms, resident |\n|---|---|---|---|---|---|---|---|---|---|\n')
        for r in out['rows']:
            f.write('| {config} ({size} x {size}) | {source} | {items} | {store} | {loader_w0_batches_per_s:.2f} | {loader_w16_batches_per_s:.2f} | '
                    '{resident_batches_per_s:.1f} | {loader_w0_step_ms:.1f} | {loader_w16_step_ms:.1f} | {resident_step_ms:.1f} |\n'.format(**r))
        f.write('\nBuilding the store, once (seconds; generated on the device for the synthetic scenes, ingested by this process without workers for '
                'the folder - its fast colour separation included): ' + ', '.join('{config} / {source}: {build_store_s:.2f}'.format(**r)
                                                                                  for r in out['rows']) + '.\n')
        f.write('\nThe gather launch alone, batch {} (256 in the last row) with a fresh random index list per launch, median (min .. max) of 20 samples of 50 back-to-back '
                'launches between HIP events.  Bytes: 3 (float32 store: 12) + 2 read and 12 + planes written per pixel.  The outputs are the same '
                'two buffers every launch, so the writes can stay in cache; how much of the reads can is a matter of the store size in the table '
                'against the 256 MB last-level cache.\n\n'.format(a['batch']))
        f.write('| store | store MiB | planes | ms per launch | MB per launch | ms at 8 TB/s | fraction of 8 TB/s |\n|---|---|---|---|---|---|---|\n')
        for g in out['gather']:
            f.write('| {store} | {store_mib} | {planes} | {ms_median:.4f} ({ms_min:.4f} .. {ms_max:.4f}) | {mb:.2f} | {ideal:.4f} | {fraction_of_8TBps:.3f} |\n'.format(
                mb=g['bytes'] / 1e6, ideal=g['bytes'] / PEAK_BPS * 1e3, **g))
        b32 = [g for g in out['gather'] if 'batch' not in g['store']]
        lo, hi = min(b32, key=lambda g: g['bytes']), max(b32, key=lambda g: g['bytes'])
        f.write('\nAt batch {}, the launch with the fewest bytes ({:.1f} MB) takes {:.4f} ms, the one with the most ({:.1f} MB) {:.4f} ms: {:.1f}x the bytes in '
                '{:.2f}x the time.  Where that second ratio is near 1 the launch is bound by the cost of a back-to-back kernel launch, a few '
                'microseconds, not by HBM: such a batch is too few bytes to keep the memory system busy for longer than that, and the last '
                'row shows what the kernel reaches with eight times the bytes.\n'.format(
                    a['batch'], lo['bytes'] / 1e6, lo['ms_median'], hi['bytes'] / 1e6, hi['ms_median'], hi['bytes'] / lo['bytes'], hi['ms_median'] / lo['ms_median']))
        h = out['host']
        f.write('\nHost costs per image on this machine\'s CPU (median, {} torch threads): `data.clevr_image` + `data.clevr_masks` on a 320 x 240 '
                'frame with six objects, without PNG decoding: {} ms; `synth.make_images(1, 128, kind=\'blobs\')`: {} ms.\n'.format(
                    h['torch_threads'], h['clevr_image_plus_masks_320x240_ms'], h['make_images_blobs_128_ms']))
        f.write('\nNot measured: real CLEVR / multi-dSprites files, several GPUs, the spread between runs, kernel time from a profiler trace.\n')


if __name__ == '__main__':
    main()
