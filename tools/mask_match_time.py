"""Time of ``iodine_amd.matching.matched_mask_loss`` - forward and backward, three launches - against the eager composite a user writes
without it, and the step time of a dSprites training step with and without the term.  HIP events after warm-up.

    python tools/mask_match_time.py [--reps 50] [--inner 20] [--warmup 5] [--step-reps 20] [--out FILE.json] [--md FILE.md]

Shapes (B, K, G, S) = (32, 7, 6, 128) - the benchmarked CLEVR config with six objects - and (32, 6, 4, 64).  One sample is the time of
``inner`` back-to-back forward + backward calls between two events divided by ``inner``; the two contenders alternate sample by sample in
one process, the figure is the median of ``reps`` samples; every shape is warmed first.  The eager composite is the yardstick: einsum
statistics over (B, G, K, P), ``.cpu()``, a host assignment (scipy's ``linear_sum_assignment`` if importable, else the brute force of
tests/match_reference.py), a gather and the autograd backward.  Its loss, assignment and gradient are checked against the op's before
anything is timed.  The two per-pixel launches are also timed alone (through the C entries) for their achieved fraction of 8 TB/s on the
algorithmic bytes: overlap reads 4 B K P (masks) + B G P (gt), backward reads 5 P per matched slot and writes 4 B K P.
The step: ``dsprites_arch`` at batch 32, ``model(x, attach_state=True)`` + backward, with and without ``+ matched_mask_loss(model.mask,
gt)``, alternating, median of ``step-reps`` samples of one step.  Prints one JSON line; ``--md`` writes profiles/mask_match_timing.md."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from iodine_amd import _lib, matching                                  # noqa: E402

SHAPES = ((32, 7, 6, 128), (32, 6, 4, 64))
PEAK_BPS = 8e12


def planted(B, K, G, S, seed):
    """gt: a random partition into G regions plus background; mask = softmax_K(randn + 2 gt_i) with object i on slot i % K"""
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, G + 1, (B, S, S), generator=g)
    gt = torch.stack([(label == i) for i in range(G)], 1)
    logits = torch.randn(B, K, S, S, generator=g)
    for i in range(G):
        logits[:, i % K] += 2.0 * gt[:, i].float()
    return torch.softmax(logits, 1).unsqueeze(2).contiguous(), gt.to(torch.uint8).contiguous()


def host_assign(cost, valid):
    """(G, K) float64 cost, valid rows -> assignment list"""
    rows = [g for g in range(cost.shape[0]) if valid[g]]
    out = [-1] * cost.shape[0]
    if not rows:
        return out
    try:
        from scipy.optimize import linear_sum_assignment
        r, c = linear_sum_assignment(cost[rows])
        for i, k in zip(r, c):
            out[rows[i]] = int(k)
        return out
    except ImportError:
        import match_reference
        return match_reference.brute_force(cost, valid)[0]


def eager_loss(mask, gt, loss='ce', match='iou', eps=1e-6):
    """the composite: statistics with ATen, the assignment on the host, gather, mean; autograd does the backward"""
    m, t = mask[:, :, 0], gt.float()
    inter = torch.einsum('bgyx,bkyx->bgk', t, m)
    n = t.sum((-1, -2))
    safe = n.clamp_min(1.0)[..., None]
    values = {'iou': lambda: 1.0 - inter / (safe + m.sum((-1, -2))[:, None, :] - inter),
              'ce': lambda: -torch.einsum('bgyx,bkyx->bgk', t, torch.log(m + eps)) / safe}
    L = values[loss]()
    cost = (L if match == loss else values[match]()).detach().double().cpu().numpy()      # the synchronise
    valid = (n > 0).cpu().numpy()
    asg = torch.tensor([host_assign(cost[b], valid[b]) for b in range(cost.shape[0])], device=mask.device)
    on = (asg >= 0).to(L.dtype)
    picked = torch.gather(L, 2, asg.clamp_min(0)[..., None])[..., 0] * on
    return (picked.sum(-1) / on.sum(-1).clamp_min(1.0)).mean(), asg


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(runs, reps, inner, warmup):
    times = {k: [] for k in runs}
    for r in range(warmup + reps):
        for k, fn in runs.items():
            t = timed(fn, inner)
            if r >= warmup:
                times[k].append(t)
    return times


def med(v):
    return sorted(v)[len(v) // 2]


def measure(B, K, G, S, reps, inner, warmup, dev):
    mask, gt = planted(B, K, G, S, seed=7)
    mask, gt = mask.to(dev), gt.to(dev)

    def op(i):
        m = mask.detach().requires_grad_(True)
        out = matching.matched_mask_loss(m, gt)
        out.backward()
        return out, m.grad

    def eager(i):
        m = mask.detach().requires_grad_(True)
        out, asg = eager_loss(m, gt)
        out.backward()
        return out, m.grad, asg
    # the yardstick computes the same thing
    o, og = op(0)
    e, eg, easg = eager(0)
    assert torch.equal(o.assign.long(), easg), 'assignments differ'
    rel_loss = abs(float(o) - float(e)) / abs(float(e))
    rel_grad = float((og - eg).abs().max() / eg.abs().max())
    assert rel_loss < 1e-4 and rel_grad < 1e-3, f'eager composite and op disagree: loss {rel_loss}, gradient {rel_grad}'
    times = alternate({'op': op, 'eager': eager}, reps, inner, warmup)
    # the two per-pixel launches alone
    L, P = _lib.lib(), S * S
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    stats = matching._overlap(mask, gt, B, K, G, S, 1e-6, True)
    asg, _, coef, _, _ = matching._match(stats, B, K, G, 0, 1, False)
    gl = torch.full((B,), 1.0 / B, device=dev)
    grad = torch.empty_like(mask)
    inter, nl, area, n = stats
    launches = {
        'overlap': lambda i: L.iodine_mask_overlap(st, _lib.ptr(mask), _lib.ptr(gt), B, K, G, S, 1e-6, _lib.ptr(inter), _lib.ptr(nl),
                                                   _lib.ptr(area), _lib.ptr(n)),
        'match': lambda i: L.iodine_mask_match(st, _lib.ptr(inter), _lib.ptr(nl), _lib.ptr(area), _lib.ptr(n), B, K, G, 0, 1, _lib.ptr(asg),
                                               _lib.ptr(gl.new_empty(B)), _lib.ptr(coef), None, None),
        'backward': lambda i: L.iodine_mask_match_backward(st, _lib.ptr(mask), _lib.ptr(gt), _lib.ptr(asg), _lib.ptr(coef), _lib.ptr(gl), B, K,
                                                           G, S, 1, 1e-6, _lib.ptr(grad))}
    lt = alternate(launches, reps, inner, warmup)
    matched = int((asg >= 0).sum())
    nbytes = {'overlap': 4 * B * K * P + B * G * P, 'backward': 4 * B * K * P + 5 * matched * P}
    out = dict(shape=[B, K, G, S], rel_loss_vs_eager=rel_loss, rel_grad_vs_eager=rel_grad,
               speedup_median=round(med(times['eager']) / med(times['op']), 2))
    for k, v in list(times.items()) + [(k + '_launch', v) for k, v in lt.items()]:
        out[k + '_ms_median'], out[k + '_ms_min'], out[k + '_ms_max'] = round(med(v), 5), round(min(v), 5), round(max(v), 5)
    for k, nb in nbytes.items():
        out[k + '_algorithmic_bytes'] = nb
        out[k + '_fraction_of_8TBps'] = round(nb / (med(lt[k]) * 1e-3) / PEAK_BPS, 4)
    return out


def step_time(reps, warmup, dev, batch=32):
    from iodine_amd import IODINE, synth
    from iodine_amd.model import dsprites_arch
    arch = dsprites_arch()
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    model.train()
    imgs, masks = synth.make_images(batch, arch.IMG_SIZE, seed=3, kind='blobs')
    x = torch.from_numpy(imgs).to(dev)
    gt = matching.pack_gt(masks, arch.IMG_SIZE, dev)

    def plain(i):
        model.zero_grad(set_to_none=True)
        model(x, attach_state=True).mean().backward()

    def with_term(i):
        model.zero_grad(set_to_none=True)
        loss = model(x, attach_state=True).mean()
        (loss + matching.matched_mask_loss(model.mask, gt)).backward()
    times = alternate({'attach_state': plain, 'with_mask_term': with_term}, reps, 1, warmup)
    out = dict(config='dsprites', batch=batch, slots=int(model.K), size=int(arch.IMG_SIZE), gt_rows=int(gt.shape[1]))
    for k, v in times.items():
        out[k + '_ms_median'], out[k + '_ms_min'], out[k + '_ms_max'] = round(med(v), 4), round(min(v), 4), round(max(v), 4)
    out['added_ms_median'] = round(med(times['with_mask_term']) - med(times['attach_state']), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step-reps', type=int, default=20)
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mask_match_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = [measure(B, K, G, S, args.reps, args.inner, args.warmup, dev) for B, K, G, S in SHAPES]
    step = step_time(args.step_reps, args.warmup, dev)
    try:
        import scipy  # noqa: F401
        solver = 'scipy.optimize.linear_sum_assignment'
    except ImportError:
        solver = 'brute force (tests/match_reference.py)'
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, inner=args.inner, warmup=args.warmup, step_reps=args.step_reps,
               eager_host_solver=solver, rows=rows, step=step)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        fmt = lambda r, k: '{:.4f} ({:.4f} .. {:.4f})'.format(r[k + '_ms_median'], r[k + '_ms_min'], r[k + '_ms_max'])
        with open(args.md, 'w') as f:
            f.write('# matched_mask_loss: three launches against the eager composite\n\n')
            f.write(f'`python tools/mask_match_time.py --reps {args.reps} --inner {args.inner} --warmup {args.warmup} --step-reps {args.step_reps}` on '
                    f'one MI355X (the name torch reports is "{out["device"]}").  ms per call: median (min .. max) of {args.reps} samples of '
                    f'{args.inner} back-to-back calls, HIP events, the contenders alternating, every shape warmed.  "op" is forward + backward of '
                    '`matched_mask_loss(mask, gt)` (loss `ce`, match `iou`); "eager" is the composite - einsum statistics, `.cpu()`, '
                    f'{solver} on the host, gather, autograd backward - whose loss, assignment and gradient matched the op\'s before timing '
                    '(relative differences in the table).  The inputs are one planted set per shape, re-read by every call: cache-resident '
                    '("hot"); a cold-cache figure was not measured.\n\n')
            f.write('| (B, K, G, S) | op ms | eager ms | eager / op | loss rel. diff | gradient rel. diff |\n|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| ({}, {}, {}, {}) | {} | {} | {:.1f} | {:.1e} | {:.1e} |\n'.format(
                    *r['shape'], fmt(r, 'op'), fmt(r, 'eager'), r['speedup_median'], r['rel_loss_vs_eager'], r['rel_grad_vs_eager']))
            f.write('\nThe launches alone, through the C entries (same sampling).  Algorithmic bytes: overlap reads 4 B K P of masks and B G P of '
                    'ground truth; backward reads 5 P (mask plane and ground-truth plane) per matched slot and writes 4 B K P.  The '
                    'fraction is those bytes over the median time over 8 TB/s; at these sizes a launch is a few microseconds, so launch '
                    'overhead is a large part of the time and the inputs are cache-resident.\n\n')
            f.write('| (B, K, G, S) | overlap ms | MB | fraction of 8 TB/s | match ms | backward ms | MB | fraction of 8 TB/s |\n|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| ({}, {}, {}, {}) | {} | {:.2f} | {:.3f} | {} | {} | {:.2f} | {:.3f} |\n'.format(
                    *r['shape'], fmt(r, 'overlap_launch'), r['overlap_algorithmic_bytes'] / 1e6, r['overlap_fraction_of_8TBps'],
                    fmt(r, 'match_launch'), fmt(r, 'backward_launch'), r['backward_algorithmic_bytes'] / 1e6, r['backward_fraction_of_8TBps']))
            f.write('\nTraining step, `dsprites_arch` at batch {batch} (K = {slots}, S = {size}, {gt_rows} ground-truth rows): forward with '
                    '`attach_state=True` + backward, with and without `+ matched_mask_loss(model.mask, gt)`, alternating, median (min .. max) of '
                    '{n} samples of one step.  The difference holds the three launches, the Python around them and what the model\'s backward does '
                    'with a cotangent on `mask` (`iodine_train_backward_aux`); the parts were not separated.\n\n'.format(n=args.step_reps, **step))
            f.write('| step | ms |\n|---|---|\n| attach_state=True | {} |\n| + mask term | {} |\n| added (medians) | {:.4f} |\n'.format(
                fmt(step, 'attach_state'), fmt(step, 'with_mask_term'), step['added_ms_median']))
            f.write('\nNot measured: cold-cache inputs, other cost kinds than `ce` / `iou` above, the CLEVR-size training step, several GPUs.\n')


if __name__ == '__main__':
    main()
