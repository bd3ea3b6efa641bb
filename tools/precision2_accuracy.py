"""What conv_precision 2 costs in accuracy: the device and the CPU emulation of the mode (tests/f16x1_reference.py), each against the fp64
oracle, on three committed goldens.

    python tools/precision2_accuracy.py [--cache DIR] [--cpu-only] [--md FILE.md]

Per golden: the worst relative ELBO deviation over the evaluations of ``reconstruct``, the largest absolute deviation of ``pred``, the
arg-max mask agreement, the relative deviation of the training loss and the worst per-tensor ``rel_l2`` of the parameter gradients
(``grad_views``: without the mask-logit bias, whose gradient is zero up to rounding).  The oracle runs in fp64 on the CPU, which takes a
while at 64 x 64: ``--cache DIR`` keeps its results (and the emulation's) in DIR, ``--cpu-only`` stops after filling it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import f16x1_reference as R                                              # noqa: E402
from oracle import iodine_oracle as O                                    # noqa: E402
from util import golden_setup, grad_views, load_golden, make_hip_model, rel_l2   # noqa: E402

GOLDENS = ('tiny', 'cfg1_dsprites_k4_t3_b4', 'cfg2_dsprites_k6_t5_b2')
KEEP = ('elbos', 'pred', 'mask')


def cpu_side(name, cache):
    path = os.path.join(cache, f'precision2_{name}.pt') if cache else None
    if path and os.path.exists(path):
        return torch.load(path)
    arch, params, x, eps, _ = golden_setup(load_golden(name), torch.float64)
    res = {}
    for tag, wrap in (('f64', lambda f: f), ('emu', R.emulated)):
        rec = wrap(O.reconstruct)(x, eps, params, arch)
        out, grads = wrap(O.train_step_grads)(x, eps, params, arch)
        res[tag] = dict({k: rec[k] for k in KEEP}, loss=out['loss'], grads=grads)
    if path:
        os.makedirs(cache, exist_ok=True)
        torch.save(res, path)
    return res


def row(got, ref):
    """got / ref: dicts with elbos, pred, mask, loss, grads"""
    elbo = ((got['elbos'].double() - ref['elbos']).abs() / ref['elbos'].abs()).max().item()
    pred = (got['pred'].double() - ref['pred']).abs().max().item()
    agree = (got['mask'][:, :, 0].argmax(1) == ref['mask'][:, :, 0].argmax(1)).double().mean().item()
    loss = abs(float(got['loss']) - float(ref['loss'])) / abs(float(ref['loss']))
    worst = max((rel_l2(*grad_views(n, np.asarray(got['grads'][n]), np.asarray(ref['grads'][n]))), n) for n in ref['grads'])
    return elbo, pred, agree, loss, worst


def device_side(name, precision):
    arch, params, x, eps, _ = golden_setup(load_golden(name))
    m = make_hip_model(arch, params, options={'conv_precision': precision})
    pred, mask, _ = m.reconstruct(x.cuda(), eps.cuda())
    got = dict(pred=pred.cpu(), mask=mask.cpu(), elbos=m.elbo_terms[:, 0].cpu())
    m.zero_grad(set_to_none=True)
    loss = m(x.cuda(), eps.cuda())
    loss.backward()
    got.update(loss=loss.item(), grads={n: p.grad.cpu() for n, p in m.named_parameters()})
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cache')
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--md')
    args = ap.parse_args()
    lines = ['| golden | what | ELBO, worst evaluation (rel) | `pred` max abs | arg-max mask agreement | training loss (rel) | worst parameter gradient (`rel_l2`) |',
             '|---|---|---|---|---|---|---|']
    for name in GOLDENS:
        cpu = cpu_side(name, args.cache)
        rows = [('CPU emulation', row(cpu['emu'], cpu['f64']))]
        if not args.cpu_only:
            if not torch.cuda.is_available():
                raise SystemExit('precision2_accuracy.py: no ROCm device (use --cpu-only for the emulation alone)')
            rows.append(('device, conv_precision 2', row(device_side(name, 2), cpu['f64'])))
            rows.append(('device, conv_precision 1', row(device_side(name, 1), cpu['f64'])))
        for what, (elbo, pred, agree, loss, worst) in rows:
            lines.append(f'| `{name}` | {what} | {elbo:.1e} | {pred:.1e} | {100 * agree:.3f} % | {loss:.1e} | {worst[0]:.1e} ({worst[1]}) |')
            print(lines[-1], flush=True)
    if args.md:
        with open(args.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
