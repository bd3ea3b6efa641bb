"""A/B of option gen_conv_precision (0 = fp32 MFMA generic convs, 1 = split-fp16 forward / data gradient / weight gradient, kernels_gensplit.hip) in ONE
process on one device, the two settings alternating on the same model so that the drift between equal settings is visible:

    python tools/gen_split_ab.py [--rounds 3] [--steps 3] [--only default5|testyaml]

Workloads: the reference-default decoder at CLEVR shapes (DEC.KERNEL_SIZE 5, 64 channels, 128 x 128, K 7, T 5, batch 4: bench.py's
default_dec_kernel5 side figure) and the configs/test.yaml architecture at batch 32; training step (forward, backward, Adam) and reconstruct.
After the timed rounds one profiled step per setting (profile 2: every launch bracketed, so its total is NOT a step time) gives the time
per category; the fp32 time of the layers that option 1 moves is gen_conv(0) - gen_conv(1) (what stays in gen_conv under option 1: the output
conv and a generic refinement stack).  Prints one JSON line per workload.  `--once 0|1` runs a few steps of one setting only (for rocprofv3)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iodine_amd import IODINE, synth  # noqa: E402
from iodine_amd.model import arch_namespace  # noqa: E402
from iodine_amd.optim import make_optimizer  # noqa: E402

PEAK_F16_MFMA_TFLOPS = 2500.0          # MI355X dense fp16 matrix peak; the split roof is a third of it (as bench.py defines it)


def workloads():
    return {
        'default5': dict(arch=arch_namespace(64, 5, 7, 128, (64, 4, 256), (64, 4), kernels=(3, 5)), batch=4, S=128, C=64, k=5, layers=3, K=7, T=5),
        'testyaml': dict(arch=arch_namespace(16, 5, 6, 64, (32, 3, 128), (32, 5), sigma=0.14, kernels=(5, 5),
                                             encoding=['posterior', 'grad_post', 'image', 'leave_one_out_likelihood']),
                         batch=32, S=64, C=32, k=5, layers=4, K=6, T=5),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--once', type=int, default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    for name, wl in workloads().items():
        if args.only and name != args.only:
            continue
        m = IODINE(wl['arch'])
        sh = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(sh, seed=0).items()})
        m = m.to(dev)
        m.manual_seed(7)
        x = torch.from_numpy(synth.make_images(wl['batch'], wl['S'], seed=0)).to(dev)
        opt = make_optimizer(m, base_lr=3e-4, weight_decay=0.0)

        def train():
            loss = m(x)
            m.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        def infer():
            m.reconstruct(x)

        def timed(fn, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        if args.once is not None:
            m.set_option('gen_conv_precision', args.once)
            for fn in (train, infer):
                fn()
                timed(fn, args.steps)
            continue
        res = {f'{md}_ms_opt{o}': [] for md in ('train', 'infer') for o in (0, 1)}
        for o in (0, 1):                                                   # warm-up of both settings (attribute calls, allocator)
            m.set_option('gen_conv_precision', o)
            train(); infer()
        for _ in range(args.rounds):
            for o in (0, 1):
                m.set_option('gen_conv_precision', o)
                train(); infer()                                           # re-sent parameters, packs
                res[f'train_ms_opt{o}'].append(round(timed(train, args.steps), 3))
                res[f'infer_ms_opt{o}'].append(round(timed(infer, args.steps), 3))
        cats = {}
        for o in (0, 1):
            m.set_option('gen_conv_precision', o)
            train()
            m.set_option('profile', 2)
            for c in ('gen_conv', 'gen_conv_f16x3', 'gen_l0'):
                m.profile_read(c)
            train()
            torch.cuda.synchronize()
            m.set_option('profile', 0)
            cats[o] = {c: dict(zip(('ms', 'launches'), (round(v, 3) if i == 0 else v for i, v in enumerate(m.profile_read(c)))))
                       for c in ('gen_conv', 'gen_conv_f16x3', 'gen_l0')}
        f32_ms = cats[0]['gen_conv']['ms'] - cats[1]['gen_conv']['ms']
        split_ms = cats[1]['gen_conv_f16x3']['ms']
        n_launch = cats[1]['gen_conv_f16x3']['launches']
        N = wl['batch'] * wl['K']
        flop = 2.0 * N * wl['S'] ** 2 * wl['C'] ** 2 * wl['k'] ** 2 * n_launch
        out = dict(workload=name, batch=wl['batch'], **res,
                   train_median=dict(opt0=statistics.median(res['train_ms_opt0']), opt1=statistics.median(res['train_ms_opt1'])),
                   infer_median=dict(opt0=statistics.median(res['infer_ms_opt0']), opt1=statistics.median(res['infer_ms_opt1'])),
                   train_spread_opt0=round(max(res['train_ms_opt0']) - min(res['train_ms_opt0']), 3),
                   profiled_training_step=cats, moved_layers_ms=dict(fp32=round(f32_ms, 3), split=round(split_ms, 3), launches=n_launch,
                                                                     ratio=round(f32_ms / split_ms, 2) if split_ms else None),
                   split_tflops=round(flop / (split_ms * 1e-3) / 1e12, 1) if split_ms else None,
                   fraction_of_split_roof=round(flop / (split_ms * 1e-3) / 1e12 / (PEAK_F16_MFMA_TFLOPS / 3), 3) if split_ms else None)
        print(json.dumps(out), flush=True)
        del m, opt, x
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
