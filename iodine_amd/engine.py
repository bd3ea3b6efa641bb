"""Reference-shaped training / evaluation loops around the HIP module (the callers either side of the hot path,
SURVEY.md section 8f): `lib/engine/train.py:44-108`, `lib/engine/eval.py:14-28`, with one process per GPU instead of
`torch.nn.DataParallel` (`lib/modeling/build.py:11-12`).

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m iodine_amd.engine --steps 200

runs on synthetic blob scenes (there are no datasets on the box); `--clevr DIR` / `--dsprites DIR` read the reference's
dataset layouts through `iodine_amd.data`.
"""
import argparse
import os
import time

import torch

from . import parallel, synth
from .ari import ARIEvaluator
from .checkpoint import load_checkpoint, save_checkpoint
from .optim import FusedAdam, _check_max_norm, clip_grad_norm_, make_optimizer


class SyntheticScenes(torch.utils.data.Dataset):
    """Deterministic blob scenes with ground-truth masks (image index = seed), same item format as lib/data/clevr.py."""

    def __init__(self, n, img_size, seed=0):
        self.n, self.s, self.seed = n, img_size, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        imgs, masks = synth.make_images(1, self.s, seed=self.seed + i, kind='blobs')
        return torch.from_numpy(imgs[0]), torch.from_numpy(masks[0].astype('float32'))


def beta_warmup(step, beta, warmup_steps):
    """KL weight of training step ``step`` (counted from 0) under ``--beta-warmup``: a linear ramp from 0 at step 0 to ``beta`` at step
    ``warmup_steps``, ``beta`` from there on; ``warmup_steps`` <= 0: ``beta`` throughout."""
    if warmup_steps <= 0 or step >= warmup_steps:
        return float(beta)
    return float(beta) * step / warmup_steps


def train(model, optimizer, dataloader, device, max_steps, print_every=10, checkpoint_path=None, log=print, max_grad_norm=None,
          beta=None, beta_warmup_steps=0):
    """train.py:44-108: loss = model(data); loss.mean(); zero_grad; backward; [all-reduce]; [clip]; step.  Returns the losses.
    ``max_grad_norm``: the global gradient norm is clipped at this value (train.py:64, commented out in the reference; the paper
    uses 5.0) AFTER the all-reduce, so every rank clips the same averaged gradient with the same coefficient - what
    ``clip_grad_norm_`` after DataParallel's reduce would do - and the replicas stay bitwise identical.  A ``FusedAdam`` takes it
    as its ``max_grad_norm`` (fused into the step, kept on the optimizer afterwards); in front of any other optimizer
    ``iodine_amd.optim.clip_grad_norm_`` runs.  The log line gains ``grad-norm`` (one ``.item()`` per ``print_every`` steps).
    ``beta`` / ``beta_warmup_steps``: with ``beta`` given, ``model.beta`` is set before every step to ``beta_warmup(step, beta,
    beta_warmup_steps)`` and is left at ``beta`` afterwards; None leaves ``model.beta`` alone."""
    model.train()
    fused_clip = isinstance(optimizer, FusedAdam)
    if max_grad_norm is not None:
        max_grad_norm = _check_max_norm(max_grad_norm, 'max_grad_norm')
        if fused_clip:
            optimizer.max_grad_norm = max_grad_norm
    clipping = max_grad_norm is not None or (fused_clip and optimizer.max_grad_norm is not None)
    world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    losses, step, epoch = [], 0, 0
    while step < max_steps:
        sampler = getattr(dataloader, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)                                         # a new shuffle per pass over the data
        epoch += 1
        for data in dataloader:
            start = time.perf_counter()
            x = data[0].to(device, non_blocking=True)                        # "first one is image" (train.py:49)
            if beta is not None:
                model.beta = beta_warmup(step, beta, beta_warmup_steps)
            loss = model(x).mean()
            optimizer.zero_grad()
            loss.backward()
            if world > 1:
                parallel.allreduce_gradients(model.parameters())            # replaces DataParallel's reduce
            if clipping and not fused_clip:
                grad_norm = clip_grad_norm_(model.parameters(), max_grad_norm)
            optimizer.step()
            if clipping and fused_clip:
                grad_norm = optimizer.last_grad_norm
            losses.append(loss.item())
            step += 1
            if step % print_every == 0:
                log('iter: {}, loss: {:.4f}, batch-time: {:.4f}s, lr: {}{}'.format(
                    step, losses[-1], time.perf_counter() - start, optimizer.param_groups[0]['lr'],
                    ', grad-norm: {:.4f}'.format(grad_norm.item()) if clipping else ''))
            if step >= max_steps:
                break
    if beta is not None:
        model.beta = float(beta)
    if checkpoint_path and (not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0):
        save_checkpoint(checkpoint_path, model, optimizer, epoch=0, iteration=step)
    return losses


def evaluate(model, dataloader, device, evaluator=None, slots=None, iters=None):
    """eval.py:14-28 with the ARI evaluator of lib/eval/ari_eval.py (works under no_grad, unlike the reference).  With
    several ranks every rank evaluates its shard; the samples DistributedSampler appended to pad the shards to equal length
    are dropped (they duplicate the first images) and ``evaluator.global_mean`` holds the ARI over the whole dataset.
    ``slots`` / ``iters``: evaluate at that K / T (``model.K`` / ``model.n_iters`` for the duration of the call, restored afterwards;
    e.g. weights trained at K = 7, T = 5 evaluated at K = 11) - the ARI tables take K from the masks."""
    saved = (model.K, model.n_iters)
    if slots is not None:
        model.K = slots
    if iters is not None:
        model.n_iters = iters
    try:
        return _evaluate(model, dataloader, device, evaluator)
    finally:
        model.K, model.n_iters = saved


def _evaluate(model, dataloader, device, evaluator):
    evaluator = evaluator or ARIEvaluator()
    evaluator.reset()
    model.eval()
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    world = torch.distributed.get_world_size() if dist_on else 1
    rank = torch.distributed.get_rank() if dist_on else 0
    n_total = len(dataloader.dataset)
    mine = len(range(rank, n_total, world)) if world > 1 else n_total       # un-padded share of this rank (sampler stride = world)
    with torch.no_grad():
        for image, masks in dataloader:
            evaluator.evaluate(model, (image.to(device), [m.numpy() for m in masks]))
    del evaluator.aris[mine:]
    stats = torch.tensor([float(sum(evaluator.aris)), float(len(evaluator.aris))], dtype=torch.float64,
                         device=device if dist_on and torch.distributed.get_backend() == 'nccl' else 'cpu')
    if world > 1:
        torch.distributed.all_reduce(stats)
    evaluator.global_mean = float(stats[0] / stats[1]) if float(stats[1]) > 0 else 0.0
    return evaluator


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', choices=['clevr6', 'dsprites'], default='dsprites')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--batch', type=int, default=8, help='images per GPU')
    ap.add_argument('--lr', type=float, default=3e-4)                        # configs/clevr6_prop.yaml:19
    ap.add_argument('--clip', type=float, default=None, metavar='FLOAT',
                    help='clip the global gradient norm at this value (train.py:64; the paper uses 5.0)')
    ap.add_argument('--clevr'); ap.add_argument('--dsprites')
    ap.add_argument('--resume'); ap.add_argument('--save')
    ap.add_argument('--gen-conv-precision', type=int, choices=[0, 1], default=0,
                    help='generic decoder convs C -> C (KERNEL_SIZE 5 / 7, other channel counts): 0 = exact fp32 MFMA, '
                         '1 = split-fp16 (3 x f16 MFMA, fp32-class accuracy) forward and data gradient')
    ap.add_argument('--sigma', type=float, default=None, metavar='FLOAT',
                    help='likelihood scale (model.sigma); default: ARCH.SIGMA of the config')
    ap.add_argument('--beta', type=float, default=1.0, metavar='FLOAT', help='weight of the KL term (model.beta)')
    ap.add_argument('--beta-warmup', type=int, default=0, metavar='STEPS',
                    help='ramp the KL weight linearly from 0 to --beta over the first STEPS training steps')
    ap.add_argument('--iter-weights', choices=['linspace', 'uniform', 'last'], default='linspace',
                    help='per-iteration loss weights (model.iter_weights): (i+1)/(T+1), 1/(T+1) each, or the final ELBO only')
    return ap


def main(argv=None):
    from . import IODINE
    from .data import CLEVR, MultiDSprites, make_dataloader
    from .model import clevr6_arch, dsprites_arch
    args = make_parser().parse_args(argv)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank, local = int(os.environ.get('RANK', '0')), int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        torch.distributed.init_process_group('nccl', rank=rank, world_size=world)    # RCCL on ROCm
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    arch = clevr6_arch() if args.config == 'clevr6' else dsprites_arch()
    torch.manual_seed(0)                                                     # same initial replica on every rank
    model = IODINE(arch).to(device)
    model.manual_seed(1000 + rank)                                           # ... but its own reparameterisation noise
    if args.gen_conv_precision:
        model.set_option('gen_conv_precision', args.gen_conv_precision)
    if args.sigma is not None:
        model.sigma = args.sigma
    model.beta, model.iter_weights = args.beta, args.iter_weights
    optimizer = make_optimizer(model, base_lr=args.lr, max_grad_norm=args.clip)
    if args.resume:
        load_checkpoint(args.resume, model, optimizer)
    if args.clevr:
        ds = CLEVR(args.clevr)
    elif args.dsprites:
        ds = MultiDSprites(args.dsprites)
    else:
        ds = SyntheticScenes(args.batch * world * 8, arch.IMG_SIZE)
    dl = make_dataloader(ds, args.batch, shuffle=True, rank=rank, world_size=world)
    losses = train(model, optimizer, dl, device, args.steps, checkpoint_path=args.save,
                   log=print if rank == 0 else (lambda *a: None), beta=args.beta, beta_warmup_steps=args.beta_warmup)
    ev = evaluate(model, make_dataloader(ds, args.batch, shuffle=False, rank=rank, world_size=world), device)
    if rank == 0:
        print('first loss {:.2f} -> last loss {:.2f}; Ari over all ranks: {}'.format(losses[0], losses[-1], ev.global_mean))


if __name__ == '__main__':
    main()
