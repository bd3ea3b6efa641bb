"""Rank of tests/test_gpu_clip.py: a few steps of iodine_amd.engine.train with max_grad_norm on this rank's own images.  The norm
is taken after the all-reduce (lib/engine/train.py:64 after DataParallel's reduce), so every rank clips the same averaged gradient
with the same coefficient: the replicas stay bitwise identical and every rank reports the same last_grad_norm bits."""
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from iodine_amd import engine, parallel  # noqa: E402
from iodine_amd.optim import make_optimizer  # noqa: E402
from util import golden_setup, load_golden, make_hip_model  # noqa: E402

rank, world, local = int(os.environ['RANK']), int(os.environ['WORLD_SIZE']), int(os.environ['LOCAL_RANK'])
share = os.environ.get('IODINE_BENCH_SHARE_DEVICE') == '1'        # 1-GPU box: both ranks on device 0, collectives over gloo
dev = torch.device('cuda', 0 if share else local)
torch.cuda.set_device(dev)
if share:
    dist.init_process_group('gloo', rank=rank, world_size=world)
else:
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

g = load_golden('tiny')
arch, params, x, eps, _ = golden_setup(g)
m = make_hip_model(arch, params, dev)
m.manual_seed(1000 + rank)                                        # every rank its own noise ...
before = parallel.replicas_identical(m.parameters())
STEPS, MAX_NORM = 4, 1.0
opt = make_optimizer(m, base_lr=3e-4)
lines, norms = [], []
for s in range(STEPS):                                            # ... and its own images
    engine.train(m, opt, [(x + 0.01 * (rank + 1) * s,)], dev, 1, print_every=1, log=lines.append, max_grad_norm=MAX_NORM)
    norms.append(opt.last_grad_norm.clone())
after = parallel.replicas_identical(m.parameters())
mine = torch.stack(norms).view(torch.int32)
gathered = [torch.zeros_like(mine) for _ in range(world)]
dist.all_gather(gathered, mine)
if rank == 0:
    print(json.dumps(dict(world=world, backend=dist.get_backend(), steps=len(norms), replicas_identical_before=before,
                          replicas_identical_after=after, same_norm_bits=all(torch.equal(gathered[0], t) for t in gathered),
                          clipped_every_step=all(float(n) > MAX_NORM for n in norms),
                          logged_grad_norm=len(lines) == STEPS and all('grad-norm: ' in ln for ln in lines),
                          norms=[float(n) for n in norms])), flush=True)
dist.barrier()
dist.destroy_process_group()
