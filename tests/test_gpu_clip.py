"""Global-norm gradient clipping fused into the Adam step (lib/engine/train.py:64, the line the reference carries commented out):
grad_sumsq_multi_kernel + grad_clip_finalize_kernel, adam_multi_kernel<CLIP>, grad_scale_multi_kernel and their Python surface
against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import iodine_oracle as O
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM_SHAPES = [(64, 17, 3, 3), (64,), (1024, 512), (7,), (4, 64, 3, 3)]         # tests/test_gpu_extras.py, test_fused_adam_matches_torch_adam
ULP = 2.0 ** -23                                                                # fp32: 1.19e-7 relative


def _clevr_shapes():
    from iodine_amd import IODINE
    from iodine_amd.model import clevr6_arch
    return [tuple(p.shape) for p in IODINE(clevr6_arch()).parameters()]


def _norm_out4(grads, max_norm):
    """(out4 as a CPU tensor) of iodine_grad_norm over device gradients, through the optimizer's own buffer class"""
    from iodine_amd.optim import _GradNorm
    gn = _GradNorm()
    ptrs, offs, total = gn.table(grads)
    gn.norm(ptrs, offs, len(grads), total, float(max_norm), grads[0].device)
    return gn.out4.cpu()


def _layouts(cpu_grads, seed):
    """the same gradients (a) as views of ONE flat device buffer, back to back - what IODINE.backward produces - and (b) as
    separately allocated tensors handed over in shuffled order"""
    flat = torch.cat([g.reshape(-1) for g in cpu_grads]).to(DEV)
    views, off = [], 0
    for g in cpu_grads:
        views.append(flat[off:off + g.numel()].view(g.shape))
        off += g.numel()
    order = np.random.default_rng(seed).permutation(len(cpu_grads))
    separate = [cpu_grads[i].clone().to(DEV) for i in order]
    return {'flat_views': views, 'separate_shuffled': separate}


@pytest.mark.parametrize('scale', [1e-4, 1e-2, 1.0, 1e3])
@pytest.mark.parametrize('shapes', ['adam_test', 'clevr6'])
def test_norm_and_coefficient_match_fp64(shapes, scale):
    """total_norm against torch.linalg.vector_norm of the concatenated fp64 gradients on the CPU.  The kernels accumulate in fp64,
    so the only fp32 roundings are the square root's result and its cast: bound 2 fp32 ulps = 2.4e-7 relative (derived, not
    tuned); the coefficient adds one fp32 add and one fp32 divide: 4 ulps."""
    g = torch.Generator().manual_seed(11)
    grads = [torch.randn(s, generator=g) * scale for s in (ADAM_SHAPES if shapes == 'adam_test' else _clevr_shapes())]
    ref = float(torch.linalg.vector_norm(torch.cat([x.double().reshape(-1) for x in grads])))
    for max_norm in (5.0, ref / 3.0, float('inf')):
        ref_coef = min(1.0, max_norm / (ref + 1e-6))
        for name, dev_grads in _layouts(grads, seed=5).items():
            out = _norm_out4(dev_grads, max_norm)
            e_norm, e_coef = abs(float(out[0]) - ref) / ref, abs(float(out[1]) - ref_coef) / ref_coef
            print(f'[{shapes} x{scale:g} max_norm {max_norm:g} {name}] norm {float(out[0])!r} vs {ref!r}: {e_norm:.2e}; coef {e_coef:.2e}')
            assert e_norm <= 2 * ULP, (name, max_norm, float(out[0]), ref)
            assert e_coef <= 4 * ULP, (name, max_norm, float(out[1]), ref_coef)
            assert float(out[2]) == 0.0 and float(out[3]) == 0.0
            if max_norm == float('inf'):
                assert float(out[1]) == 1.0


def test_norm_of_unaligned_and_tiny_tensors():
    """the table form for arbitrary tensors: starts that are not 16-byte aligned, sizes below one 16-byte load, any order"""
    g = torch.Generator().manual_seed(3)
    base = torch.randn(4096 + 64, generator=g).to(DEV)
    pieces = [base[1:8], base[9:10], base[11:1030], base[1031:1034], base[1037:4096 + 61]]           # odd starts and sizes
    lone = [torch.randn(n, generator=g).to(DEV) for n in (1, 2, 3, 5, 7, 4097)]
    grads = [pieces[3], lone[5], pieces[0], lone[0], pieces[4], lone[2], pieces[1], lone[4], pieces[2], lone[1], lone[3]]
    ref = float(torch.linalg.vector_norm(torch.cat([x.double().cpu().reshape(-1) for x in grads])))
    out = _norm_out4(grads, 1.0)
    assert abs(float(out[0]) - ref) / ref <= 2 * ULP
    one = _norm_out4([lone[0]], 1.0)                                             # a single element: |x|
    assert abs(float(one[0]) - abs(float(lone[0]))) <= 2 * ULP * abs(float(lone[0]))


def test_norm_is_bitwise_reproducible():
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(s, generator=g) * 3.0 for s in _clevr_shapes()]
    for dev_grads in _layouts(grads, seed=9).values():
        a = _norm_out4(dev_grads, 5.0)
        for _ in range(3):
            b = _norm_out4(dev_grads, 5.0)
            assert torch.equal(a[:2].view(torch.int32), b[:2].view(torch.int32))


def _pairs(seed=0, shapes=ADAM_SHAPES):
    g = torch.Generator().manual_seed(seed)
    ref_p = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    hip_p = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    return g, ref_p, hip_p


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_clipped_trajectory_matches_torch(wd):
    """five steps of torch.nn.utils.clip_grad_norm_(ps, 5.0) + torch.optim.Adam on the CPU against FusedAdam(max_grad_norm=5.0).
    Gradients randn * 10**(it - 4) over ~5.4e5 elements: norms ~0.07, 0.7, 7, 73, 730 - steps 0-1 do not clip, steps 2-4 do
    (asserted from the CPU reference's norms).  Bound: the project's own for the unclipped optimizer, rel_err < 2e-6
    (tests/test_gpu_extras.py:31); torch's fp32 and fp64 runs of this trajectory on the CPU end 1.2e-7 apart."""
    from iodine_amd.optim import FusedAdam
    g, ref_p, hip_p = _pairs()
    ref_opt = torch.optim.Adam(ref_p, lr=3e-4, weight_decay=wd)
    hip_opt = FusedAdam(hip_p, lr=3e-4, weight_decay=wd, max_grad_norm=5.0)
    norms = []
    for it in range(5):
        for rp, hp in zip(ref_p, hip_p):
            gr = torch.randn(rp.shape, generator=g) * (10.0 ** (it - 4))
            rp.grad = gr.clone()
            hp.grad = gr.clone().to(DEV)
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref_p, 5.0)))          # lib/engine/train.py:64
        ref_opt.step()
        hip_opt.step()
        assert (norms[-1] > 5.0) == (it >= 2), norms                             # the reference itself: which steps clip
        assert abs(float(hip_opt.last_grad_norm) - norms[-1]) <= 1e-5 * norms[-1]    # (torch's own fp32 norm is the looser side)
        worst = max(rel_err(hp.detach().cpu(), rp.detach()) for rp, hp in zip(ref_p, hip_p))
        print(f'[wd {wd}] step {it}: norm {norms[-1]:.4f}, worst parameter rel_err {worst:.2e}')
        assert worst < 2e-6, (it, worst)
    st = hip_opt.state[hip_p[0]]
    assert st['step'] == 5 and rel_err(st['exp_avg_sq'].cpu(), ref_opt.state[ref_p[0]]['exp_avg_sq']) < 1e-5
    assert float(hip_opt.skipped_steps) == 0.0


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_fused_equals_clip_then_step_bitwise(wd):
    from iodine_amd.optim import FusedAdam, clip_grad_norm_
    g, ref_p, a_p = _pairs(seed=4)
    b_p = [torch.nn.Parameter(p.detach().clone()) for p in a_p]
    fused = FusedAdam(a_p, lr=3e-4, weight_decay=wd, max_grad_norm=2.0)
    plain = FusedAdam(b_p, lr=3e-4, weight_decay=wd)
    for it in range(3):
        grads = [torch.randn(p.shape, generator=g) * (10.0 ** (it - 3)) for p in ref_p]          # norms ~0.7 (no clip), 7, 73
        for ap, bp, gr in zip(a_p, b_p, grads):
            ap.grad, bp.grad = gr.clone().to(DEV), gr.clone().to(DEV)
        fused.step()
        norm = clip_grad_norm_(b_p, 2.0)
        assert norm.device.type == 'cuda' and norm.dim() == 0
        plain.step()
        assert torch.equal(_bits(norm), _bits(fused.last_grad_norm))
        coef = fused._gradnorm.out4[1]
        assert (float(coef) < 1.0) == (it >= 1)
        for ap, bp, gr in zip(a_p, b_p, grads):
            assert torch.equal(_bits(ap), _bits(bp))
            for k in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(_bits(fused.state[ap][k]), _bits(plain.state[bp][k])), (it, k)
            assert torch.equal(_bits(ap.grad), _bits(gr.to(DEV)))                                 # the fused path does not write back
            assert torch.equal(_bits(bp.grad), _bits(gr.to(DEV) * coef))                          # the stand-alone one leaves g * coef


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_infinite_max_norm_equals_unclipped_bitwise(wd):
    """coef == 1: pins the CLIP = false arithmetic against the CLIP = true kernel and the clip-before-weight-decay order"""
    from iodine_amd.optim import FusedAdam
    g, ref_p, a_p = _pairs(seed=6)
    b_p = [torch.nn.Parameter(p.detach().clone()) for p in a_p]
    off = FusedAdam(a_p, lr=3e-4, weight_decay=wd, max_grad_norm=float('inf'))
    plain = FusedAdam(b_p, lr=3e-4, weight_decay=wd)
    for it in range(5):
        for ap, bp in zip(a_p, b_p):
            gr = torch.randn(ap.shape, generator=g) * (10.0 ** (it - 2))
            ap.grad, bp.grad = gr.clone().to(DEV), gr.clone().to(DEV)
        off.step()
        plain.step()
        assert float(off._gradnorm.out4[1]) == 1.0
        for ap, bp in zip(a_p, b_p):
            assert torch.equal(_bits(ap), _bits(bp)), it
            for k in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(_bits(off.state[ap][k]), _bits(plain.state[bp][k])), (it, k)


def test_nonfinite_norm_skip_leaves_everything_untouched():
    from iodine_amd.optim import FusedAdam
    g, ref_p, hip_p = _pairs(seed=8)
    ref_opt = torch.optim.Adam(ref_p, lr=3e-4)
    opt = FusedAdam(hip_p, lr=3e-4, max_grad_norm=5.0, nonfinite='skip')

    def set_grads(poison):
        for i, (rp, hp) in enumerate(zip(ref_p, hip_p)):
            gr = torch.randn(rp.shape, generator=g)
            rp.grad = gr.clone()
            if poison and i == 2:
                gr.view(-1)[12345] = float('inf')
            hp.grad = gr.clone().to(DEV)

    def step_ref():
        torch.nn.utils.clip_grad_norm_(ref_p, 5.0)
        ref_opt.step()

    set_grads(False); step_ref(); opt.step()                                      # a normal step first: the moments are non-zero
    before = [(p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for p in hip_p]
    set_grads(True); opt.step()                                                   # (the CPU reference does not see this step)
    assert float(opt.skipped_steps) == 1.0 and not np.isfinite(float(opt.last_grad_norm))
    for p, (p0, m0, v0) in zip(hip_p, before):
        assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(opt.state[p]['exp_avg']), _bits(m0))
        assert torch.equal(_bits(opt.state[p]['exp_avg_sq']), _bits(v0))
    assert opt.state[hip_p[0]]['step'] == 2                                       # the host cannot know: the count advances
    set_grads(False); opt.step()                                                  # the next finite step updates normally
    assert float(opt.skipped_steps) == 1.0 and np.isfinite(float(opt.last_grad_norm))
    for p, (p0, _, _) in zip(hip_p, before):
        assert not torch.equal(p.detach(), p0)
        assert torch.isfinite(p).all()
    # (the CPU reference took its finite steps as steps 1, 2; this one ran as step 3, with the bias corrections of step 3, so only
    # the size is checked: Adam moves an element by less than lr per step here)
    assert max(float((p.detach() - p0).abs().max()) for p, (p0, _, _) in zip(hip_p, before)) < 2 * 3e-4


def test_nonfinite_norm_propagates_like_torch(wd=0.0):
    """'propagate' = torch: total_norm = inf gives clip_coef = 0, the inf element becomes inf * 0 = NaN, every other gradient 0.
    (Without weight decay: the first Adam step is lr * g / (|g| + eps), a sign function of the gradient, and with
    wd * p of the size of the clipped gradient some of the 5.4e5 elements cancel to within fp32 rounding and step either way -
    a property of that construction, seen on the first, finite step, not of the non-finite handling under test.)"""
    from iodine_amd.optim import FusedAdam
    g, ref_p, hip_p = _pairs(seed=8)
    ref_opt = torch.optim.Adam(ref_p, lr=3e-4, weight_decay=wd)
    opt = FusedAdam(hip_p, lr=3e-4, weight_decay=wd, max_grad_norm=5.0)            # nonfinite='propagate' is the default
    for it in range(3):
        for i, (rp, hp) in enumerate(zip(ref_p, hip_p)):
            gr = torch.randn(rp.shape, generator=g)
            if it == 1 and i == 2:
                gr.view(-1)[12345] = float('inf')
            rp.grad, hp.grad = gr.clone(), gr.clone().to(DEV)
        torch.nn.utils.clip_grad_norm_(ref_p, 5.0)
        ref_opt.step()
        opt.step()
        for rp, hp in zip(ref_p, hip_p):
            a, b = hp.detach().cpu(), rp.detach()
            assert torch.equal(torch.isnan(a), torch.isnan(b)), it                 # NaN pattern included
            ok = ~torch.isnan(b)
            assert rel_err(a[ok], b[ok]) < 2e-6, it
    assert int(torch.isnan(ref_p[2].detach()).sum()) == 1 and float(opt.skipped_steps) == 1.0     # counted, not skipped


def test_norm_is_global_over_param_groups_and_buckets():
    """the reference's one-group-per-parameter layout (lib/solver/build.py:10-14) with two lr values: two buckets, two Adam
    launches, ONE norm over all gradients.  (No weight decay, for the reason given in test_nonfinite_norm_propagates_like_torch:
    a first Adam step on clipped gradient + wd * p of equal size is a sign function of a cancelling sum for some elements.)"""
    from iodine_amd.optim import FusedAdam, clip_grad_norm_
    g, ref_p, a_p = _pairs(seed=12)
    b_p = [torch.nn.Parameter(p.detach().clone()) for p in a_p]
    lrs = [3e-4, 1e-3, 3e-4, 1e-3, 3e-4]

    def groups(ps):
        return [{'params': [p], 'lr': lr, 'weight_decay': 0.0} for p, lr in zip(ps, lrs)]
    ref_opt = torch.optim.Adam(groups(ref_p), lr=3e-4)
    fused = FusedAdam(groups(a_p), lr=3e-4, max_grad_norm=5.0)
    plain = FusedAdam(groups(b_p), lr=3e-4)
    for it in range(3):
        grads = [torch.randn(p.shape, generator=g) * 0.1 for p in ref_p]                 # global norm ~73; the lr 1e-3 bucket alone
        for rp, ap, bp, gr in zip(ref_p, a_p, b_p, grads):                              # ((64,) + (7,)) has norm ~0.8 < 5
            rp.grad, ap.grad, bp.grad = gr.clone(), gr.clone().to(DEV), gr.clone().to(DEV)
        ref_norm = float(torch.linalg.vector_norm(torch.cat([x.double().reshape(-1) for x in grads])))
        small = float(torch.linalg.vector_norm(torch.cat([grads[1].double().reshape(-1), grads[3].double().reshape(-1)])))
        assert ref_norm > 5.0 > small
        torch.nn.utils.clip_grad_norm_(ref_p, 5.0)
        ref_opt.step()
        fused.step()
        clip_grad_norm_(b_p, 5.0)
        plain.step()
        assert len(fused._tables) == 2                                                   # two buckets
        assert abs(float(fused.last_grad_norm) - ref_norm) <= 2 * ULP * ref_norm
        for rp, ap, bp in zip(ref_p, a_p, b_p):
            assert torch.equal(_bits(ap), _bits(bp))                                     # both buckets used the global coefficient
            assert rel_err(ap.detach().cpu(), rp.detach()) < 2e-6


class _Traj(dict):
    """what util.check_trajectory_params reads of a tests/golden/traj_*.npz fixture"""
    @property
    def files(self):
        return list(self.keys())


def _clipped_oracle_run(name, dtype, max_grad_norm):
    """tests/test_oracle_golden.py:169-186 with the clip line of lib/engine/train.py:64 added"""
    from util import trajectory_setup
    tr, arch, params, x, eps = trajectory_setup(name, dtype)
    ps = {k: torch.nn.Parameter(v.clone()) for k, v in params.items()}
    opt = torch.optim.Adam(ps.values(), lr=float(tr['meta_lr']), weight_decay=0.0)
    losses, norms = [], []
    for e in eps:
        out, grads = O.train_step_grads(x, e, {k: p.detach() for k, p in ps.items()}, arch)
        opt.zero_grad()
        for k, p in ps.items():
            p.grad = grads[k].to(dtype)
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(ps.values()), max_grad_norm)))
        opt.step()
        losses.append(float(out['loss']))
    return losses, norms, ps


@pytest.fixture(scope='module')
def clipped_tiny_reference():
    _, norms0, _ = _clipped_oracle_run('traj_tiny', torch.float64, float('inf'))
    max_norm = 0.5 * norms0[0]                                  # half of the first-step norm: every step clips
    l64, n64, _ = _clipped_oracle_run('traj_tiny', torch.float64, max_norm)
    l32, n32, p32 = _clipped_oracle_run('traj_tiny', torch.float32, max_norm)
    assert all(n > max_norm for n in n64) and all(n > max_norm for n in n32), (max_norm, n64, n32)
    return max_norm, l64, n64, p32


@pytest.mark.parametrize('prec', [1, 0], ids=['split_f16x3', 'exact_fp32'])
def test_clipped_training_trajectory_on_the_model(prec, clipped_tiny_reference):
    """four training steps on the tiny golden architecture, as test_training_trajectory_matches_reference (tests/test_gpu_train.py)
    with max_grad_norm: HIP forward / backward + the clipped fused Adam against the oracle's gradients driven through
    torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU (fp64 for the losses, fp32 for the parameters).  Same measures
    and numbers as that test: losses 2e-5 of the largest loss; parameters 0.05 of lr * steps."""
    from iodine_amd.optim import make_optimizer
    from util import check_trajectory_params, make_hip_model, trajectory_setup
    max_norm, ref_losses, ref_norms, ref_params = clipped_tiny_reference
    tr, arch, params, x, eps = trajectory_setup('traj_tiny')
    m = make_hip_model(arch, params, options={'conv_precision': prec})
    opt = make_optimizer(m, base_lr=float(tr['meta_lr']), weight_decay=0.0, max_grad_norm=max_norm)
    xd, losses, norms = x.to(DEV), [], []
    for e in eps:
        loss = m(xd, e.to(DEV))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
        norms.append(float(opt.last_grad_norm))
    ref = np.array(ref_losses)
    print(f'[conv_precision {prec}] max_norm {max_norm:.4f}; norms HIP {norms} vs CPU fp64 {ref_norms}; losses {losses} vs {ref_losses}')
    assert np.abs(np.array(losses) - ref).max() <= 2e-5 * np.abs(ref).max(), (losses, ref_losses)
    assert all(n > max_norm for n in norms)
    assert np.abs(np.array(norms) - np.array(ref_norms)).max() <= 1e-3 * max(ref_norms)      # (gradient gate of tests/test_gpu_train.py)
    fake = _Traj({'meta_lr': tr['meta_lr'], 'meta_steps': tr['meta_steps']})
    for n, p in ref_params.items():
        fake['f32.param.' + n] = p.detach().numpy()
    check_trajectory_params(fake, 'f32', m.named_parameters(), 0.05)


def test_clipped_step_does_not_synchronise():
    from iodine_amd.optim import FusedAdam
    g, ref_p, hip_p = _pairs(seed=2)
    opt = FusedAdam(hip_p, lr=3e-4, weight_decay=0.01, max_grad_norm=5.0, nonfinite='skip')
    for hp in hip_p:
        hp.grad = (torch.randn(hp.shape, generator=g) * 10).to(DEV)
    opt.step()                                                   # warm-up: builds the tables, scratch and out4
    before = [p.detach().clone() for p in hip_p]
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode('error')
    except Exception as e:                                       # noqa: BLE001
        pytest.skip(f'torch.cuda.set_sync_debug_mode is not available in this build: {e}')
    try:
        try:
            torch.ones(1, device=DEV).item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            opt.step()                                           # any synchronising call in here raises
            norm, skipped = opt.last_grad_norm, opt.skipped_steps
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not detects:
        pytest.skip('sync debug mode does not flag a synchronising .item() in this ROCm build')
    assert float(norm) > 5.0 and float(skipped) == 0.0
    assert all(not torch.equal(p.detach(), b) for p, b in zip(hip_p, before))


def _last_json(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith('{')][-1])


def _check_two_ranks(out):
    assert out['world'] == 2 and out['steps'] >= 3
    assert out['replicas_identical_before'] and out['replicas_identical_after']
    assert out['same_norm_bits'] and out['clipped_every_step']
    assert out['logged_grad_norm']


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs >= 2 ROCm devices')
def test_two_ranks_clip_the_same_gradient_over_rccl():
    from iodine_amd import launch
    r = launch.spawn(os.path.join(ROOT, 'tests', 'clip_rank_worker.py'), [], 2, capture=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_json(r.stdout)
    assert out['backend'] == 'nccl'
    _check_two_ranks(out)


def test_two_ranks_sharing_one_device_clip_the_same_gradient():
    """the same with both ranks on one device and the collectives over gloo, as tests/test_gpu_multirank.py does for the 1-GPU boxes"""
    from iodine_amd import launch
    env = dict(os.environ)
    env['IODINE_BENCH_SHARE_DEVICE'] = '1'
    r = launch.spawn(os.path.join(ROOT, 'tests', 'clip_rank_worker.py'), [], 2, env=env, capture=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_json(r.stdout)
    assert out['backend'] == 'gloo'
    _check_two_ranks(out)
