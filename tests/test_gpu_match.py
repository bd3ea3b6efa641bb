"""iodine_amd.matching on the device against the float64 restatement in tests/match_reference.py: overlap statistics, the assignment,
the matched loss and its gradient, determinism, one training step end to end, the engine flag and the evaluator.

Inputs are planted (match_reference.planted): ``gt`` is a random partition, the masks a softmax of ``randn + 2 gt_i`` on a slot per object,
so the best and the second-best assignment are far apart and equality of assignments is a fair demand; every test that compares
assignments asserts that gap on the reference side first.

Tolerances, with e = 2^-24 (half an fp32 ulp, relative) and u = 1 the documented ulp bound of HIP's logf:
* ``gt_area`` is an integer count: exact.
* ``inter``, ``mask_area``: fp64 sums of exact fp32 terms (<= 2^20 terms: the fp64 error is below 2^-32 relative) rounded to fp32 once:
  e < 2^-23 relative.
* ``nll``: the term -logf(a), a = fl(m + eps) the same fp32 number on both sides, is within u ulp <= u 2^-23 relative of the exact log;
  all terms of a sum have one sign (a < 1 for every pixel of these inputs, or a > 1 for every pixel when K = 1), so the per-term bound
  carries to the sum; one rounding more: (u + 1) 2^-23 relative.
* loss 'ce' = mean_g N / n: the same relative bound plus the rounding of the result, ((u + 1) 2^-23 + e) mean|N / n|.
* loss 'iou' = mean_g 1 - I / U, U = n + a - I >= max(a, I): |dU| <= 2e (a + I) <= 4e U and |dI| <= 2e I, so |d(I / U)| <= 6e I / U; with the
  rounding of the result: 6e mean(I / U) + e loss.
* gradient, element-wise against the tensor's largest magnitude.  'ce': -gl / (M n a) is evaluated as fl(fl(gl fl(1 / (M n))) / a): three
  roundings (the division is correctly rounded by default; 2.5 ulp if it were not), bound 8e.  'iou': on = -gl / (M U) carries dU / U <= 4e
  and two roundings: 6e; off = gl I / (M U^2) carries 2e + 2 * 4e and two roundings: 12e; bound 13e with the second-order terms."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import match_reference as R
from iodine_amd import _lib, matching, synth
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E = 2.0 ** -24
U_LOGF = 1
GATE = 1e-3                                                                  # tests/test_gpu_train_aux.py: rel-L2 per parameter gradient
MIN_GAP = 1e-3

# (B, K, G, S): S = 5 scalar path (P = 25); S = 8 vector path with fewer vectors than threads; S = 68: P / 4 = 1156 vectors, one full pass
# of the 1024 threads and a partial one
SHAPES = [(1, 1, 1, 5), (3, 2, 3, 8), (3, 7, 3, 68), (1, 16, 16, 8), (3, 7, 16, 5), (3, 2, 3, 5), (1, 16, 1, 68), (3, 1, 3, 8)]
SPECIAL = {'zero_row_between': dict(shape=(3, 5, 4, 8), empty_rows=(1,)), 'image_without_objects': dict(shape=(3, 3, 3, 8), empty_images=(1,)),
           'more_objects_than_slots': dict(shape=(3, 3, 5, 8))}


def _case(shape, seed=0, **kw):
    B, K, G, S = shape
    return R.planted(B, K, G, S, seed=1000 * K + 10 * G + S + seed, **kw)


def _cases():
    out = [(f'B{b}K{k}G{g}S{s}', _case((b, k, g, s))) for b, k, g, s in SHAPES]
    out += [(name, _case(kw['shape'], **{k: v for k, v in kw.items() if k != 'shape'})) for name, kw in SPECIAL.items()]
    return out


CASES = dict(_cases())


def _misaligned(t):
    """the same values behind a base pointer offset by one element (one float for a mask, one byte for gt)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % (16 if t.dtype == torch.float32 else 4) != 0
    return out


def _close(got, ref, rel, what):
    got, ref = got.double().cpu(), ref.double()
    err = (got - ref).abs()
    bound = rel * ref.abs()
    worst = float((err / ref.abs().clamp_min(1e-300)).max()) if ref.numel() else 0.0
    print(f'[{what}] worst relative error {worst:.3e} (bound {rel:.3e})')
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


def _one_sign(mask, eps=1e-6):
    a = mask.float() + torch.tensor(eps, dtype=torch.float32)
    return bool((a < 1).all()) or bool((a > 1).all())


# ---- statistics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset_by_one'])
def test_overlap_statistics_match_float64_reference(name, aligned):
    mask, gt = CASES[name]
    assert _one_sign(mask), 'the log terms of these inputs must share a sign (see the module docstring)'
    inter, nll, area, n = R.stats(mask, gt)
    md, gd = mask.to(DEV), gt.to(DEV)
    if not aligned:
        md, gd = _misaligned(md), _misaligned(gd)
    got = matching.overlap(md, gd)
    assert torch.equal(got.gt_area.cpu().long(), n)
    _close(got.inter, inter, 2.0 ** -23, f'{name} inter')
    _close(got.mask_area, area, 2.0 ** -23, f'{name} mask_area')
    _close(got.nll, nll, (U_LOGF + 1) * 2.0 ** -23, f'{name} nll')
    again = matching.overlap(md, gd)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))
    plain = matching.overlap(md, gd, nll=False)
    assert plain.nll is None and torch.equal(plain.inter.view(torch.int32), got.inter.view(torch.int32))


# ---- assignment -------------------------------------------------------------------------------------------------------------------
ASSIGN_SHAPES = [(5, 4), (3, 5), (5, 5), (4, 1), (7, 3), (2, 3), (16, 3), (1, 1), (2, 1)]


def _reference_assign(cost, n):
    """brute force per image + the asserted gap"""
    out = []
    for b in range(cost.shape[0]):
        valid = [bool(v) for v in (n[b] > 0)]
        if not any(valid):
            out.append([-1] * cost.shape[1])
            continue
        a, _, gap = R.brute_force(cost[b].numpy(), valid)
        assert gap >= MIN_GAP, ('the planted input has no clear best assignment', b, gap)
        out.append(a)
    return torch.tensor(out)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('KG', ASSIGN_SHAPES + list(SPECIAL), ids=str)
def test_assignment_equals_brute_force_on_planted_inputs(KG, kind):
    if isinstance(KG, str):
        mask, gt = CASES[KG]
    else:
        mask, gt = R.planted(3, KG[0], KG[1], 16, seed=100 * KG[0] + KG[1])
    st = R.stats(mask, gt)
    cost = R.pair_values(kind, *st)
    want = _reference_assign(cost, st[3])
    got = matching.match_masks(mask.to(DEV), gt.to(DEV), cost=kind)
    assert torch.equal(got.assign.cpu().long(), want), (got.assign.cpu(), want)
    tol = 6 * E if kind == 'iou' else (U_LOGF + 1) * 2.0 ** -23 + E
    real = (st[3] > 0)[..., None].expand_as(cost)
    ref_abs = cost.abs() if kind == 'ce' else (1.0 - cost).abs() + E        # ('iou': the error sits in I / U)
    assert bool((((got.cost.double().cpu() - cost).abs() <= tol * ref_abs + E * cost.abs()) | ~real).all())
    assert not got.cost.cpu()[~real].any() and not got.iou.cpu()[~real].any()
    # the loss op reports the same map
    loss = matching.matched_mask_loss(mask.to(DEV), gt.to(DEV), loss='ce', match=kind)
    assert torch.equal(loss.assign, got.assign) and not loss.assign.requires_grad


def _host_assign(cost, valid):
    c = np.ascontiguousarray(cost, dtype=np.float32)
    a, t = np.full(c.shape[0], -7, dtype=np.int32), np.full(1, -7.0, dtype=np.float32)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    rc = _lib.lib().iodine_assign_host(c.ctypes.data_as(C.c_void_p), None if v is None else v.ctypes.data_as(C.c_void_p), c.shape[0], c.shape[1],
                                       a.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return a, t[0]


@pytest.mark.parametrize('GK', [(1, 1), (3, 5), (5, 3), (6, 6), (16, 16), (16, 7), (7, 16)], ids=str)
def test_device_assign_is_the_host_solver_bitwise(GK):
    """random, non-planted costs (ties included): the device kernel and iodine_assign_host run one function and must agree bit for bit;
    against the brute force only totals and validity are compared, where it is affordable.  A refused matrix (NaN / inf in a real row) is
    part of the batch: the documented refuse-up-front path, all -1 and a NaN total."""
    G, K = GK
    g = torch.Generator().manual_seed(G * 17 + K)
    B = 12
    cost = torch.rand(B, G, K, generator=g)
    cost[1] = torch.randint(0, 3, (G, K), generator=g).float()              # ties
    cost[2] = -cost[2]
    valid = torch.rand(B, G, generator=g) > 0.3
    valid[3] = False
    valid[4] = True
    cost[5, G // 2, K // 2], valid[5, G // 2] = float('nan'), True
    cost[6, 0, 0], valid[6, 0] = float('inf'), True
    cost[7, G - 1, 0], valid[7, G - 1] = float('nan'), False                 # non-finite in a padding row: never read
    for rv in (valid, None):
        a, t = matching.assign(cost.to(DEV), None if rv is None else rv.to(DEV))
        a2, t2 = matching.assign(cost.to(DEV), None if rv is None else rv.to(DEV))
        assert torch.equal(a, a2) and torch.equal(t.view(torch.int32), t2.view(torch.int32))
        a, t = a.cpu(), t.cpu()
        for b in range(B):
            ha, ht = _host_assign(cost[b].numpy(), None if rv is None else rv[b].numpy())
            assert a[b].tolist() == ha.tolist(), (b, a[b], ha)
            assert np.float32(t[b]).view(np.int32) == np.float32(ht).view(np.int32) or (np.isnan(ht) and bool(torch.isnan(t[b])))
            row_ok = [True] * G if rv is None else rv[b].tolist()
            finite = bool(torch.isfinite(cost[b][torch.tensor(row_ok)]).all()) if any(row_ok) else True
            if not finite:
                assert a[b].tolist() == [-1] * G and bool(torch.isnan(t[b]))
                continue
            got = [i for i in range(G) if a[b, i] >= 0]
            assert len({int(a[b, i]) for i in got}) == len(got) == min(sum(row_ok), K) and all(row_ok[i] for i in got)
            if any(row_ok) and max(G, K) <= 6:
                c64 = torch.where(torch.isfinite(cost[b]), cost[b], torch.zeros(())).double().numpy()
                _, best, _ = R.brute_force(c64, row_ok)
                assert abs(float(t[b]) - best) <= 4 * E * sum(abs(float(cost[b, i, a[b, i]])) for i in got) + 1e-12
    lead = matching.assign(cost.view(3, 4, G, K).to(DEV), valid.view(3, 4, G).to(DEV))
    assert tuple(lead[0].shape) == (3, 4, G) and tuple(lead[1].shape) == (3, 4)
    assert torch.equal(lead[0].view(B, G), matching.assign(cost.to(DEV), valid.to(DEV))[0])


# ---- loss and gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('kinds', list(itertools.product(R.KINDS, R.KINDS)), ids=lambda k: f'loss_{k[0]}_match_{k[1]}')
def test_loss_and_gradient_match_float64_reference(name, kinds):
    loss_kind, match_kind = kinds
    mask, gt = CASES[name]
    B, K = mask.shape[:2]
    md = mask.to(DEV).requires_grad_(True)
    gd = gt.to(DEV)
    per = matching.matched_mask_loss(md, gd, loss=loss_kind, match=match_kind, reduction='none')
    asg = per.assign.cpu().long()
    inter, nll, area, n = R.stats(mask, gt)
    # the map is valid: injective, real rows only, min(|R|, K) of them
    for b in range(B):
        got = [g for g in range(asg.shape[1]) if asg[b, g] >= 0]
        assert len({int(asg[b, g]) for g in got}) == len(got) == min(int((n[b] > 0).sum()), K) and all(n[b, g] > 0 for g in got)
    gl = torch.linspace(0.5, 1.5, B)
    ref_per, ref_grad = R.loss_and_grad(mask, gt, asg, loss_kind, grad_loss=gl)
    # loss
    L = R.pair_values(loss_kind, inter, nll, area, n)
    on = (asg >= 0).double()
    M = on.sum(-1).clamp_min(1.0)
    picked = torch.gather(L, 2, asg.clamp_min(0)[..., None])[..., 0] * on
    if loss_kind == 'ce':
        bound = ((U_LOGF + 1) * 2.0 ** -23 + E) * picked.abs().sum(-1) / M
    else:
        bound = 6 * E * ((1.0 - picked) * on).sum(-1) / M + E * ref_per.abs()
    err = (per.detach().double().cpu() - ref_per).abs()
    print(f'[{name} {kinds}] loss error {float(err.max()):.3e}, bound {float(bound.max()):.3e}')
    assert bool((err <= bound + 1e-12).all()), (err, bound)
    mean = matching.matched_mask_loss(md, gd, loss=loss_kind, match=match_kind)
    assert abs(float(mean.detach()) - float(ref_per.mean())) <= float(bound.mean()) + 2 * E * float(ref_per.abs().mean()) + 1e-12
    # gradient
    (per * gl.to(DEV)).sum().backward()
    grad = md.grad.cpu()
    assert grad.shape == mask.shape
    top = float(ref_grad.abs().max())
    gerr = float((grad.double() - ref_grad).abs().max())
    gb = (8 if loss_kind == 'ce' else 13) * E * top
    print(f'[{name} {kinds}] gradient error {gerr:.3e} of max {top:.3e}, bound {gb:.3e}')
    assert gerr <= gb
    for b in range(B):
        for k in range(K):
            if not bool((asg[b] == k).any()):
                assert not grad[b, k].any(), 'a slot that is no row\'s match gets exactly 0'
    # ground truth never receives a gradient, and the unaligned path writes the same gradient
    m2 = _misaligned(mask.to(DEV)).requires_grad_(True)
    per2 = matching.matched_mask_loss(m2, _misaligned(gd), loss=loss_kind, match=match_kind, reduction='none')
    if torch.equal(per2.assign, per.assign):
        g2, = torch.autograd.grad((per2 * gl.to(DEV)).sum(), m2)
        assert float((g2.cpu().double() - ref_grad).abs().max()) <= gb


def test_images_without_objects_cost_nothing():
    mask, gt = CASES['image_without_objects']
    md = mask.to(DEV).requires_grad_(True)
    per = matching.matched_mask_loss(md, gt.to(DEV), reduction='none')
    assert float(per[1].detach()) == 0.0 and per.assign[1].tolist() == [-1] * gt.shape[1]
    per.sum().backward()
    assert not md.grad[1].any() and bool(md.grad[0].any())
    none = matching.matched_mask_loss(md, torch.zeros_like(gt).to(DEV))
    assert float(none) == 0.0
    s = matching.segmentation_scores(mask.to(DEV), gt.to(DEV))
    assert all(np.isnan(v[1]) and np.isfinite(v[0]) and np.isfinite(v[2]) for v in s)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_outputs_are_bitwise_reproducible_and_frames_equal_stacked_calls():
    F, B, K, G, S = 3, 2, 4, 3, 12
    pairs = [R.planted(B, K, G, S, seed=40 + f) for f in range(F)]
    mask = torch.stack([p[0] for p in pairs]).to(DEV)
    gt = torch.stack([p[1] for p in pairs]).to(DEV)
    bits = lambda t: t.contiguous().view(torch.int32)

    def run(m, g):
        m = m.clone().requires_grad_(True)
        per = matching.matched_mask_loss(m, g, loss='iou', match='ce', reduction='none')
        (per * torch.arange(1, per.numel() + 1, device=DEV).view(per.shape)).sum().backward()
        return per.detach(), per.assign, m.grad
    a, b = run(mask, gt), run(mask, gt)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    assert tuple(a[0].shape) == (F, B) and tuple(a[1].shape) == (F, B, G) and a[2].shape == mask.shape
    for f in range(F):
        m = mask[f].clone().requires_grad_(True)
        per = matching.matched_mask_loss(m, gt[f], loss='iou', match='ce', reduction='none')
        (per * torch.arange(1 + f * B, 1 + (f + 1) * B, device=DEV)).sum().backward()
        assert torch.equal(bits(per.detach()), bits(a[0][f])) and torch.equal(per.assign, a[1][f]) and torch.equal(bits(m.grad), bits(a[2][f]))
    st = matching.overlap(mask, gt)
    for f in range(F):
        assert all(torch.equal(bits(x), bits(y[f])) for x, y in zip(matching.overlap(mask[f], gt[f]), st))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _torch_term(mask, gt, asg, kind, eps=1e-6):
    """the matched loss in torch ops on model.mask, with the assignment the op reported"""
    m, t = mask[:, :, 0], gt.float()
    inter = torch.einsum('bgyx,bkyx->bgk', t, m)
    n = t.sum((-1, -2)).clamp_min(1.0)[..., None]
    if kind == 'iou':
        L = 1.0 - inter / (n + m.sum((-1, -2))[:, None, :] - inter)
    else:
        L = -torch.einsum('bgyx,bkyx->bgk', t, torch.log(m + eps)) / n
    on = (asg >= 0).float()
    picked = torch.gather(L, 2, asg.long().clamp_min(0)[..., None])[..., 0] * on
    return (picked.sum(-1) / on.sum(-1).clamp_min(1.0)).mean()


@pytest.mark.parametrize('kind', R.KINDS)
def test_training_step_with_the_mask_term_matches_the_torch_composite(kind):
    arch = O.tiny_arch(slots=3, iters=2, img_size=16)
    B = 2
    pn = synth.make_params(O.param_shapes(arch), seed=50, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    imgs, masks = synth.make_images(B, arch.img_size, seed=51, kind='blobs')
    x = torch.from_numpy(imgs).to(DEV)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=52)).to(DEV)
    gt = matching.pack_gt(masks, arch.img_size, DEV)
    assert gt.shape[0] == B and int(gt.sum()) > 0
    m = make_hip_model(arch, params)

    def grads(use_op, w_loss, w):
        m.zero_grad(set_to_none=True)
        loss = m(x, eps, attach_state=True)
        op = matching.matched_mask_loss(m.mask, gt, loss=kind, match='iou')
        term = op if use_op else _torch_term(m.mask, gt, op.assign, kind)
        (w_loss * loss + w * term).backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, float(op), float(term)
    for w_loss, w in ((1.0, 10.0), (0.0, 1.0)):                              # the step of the issue, and the term alone
        got, v_op, _ = grads(True, w_loss, w)
        ref, _, v_ref = grads(False, w_loss, w)
        assert abs(v_op - v_ref) <= 1e-5 * abs(v_ref) and set(got) == set(ref)
        worst = 0.0
        for n in ref:
            a, r = grad_views(n, got[n].cpu().numpy(), ref[n].cpu().numpy())
            e = rel_l2(a, r)
            worst = max(worst, e)
            assert e < GATE, (n, e, w_loss, w)
        print(f'[{kind}, {w_loss} loss + {w} term] worst rel-L2 {worst:.2e}')
        assert any(bool(g.any()) for n, g in got.items() if n.startswith('decoder.'))


# ---- engine -----------------------------------------------------------------------------------------------------------------------
def _engine_model():
    from iodine_amd import IODINE
    from iodine_amd.model import arch_namespace
    from iodine_amd.optim import make_optimizer
    torch.manual_seed(0)
    m = IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))).to(DEV)
    m.manual_seed(3)
    return m, make_optimizer(m, base_lr=3e-3)


def test_mask_loss_zero_is_the_parent_step_bitwise_and_the_flag_trains():
    from iodine_amd import engine
    from iodine_amd.data import make_dataloader
    dl = make_dataloader(engine.SyntheticScenes(8, 16), batch_size=4, shuffle=False)
    runs = []
    for kw in ({}, {'mask_loss': 0.0}):
        m, opt = _engine_model()
        losses = engine.train(m, opt, dl, torch.device(DEV), 2, print_every=1000, **kw)
        runs.append((losses, [p.detach().clone() for p in m.parameters()]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    # with the term: the log line gains mask-loss, unlabelled batches train unsupervised, the loss stays finite
    m, opt = _engine_model()
    lines = []
    x, masks = next(iter(dl))
    batches = [(x, masks), (x, (None,) * len(masks)), (x, masks)]
    losses = engine.train(m, opt, batches, torch.device(DEV), 3, print_every=1, log=lines.append, mask_loss=1.0, mask_loss_kind='ce')
    assert len(losses) == 3 and np.isfinite(losses).all() and all('mask-loss: ' in s for s in lines)
    assert float(lines[0].split('mask-loss: ')[1]) > 0.0 and float(lines[1].split('mask-loss: ')[1]) == 0.0
    ev = engine.evaluate(m, dl, torch.device(DEV), evaluator=matching.SegmentationEvaluator())
    assert len(ev.aris) == len(ev.mious) == len(ev.scs) == len(ev.mscs) == 8
    assert set(ev.global_means) == {'aris', 'mious', 'scs', 'mscs'} and ev.global_means['aris'] == ev.global_mean
    assert all(0.0 <= ev.global_means[k] <= 1.0 for k in ('mious', 'scs', 'mscs'))
    assert abs(ev.global_means['mious'] - float(np.mean(ev.mious))) < 1e-12
    plain = engine.evaluate(m, dl, torch.device(DEV))
    assert len(plain.aris) == 8 and not hasattr(plain, 'global_means')


# ---- evaluator --------------------------------------------------------------------------------------------------------------------
class _Decode:
    """stands in for a model: reconstruct returns the given masks"""

    def __init__(self, mask):
        self.mask = mask

    def reconstruct(self, image):
        return None, self.mask, None


def test_segmentation_evaluator_scores():
    B, G, S = 3, 4, 16
    g = torch.Generator().manual_seed(9)
    label = torch.randint(0, G + 1, (B, S, S), generator=g)                 # G = background
    gt = torch.stack([(label == i) for i in range(G)], 1).to(torch.uint8)
    perm = torch.randperm(G + 1, generator=g)
    hot = torch.stack([(label == int(perm[k])) for k in range(G + 1)], 1).float().unsqueeze(2)
    ev = matching.SegmentationEvaluator()
    ev.evaluate(_Decode(hot.to(DEV)), (None, [m.numpy() for m in gt]))
    assert ev.aris == [1.0] * B and ev.mious == [1.0] * B and ev.scs == [1.0] * B and ev.mscs == [1.0] * B
    assert ev.get_results() == 'Ari: 1.0, mIoU: 1.0, SC: 1.0, mSC: 1.0'
    ev.reset()
    assert ev.aris == [] and ev.mious == []
    # planted soft masks: the reference scores to float64 rounding, the ARI as ARIEvaluator computes it
    from iodine_amd.ari import ARIEvaluator
    for name in ('B3K7G3S68', 'zero_row_between', 'more_objects_than_slots'):
        mask, gt = CASES[name]
        ev.reset()
        ev.evaluate(_Decode(mask.to(DEV)), (None, [m.numpy() for m in gt]))
        ref = R.hard_scores(mask, gt)
        for b, (miou, sc, msc) in enumerate(ref):
            assert abs(ev.mious[b] - miou) < 1e-12 and abs(ev.scs[b] - sc) < 1e-12 and abs(ev.mscs[b] - msc) < 1e-12, (name, b)
        s = matching.segmentation_scores(mask.to(DEV), gt.to(DEV))
        assert s.miou.tolist() == ev.mious and s.sc.tolist() == ev.scs and s.msc.tolist() == ev.mscs
        ari = ARIEvaluator()
        ari.evaluate(_Decode(mask.to(DEV)), (None, [m.numpy() for m in gt]))
        assert ari.aris == ev.aris
