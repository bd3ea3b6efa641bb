"""``model.likelihood = 'joint'`` (library option joint_likelihood) on the device: one mixture per pixel over the RGB vector in place of the
reference's mixture per colour channel.  The reference of the mode is tests/joint_reference.py (the pinned oracle under a three-line
change of its ``elbo_terms``); every test here fails on a library without the option.

Kernel level (iodine_op_pixel_encode with flags bit 3: pixel_pass1 / pixel_sigma_grad / pixel_pass2 plain and split, strict and default,
stable 0 / 1; iodine_op_pixel_maps with bit 1: pixel_like_maps / pixel_input_grad): against float64 at the project's margins
(pixel_reference.MARGIN) over the float32 CPU floor of the JOINT reference, capped at pixel_reference.GATE_CAP - measured from the
reference, never from the kernel; exclusions are pixel_reference.excluded()'s, by name.  Exact properties: split = plain, two runs, unit
weights, zero weights, and the bits the form must not reach (channels 8 and 14 and their statistics, the decode).

Module level (three architectures: the unfused first refinement layer, refine_l0_fused, the generic path; default and strict path):
reconstruct, a training step with x, weights= and sigma as leaves, elbo(x).backward(), at the gates of the per-channel tests of the same
quantities (tests/test_gpu_train.py, test_gpu_reconstruct.py, test_gpu_input_grad.py, test_gpu_sigma_grad.py: values 1e-4, gradient tensors
rel-L2 1e-3); predictive, the likelihood map, K = 1, mode switches (eager and hipGraph), the refused backward, a clip with per-frame weights."""
import ctypes as C
import dataclasses
import functools
import itertools
import math

import pytest
import torch

import joint_reference as J
import pixel_reference as R
import sigma_reference as SR
import weights_reference as W
from clip_reference import moving_clip
from iodine_amd import _lib
from oracle import iodine_oracle as O
from test_gpu_pixel import OUT, _check, _dev, _out, _take, assemble, same_bits
from util import grad_views, make_hip_model, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE, VGATE = 1e-3, 1e-4
FORMS = list(itertools.product((0, 1), (0, 1), (0, 1)))         # (strict, split, stable)


@pytest.fixture(scope='module', autouse=True)
def library_has_the_option():
    """a library that does not know the option would ignore the flag bits below and run the per-channel kernels: refuse it up front"""
    from iodine_amd import synth
    pn = synth.make_params(O.param_shapes(O.tiny_arch()), seed=1, dec_gain=3.0, posterior_scale=0.05)
    m = make_hip_model(O.tiny_arch(), {k: torch.from_numpy(v) for k, v in pn.items()})
    m.set_option('joint_likelihood', 1)
    m._session.open(torch.device(DEV))                            # (the handle is made here and takes the options set so far)


# ---- 1. kernel level: iodine_op_pixel_encode, flags bit 3 ----------------------------------------------------------------------------------
def run(inp, strict=0, split=0, stable=0, joint=1, want=OUT):
    """test_gpu_pixel.run with the form bit -> {name: CPU tensor}"""
    B, K, P = inp['dec'].shape[:3]
    S, L = inp['lin'].numel(), inp['pm'].shape[2]
    shapes = {'g': (B, K, P, 4), 'lnstat': (B, K, 8), 'll_img': (B,), 'img_terms': (B, 2), 'scal': (3,), 'sgrad': (1,),
              'enc': (B, K, P, 12 if split else 20), 'enc_sh': (B, P, 8), 'pred': (B, 3, P), 'mask': (B, K, P), 'mean': (B, K, 3, P), 'logits': (B, K, P)}
    names = [k for k in OUT if k in want and (k != 'enc_sh' or split)]
    bufs = {k: _out(torch.Size(shapes[k]).numel()) for k in names}
    arr = (C.c_void_p * 12)(*[bufs[k].data_ptr() if k in bufs else None for k in OUT])
    flags = (1 if strict else 0) | (2 if inp['use_ln'] else 0) | (4 if stable else 0) | (8 if joint else 0)
    rc = _lib.lib().iodine_op_pixel_encode(None, _lib.ptr(inp['x']), _lib.ptr(inp['w']), _lib.ptr(inp['dec']), _lib.ptr(inp['pm']), _lib.ptr(inp['plv']),
                                           _lib.ptr(inp['lin']), B, K, S, L, inp['sigma'], inp['beta'], flags, R.CH_FULL, 1, arr)
    _check(rc, f'iodine_op_pixel_encode B {B} K {K} S {S} strict {strict} split {split} stable {stable} joint {joint}')
    torch.cuda.synchronize()
    res = {k: _take(bufs[k], shapes[k], k) for k in names}
    res['kl_img'] = res['img_terms'][:, 1]
    if 'enc' in res:
        res['enc17'] = assemble(res, split)
    return res


@pytest.mark.parametrize('case', J.GPU_CASES)
def test_kernels_against_float64(case):
    """every output of every form of the joint kernels at the gates of the joint reference"""
    ref, cpu = J.case_reference(case)
    worst = {}
    for strict, split, stable in FORMS:
        res = run(_dev(case), strict, split, stable)
        got = {k: res[k] for k in R.SCALARS + R.PLANES + ('lnstat',)}
        got['enc'] = res['enc17']
        e = R.errors(got, ref, case, stable)
        assert set(e) == set(cpu[stable]), 'the device compares what the CPU floor covers'
        for k, v in e.items():
            worst[(strict, k)] = max(worst.get((strict, k), 0.0), v)
    for strict in (1, 0):
        print(f'[joint] {case} {"strict " if strict else "default"}: ' + ', '.join(f'{k} {v:.2e}' for (s, k), v in worst.items() if s == strict and v > 0))
    for strict in (1, 0):
        gate = J.gates(strict)
        bad = {k: (v, gate[k]) for (s, k), v in worst.items() if s == strict and not v <= gate[k]}
        assert not bad, (case, strict, bad)


@pytest.mark.parametrize('case', J.GPU_CASES)
def test_exact_properties(case):
    """split = plain, two runs, unit weights: the same bits; a pixel of weight 0: no gradient at all"""
    inp = _dev(case)
    for strict, stable in ((0, 0), (1, 1)):
        plain, split = run(inp, strict, 0, stable), run(inp, strict, 1, stable)
        for lane, ch in enumerate(R.SPLIT_SLOT):
            if ch >= 0:
                assert same_bits(split['enc'][..., lane], plain['enc'][..., ch]), (case, strict, stable, ch)
        for lane, ch in enumerate(R.SPLIT_SHARED):
            if ch >= 0:
                for k in range(plain['enc'].shape[1]):
                    assert same_bits(split['enc_sh'][..., lane], plain['enc'][:, k, :, ch]), (case, strict, stable, ch, k)
        others = [k for k in plain if k not in ('enc', 'enc17') and not same_bits(plain[k], split[k])]
        assert not others, (case, others)
        again = run(inp, strict, 0, stable)
        diff = [k for k in plain if not same_bits(plain[k], again[k])]
        assert not diff, (case, strict, diff)
    if inp['w'] is None:
        B, _, P = inp['x'].shape
        a, b = run(inp, 0, 1, 0), run({**inp, 'w': torch.ones(B, P, device=DEV)}, 0, 1, 0)
        diff = [k for k in a if not same_bits(a[k], b[k])]
        assert not diff, (case, diff)
    else:
        zero = R.case_inputs(case)['w'] == 0
        assert zero.any()
        for strict in (0, 1):
            g = run(inp, strict, 0, 0, want=OUT[:5])['g'].permute(0, 2, 1, 3)                  # (B, P, K, 4): rgb lanes and the mask gradient
            assert not g[zero].any(), (case, strict)
            assert g[~zero].abs().amax(dim=(1, 2)).min() > 0


@pytest.mark.parametrize('case', J.GPU_CASES)
def test_the_form_does_not_reach_what_was_joint_already(case):
    """mask_posterior (8), the leave-one-out likelihood (14) and its statistics, the decode and the KL: the bits of the per-channel run"""
    inp = _dev(case)
    K = inp['dec'].shape[1]
    for strict, split, stable in ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        a, b = run(inp, strict, split, stable, joint=0), run(inp, strict, split, stable, joint=1)
        for k in ('pred', 'mask', 'mean', 'logits', 'kl_img'):
            assert same_bits(a[k], b[k]), (case, k)
        for ch in (0, 1, 2, 3, 4, 5, 6, 7, 8, 14, 15, 16):
            assert same_bits(a['enc17'][..., ch], b['enc17'][..., ch]), (case, strict, split, stable, ch)
        assert same_bits(a['lnstat'][..., 4:6], b['lnstat'][..., 4:6])
        if K > 1:
            assert not same_bits(a['g'], b['g']) and not same_bits(a['ll_img'], b['ll_img'])  # ... and the form does reach the objective


def test_the_default_form_ignores_nothing_else():
    """flags without bit 3 are the per-channel kernels: test_gpu_pixel's reference, its gates"""
    case = 'near_k3_s23_w_beta'
    ref, _ = R.case_reference(case)
    res = run(_dev(case), 1, 0, 0, joint=0)
    assert R.scalar_err(res['ll_img'], ref['ll_img']) <= R.gates(1)['ll_img']
    assert R.scalar_err(res['ll_img'], J.case_reference(case)[0]['ll_img']) > 0.01


# ---- 2. kernel level: iodine_op_pixel_maps, flag bit 1 ---------------------------------------------------------------------------------------
def _maps_reference(x, w, dec, sigma):
    """(ll (B, 1, P), kll (B, K, 3, P), vx (B, 3, P) = d / d x of sum_p w ll, vw (B, P) = ll) in float64, the gradients by autograd"""
    xl = x.clone().requires_grad_(True)
    wl = (torch.ones_like(x[:, 0]) if w is None else w.clone()).requires_grad_(True)
    mean = torch.sigmoid(dec[..., :3]).permute(0, 1, 3, 2)
    mask = torch.softmax(dec[..., 3], dim=1)[:, :, None]
    kll = -(xl[:, None] - mean) ** 2 / (2 * sigma ** 2) - math.log(sigma) - 0.5 * math.log(2 * math.pi)
    ll = J.joint_ll_px(mask, kll)
    vx, vw = torch.autograd.grad((wl[:, None] * ll).sum(), [xl, wl])
    return ll.detach(), kll.detach(), vx, vw


@pytest.mark.parametrize('strict', [0, 1], ids=['default', 'strict'])
@pytest.mark.parametrize('K', [1, 7, 16])
def test_maps_and_input_gradients_against_float64(K, strict):
    """ll (B, 1, P), kll, gx, gw of the joint form at VGATE (test_gpu_input_grad's gate for the per-channel kernels), a first launch followed
    by an accumulating one; sum_p ll against ll_img of the encode entry at the ll_img gate"""
    B, sigma = 2, R.f32(0.1)
    worst = dict(ll=0.0, kll=0.0, gx=0.0, gw=0.0)
    for S, weighted in itertools.product((5, 23), (False, True)):
        P = S * S
        inp = R.make_inputs('near', B, K, S, 4, sigma, 1.0, 1, weighted, 0.5)
        x, w, dec = inp['x'], inp['w'], inp['dec']
        ll, kll, vx, vw = _maps_reference(x.double(), None if w is None else w.double(), dec.double(), sigma)
        xd, wd, dd = x.to(DEV), None if w is None else w.to(DEV), dec.to(DEV).contiguous()
        llbuf = torch.full((B * P + 2 * B * P,), -7.25e9, device=DEV)                          # ll is ONE plane per image: the room of the
        llbuf[:B * P] = float('nan')                                                           # other two of a (B, 3, P) map stays untouched
        o = [llbuf[:B * P].view(B, 1, P)] + [torch.full(s, float('nan'), device=DEV) for s in ((B, K, 3, P), (B, 3, P), (B, P))]
        for coef, first, outs in ((0.75, 1, o), (-0.5, 0, [None, None, o[2], o[3]])):
            rc = _lib.lib().iodine_op_pixel_maps(None, _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(dd), B, K, P, sigma, strict | 2, coef,
                                                 *[_lib.ptr(t) for t in outs], first)
            _check(rc, f'iodine_op_pixel_maps K {K} P {P} strict {strict} joint')
        torch.cuda.synchronize()
        got = [t.cpu() for t in o]
        assert bool((llbuf[B * P:] == -7.25e9).all())
        for key, a, b in (('ll', got[0], ll), ('kll', got[1], kll), ('gx', got[2], 0.25 * vx), ('gw', got[3], 0.25 * vw)):
            assert torch.isfinite(a).all(), (key, K, P, weighted)
            worst[key] = max(worst[key], rel_err(a, b))
        if weighted:
            assert not got[2].permute(0, 2, 1)[w == 0].any(), (K, P)
        dev = {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in inp.items()}
        ll_img = run(dev, strict, 0, 0, want=OUT[:5])['ll_img']
        total = (got[0][:, 0].double() * (1.0 if w is None else w.double())).sum(dim=1)
        assert R.scalar_err(total, ll_img) <= J.gates(strict)['ll_img'], (K, P, weighted)
    print(f'[joint maps K={K} strict={strict}] ' + ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))
    assert all(v < VGATE for v in worst.values()), worst


# ---- 3. module level ---------------------------------------------------------------------------------------------------------------------------
B = 2
SIGMA = float(torch.tensor(0.1, dtype=torch.float32))
BASE = O.tiny_arch()                                                                           # K 3, T 2, S 16, 32 channels
ARCHS = {
    'tiny': BASE,                                                                              # the unfused first refinement layer
    'l0f': O.tiny_arch(slots=4, iters=2, img_size=32, chan=64),                                # refine_l0_fused: 64 channels, S >= 32
    'generic': dataclasses.replace(BASE, dec_kernel=5),                                        # the generic decoder path
    'k1': dataclasses.replace(BASE, slots=1),
}
PATHS = [pytest.param(1, id='default'), pytest.param(0, id='strict')]


@functools.lru_cache(maxsize=None)
def _inputs(key):
    return SR.inputs(ARCHS[key], B)


@functools.lru_cache(maxsize=None)
def _reference(key):
    """the patched oracle in float64: reconstruct; a training step with the image, the pixel weights and sigma as leaves; one elbo from the
    refined posterior with the posterior as a leaf"""
    a = ARCHS[key]
    params, x, eps = _inputs(key)
    p64, x64, e64, w64 = {k: v.double() for k, v in params.items()}, x.double(), eps.double(), W.pattern(B, a.img_size).double()
    with J.patched():
        rec = SR.reconstruct(x64, e64, p64, a, SIGMA)
        q = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
        xl, wl, s = x64.clone().requires_grad_(True), w64.clone().requires_grad_(True), SR.as_sigma(SIGMA, torch.float64, True)
        out = SR.train_forward(xl, e64, q, a, s, 1.0, None, wl)
        names = list(q)
        grads = torch.autograd.grad(out['loss'], [q[n] for n in names] + [xl, wl, s], allow_unused=True)
        gd = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, grads)}
        pm, plv = rec['post_mean'].clone().requires_grad_(True), rec['post_logvar'].clone().requires_grad_(True)
        t = J.joint_s_terms(x64, None, pm, plv, e64[0], p64, a, SR.as_sigma(SIGMA))
        g_pm, g_plv = torch.autograd.grad(t['elbo'], [pm, plv])
    plain = SR.train_step_grads(x64, e64, p64, a, SIGMA, w=w64)[0]      # outside the patch: the per-channel step, same weights and sigma
    return dict(rec=rec, loss=out['loss'].detach(), elbos=out['elbos'].detach(), kls=out['kls'].detach(), lls=out['lls'].detach(), grads=gd,
                gx=grads[-3].detach(), gw=grads[-2].detach(), gs=grads[-1].detach(), plain=plain, elbo=t['elbo'].detach(), g_pm=g_pm, g_plv=g_plv,
                ll_px=out['terms'][-1]['ll_px'].detach())


def _model(key, prec=1, **options):
    params, _, _ = _inputs(key)
    m = make_hip_model(ARCHS[key], params, options={'conv_precision': prec, **options})
    m.likelihood, m.sigma = 'joint', SIGMA
    return m


@pytest.mark.parametrize('prec', PATHS)
@pytest.mark.parametrize('key', ['tiny', 'l0f', 'generic'])
def test_reconstruct(key, prec):
    ref = _reference(key)['rec']
    _, x, eps = _inputs(key)
    m = _model(key, prec)
    m.set_option('profile', 2)
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV), trajectory=True)
    if key == 'l0f':
        assert m.profile_read('seen:refine_l0f')[1] == (ARCHS[key].iters if prec == 1 else 0)   # (the fused layer is a split-fp16 kernel)
    e = dict(pred=rel_err(pred.cpu(), ref['pred']), mask=rel_err(mask.cpu(), ref['mask']), mean=rel_err(mean.cpu(), ref['mean']),
             post_mean=rel_err(m.posterior.mean.cpu(), ref['post_mean']), elbo=rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']),
             kl=rel_err(m.elbo_terms[:, 1].cpu(), ref['kls']), ll=rel_err(m.elbo_terms[:, 2].cpu(), ref['lls']),
             traj_ll=rel_err(m.trajectory['ll'].cpu().mean(dim=1), ref['lls']))
    print(f'[joint reconstruct {key} prec {prec}] ' + ', '.join(f'{k} {v:.1e}' for k, v in e.items()))
    assert all(v < VGATE for v in e.values()), e


@pytest.mark.parametrize('prec', PATHS)
@pytest.mark.parametrize('key', ['tiny', 'l0f', 'generic'])
def test_training_step_with_every_leaf(key, prec):
    """loss, elbo_terms, every parameter gradient, x.grad, weights.grad and sigma.grad of one step in joint mode"""
    ref = _reference(key)
    a = ARCHS[key]
    _, x, eps = _inputs(key)
    m = _model(key, prec)
    m.set_option('profile', 2)
    s = torch.tensor(SIGMA, dtype=torch.float32, device=DEV, requires_grad=True)
    xd, wd = x.to(DEV).requires_grad_(True), W.pattern(B, a.img_size).float().to(DEV).requires_grad_(True)
    m.sigma = s
    m.zero_grad(set_to_none=True)
    loss = m(xd, eps.to(DEV), weights=wd)
    loss.backward()
    torch.cuda.synchronize()
    if key == 'l0f':
        assert m.profile_read('seen:refine_l0f')[1] == (a.iters if prec == 1 else 0)
    assert m.profile_read('seen:pixel_pass1')[1] == a.iters + 1 and m.profile_read('seen:pixel_sigma_grad')[1] == a.iters + 1
    assert m.profile_read('seen:pixel_input_grad')[1] == a.iters + 1
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), ref['grads'][n].numpy())), n) for n, p in m.named_parameters())
    e = dict(loss=abs(loss.item() - ref['loss'].item()) / abs(ref['loss'].item()), elbo=rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']),
             kl=rel_err(m.elbo_terms[:, 1].cpu(), ref['kls']), ll=rel_err(m.elbo_terms[:, 2].cpu(), ref['lls']))
    ge = dict(params=worst[0], x=rel_l2(xd.grad.cpu().numpy(), ref['gx'].numpy()), w=rel_l2(wd.grad.cpu().numpy(), ref['gw'].numpy()),
              sigma=abs(s.grad.item() - ref['gs'].item()) / abs(ref['gs'].item()))
    print(f'[joint step {key} prec {prec}] ' + ', '.join(f'{k} {v:.1e}' for k, v in {**e, **ge}.items()) + f' (worst parameter {worst[1]})')
    assert all(v <= VGATE for v in e.values()), e
    assert all(v < GATE for v in ge.values()), (ge, worst)
    # ... and it is not the per-channel step
    assert abs(loss.item() - ref['plain']['loss'].item()) > 0.01 * abs(loss.item())


@pytest.mark.parametrize('prec', PATHS)
@pytest.mark.parametrize('key', ['tiny', 'l0f', 'generic'])
def test_elbo_backward_into_the_posterior(key, prec):
    ref = _reference(key)
    _, x, eps = _inputs(key)
    m = _model(key, prec)
    m.likelihood_maps = True
    m.posterior.mean = ref['rec']['post_mean'].float().to(DEV).requires_grad_(True)
    m.posterior.logvar = ref['rec']['post_logvar'].float().to(DEV).requires_grad_(True)
    pm, plv = m.posterior.mean, m.posterior.logvar
    e = m.elbo(x.to(DEV), eps[0].to(DEV))
    S = ARCHS[key].img_size
    assert m.log_likelihood.shape == (B, 1, S, S) and m.K_log_likelihood.shape == (B, ARCHS[key].slots, 3, S, S)
    total = m.log_likelihood.double().sum().item() / B
    assert abs(total - m.elbo_terms[-1, 2].item()) <= 4 * 2.0 ** -24 * max(abs(total), m.log_likelihood.abs().sum().item() / B)    # fp32 rounding
    e.backward()
    err = dict(elbo=abs(e.item() - ref['elbo'].item()) / abs(ref['elbo'].item()), g_pm=rel_l2(pm.grad.cpu().numpy(), ref['g_pm'].numpy()),
               g_plv=rel_l2(plv.grad.cpu().numpy(), ref['g_plv'].numpy()))
    print(f'[joint elbo {key} prec {prec}] ' + ', '.join(f'{k} {v:.1e}' for k, v in err.items()))
    assert err['elbo'] <= VGATE and err['g_pm'] < GATE and err['g_plv'] < GATE, err


def test_likelihood_map_of_a_training_forward():
    ref = _reference('tiny')
    _, x, eps = _inputs('tiny')
    m = _model('tiny')
    m.likelihood_maps = True
    with torch.no_grad():
        m(x.to(DEV), eps.to(DEV), weights=W.pattern(B, BASE.img_size).float().to(DEV))
    assert m.log_likelihood.shape == (B, 1, 16, 16)
    assert rel_err(m.log_likelihood.cpu(), ref['ll_px']) < VGATE                                 # raw: the weights do not enter the map
    m.likelihood = 'per_channel'
    with torch.no_grad():
        m(x.to(DEV), eps.to(DEV))
    assert m.log_likelihood.shape == (B, 3, 16, 16)


def test_predictive_ll():
    """predictive(x, samples=4).ll against the joint likelihood in float64 torch from decode of the returned samples"""
    _, x, eps = _inputs('tiny')
    m = _model('tiny')
    xd = x.to(DEV)
    m.reconstruct(xd, eps.to(DEV))
    g = torch.Generator().manual_seed(5)
    pe = torch.randn(4, B, BASE.slots, BASE.dim_latent, generator=g)
    w = W.pattern(B, BASE.img_size).float().to(DEV)
    for weights in (None, w):
        pr = m.predictive(xd, samples=4, eps=pe.to(DEV), weights=weights)
        for s in range(4):
            _, mask, mean = m.decode(pr.z[s])
            k_ll = O.gaussian_log_likelihood(x.double()[:, None], mean.double().cpu(), SIGMA)
            ll = J.joint_ll_px(mask.double().cpu(), k_ll)
            ll = (ll if weights is None else w.double().cpu() * ll).sum(dim=(1, 2, 3))
            assert rel_err(pr.ll[s].cpu(), ll) < VGATE, (s, weights is not None)
        assert torch.isfinite(pr.iwae).all() and torch.isfinite(pr.elbo_mc).all() and torch.isfinite(pr.elbo).all()
    m.likelihood = 'per_channel'
    assert not torch.equal(m.predictive(xd, samples=4, eps=pe.to(DEV)).ll, pr.ll)


def test_one_slot_both_modes_agree():
    _, x, eps = _inputs('k1')
    m = _model('k1')
    pj = m.reconstruct(x.to(DEV), eps.to(DEV))[0]
    tj = m.elbo_terms.clone()
    m.likelihood = 'per_channel'
    pc = m.reconstruct(x.to(DEV), eps.to(DEV))[0]
    assert torch.equal(pj, pc)
    assert rel_err(tj[:, 2].cpu(), m.elbo_terms[:, 2].cpu()) <= 4 * 2.0 ** -24


@pytest.mark.parametrize('graph', [0, 1], ids=['eager', 'graph'])
def test_switching_modes_on_one_model(graph):
    """per_channel -> joint -> per_channel: the third call returns the first call's bits, and - on a fresh model - so does a model that
    never left the default; with option graph the key carries the form (replays included)"""
    params, x, eps = _inputs('tiny')
    xd, ed = x.to(DEV), eps.to(DEV)
    fresh = make_hip_model(BASE, params)
    want = [t.clone() for t in fresh.reconstruct(xd, ed)] + [fresh.elbo_terms.clone()]
    m = make_hip_model(BASE, params, options={'graph': graph})
    seen = {}
    for step, mode in enumerate(['per_channel', 'joint', 'per_channel'] * (3 if graph else 1)):
        m.likelihood = mode
        got = [t.clone() for t in m.reconstruct(xd, ed)] + [m.elbo_terms.clone()]
        if mode in seen:
            assert all(torch.equal(u, v) for u, v in zip(got, seen[mode])), (step, mode)
        seen[mode] = got
    assert all(torch.equal(u, v) for u, v in zip(seen['per_channel'], want))
    assert not torch.equal(seen['joint'][3], seen['per_channel'][3])
    assert rel_err(seen['joint'][3][:, 0].cpu(), _reference('tiny')['rec']['elbos']) < VGATE
    if graph:
        assert m.profile_read('graph_replays')[1] > 0


def test_a_mode_switch_discards_the_saved_forward():
    _, x, eps = _inputs('tiny')
    m = _model('tiny')
    loss = m(x.to(DEV), eps.to(DEV))
    m.set_option('joint_likelihood', 0)                                                         # reaches the handle at once
    with pytest.raises(RuntimeError, match='joint_likelihood changed after the forward pass'):
        loss.backward()
    assert m.likelihood == 'per_channel'
    m.posterior.mean = m.posterior.mean.detach().requires_grad_(True)
    e = m.elbo(x.to(DEV), eps[0].to(DEV))
    m.set_option('joint_likelihood', 1)
    with pytest.raises(RuntimeError, match='joint_likelihood changed after the forward pass'):
        e.backward()
    m.zero_grad(set_to_none=True)
    m(x.to(DEV), eps.to(DEV)).backward()                                                        # the next step is a step like any other
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    with pytest.raises(ValueError, match='joint_likelihood'):
        m.set_option('joint_likelihood', 2)
    assert _lib.lib().iodine_set_option(m._handle, b'joint_likelihood', 2.0) == 1              # IODINE_ERR_INVALID


def test_chunked_calls_follow_the_mode():
    """batch_cap 1: two library calls per model call, each prepared in joint form; the merged state is the whole batch's"""
    ref = _reference('tiny')
    _, x, eps = _inputs('tiny')
    m = _model('tiny', batch_cap=1)
    m.likelihood_maps = True
    m.reconstruct(x.to(DEV), eps.to(DEV))
    assert rel_err(m.elbo_terms[:, 0].cpu(), ref['rec']['elbos']) < VGATE and m.log_likelihood.shape == (B, 1, 16, 16)
    s = torch.tensor(SIGMA, dtype=torch.float32, device=DEV, requires_grad=True)
    xd, wd = x.to(DEV).requires_grad_(True), W.pattern(B, 16).float().to(DEV).requires_grad_(True)
    m.sigma = s
    m.zero_grad(set_to_none=True)
    loss = m(xd, eps.to(DEV), weights=wd)
    loss.backward()
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), ref['grads'][n].numpy())), n) for n, p in m.named_parameters())
    assert abs(loss.item() - ref['loss'].item()) <= VGATE * abs(ref['loss'].item()) and worst[0] < GATE, worst
    assert rel_l2(xd.grad.cpu().numpy(), ref['gx'].numpy()) < GATE and rel_l2(wd.grad.cpu().numpy(), ref['gw'].numpy()) < GATE
    assert abs(s.grad.item() - ref['gs'].item()) < GATE * abs(ref['gs'].item())


def test_clip_with_per_frame_weights():
    """a clip (B, T + 1, 3, S, S) with per-frame weights: evaluation e scores frame e under its own weights, in joint mode"""
    params, x, eps = _inputs('tiny')
    E = BASE.iters + 1
    xc, wc = moving_clip(x, E), W.clip_pattern(B, E, BASE.img_size)
    p64 = {k: v.double() for k, v in params.items()}
    with J.patched():
        q = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
        xl, wl = xc.double().clone().requires_grad_(True), wc.double().clone().requires_grad_(True)
        out = SR.train_forward(xl, eps.double(), q, BASE, SR.as_sigma(SIGMA), 1.0, None, wl)
        names = list(q)
        grads = torch.autograd.grad(out['loss'], [q[n] for n in names] + [xl, wl])
    m = _model('tiny')
    xd, wd = xc.to(DEV).requires_grad_(True), wc.float().to(DEV).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    loss = m(xd, eps.to(DEV), weights=wd)
    loss.backward()
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), g.numpy())), n) for (n, p), g in zip(m.named_parameters(), grads))
    assert abs(loss.item() - out['loss'].item()) <= VGATE * abs(out['loss'].item())
    assert rel_err(m.elbo_terms[:, 2].cpu(), out['lls'].detach()) < VGATE
    assert worst[0] < GATE, worst
    assert rel_l2(xd.grad.cpu().numpy(), grads[-2].numpy()) < GATE and rel_l2(wd.grad.cpu().numpy(), grads[-1].numpy()) < GATE
