"""Gradients into the image and the pixel weights (option input_grad, iodine_last_input_grad) and the per-pixel likelihood maps
(``model.likelihood_maps``, iodine_last_likelihood) on the device.

Ground truth: the float64 run of tests/input_grad_reference.py (x and w leaves that autograd sees; test_input_grad_cpu pins its closed form
to autograd, and the float32 oracle's own distance from it to far below a third of a gate).  Gates are the project's own
(tests/test_gpu_objective.py): gradient tensors rel-L2 below GATE = 1e-3, values below VGATE = 1e-4; "bitwise" is torch.equal.

Worst figures measured on an MI355X (all cases of this file): the two kernels against float64 - log_likelihood 4.3e-7, K_log_likelihood 2.5e-7,
gx 1.0e-6 (K = 2), gw 1.4e-6 (K = 16), the strict path no worse; a training step - x.grad 2.0e-6 rel-L2 (dSprites architecture; 1.5e-6 at K = 16,
<= 8.3e-7 elsewhere, both conv precisions), weights.grad 4.2e-7 (per-frame weights of a clip), parameter gradients 1.4e-6, loss 4.1e-7; elbo -
x.grad 9.8e-7, weights.grad 3.5e-7, parameters 4.6e-7; the maps after elbo / forward / reconstruct (still, clip, chunked) 8.5e-7 at worst, and their
sum over channels and pixels equals the reported LL to all printed digits (-3143.110352).  The float32 oracle is 7.6e-7 from the float64 one on the
tiny case (test_input_grad_cpu), far below a third of a gate: every case holds the plain gates."""
import dataclasses
import functools
import itertools

import pytest
import torch

from iodine_amd import _lib
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

import input_grad_reference as G
import sigma_reference as R
import weights_reference as W
from clip_reference import moving_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE, VGATE = 1e-3, 1e-4
BASE = O.tiny_arch()                                            # S = 16, K = 3, T = 2
B = 2
SIGMA = float(torch.tensor(0.1, dtype=torch.float32))

ARCHS = {
    'tiny': BASE,
    'k1': dataclasses.replace(BASE, slots=1),
    'k16': dataclasses.replace(BASE, slots=16),
    's12': dataclasses.replace(BASE, img_size=12),              # generic path; P = 144 is no multiple of 64: partial waves
    'dsprites': O.dsprites_arch(slots=4, iters=2),              # S = 64: several blocks per image, split first layer
    'padded': dataclasses.replace(BASE, dim_latent=6),          # a padded inner handle: the adapter forwards the new entries
}


# ---- 1. the two kernels through iodine_op_pixel_maps -----------------------------------------------------------------------------------
PIXELS = (1, 63, 65, 144, 257, 4097)


def _kernel_inputs(K, P, weighted):
    g = torch.Generator().manual_seed(1000 * K + P)
    x = torch.rand(B, 3, P, generator=g)
    dec = torch.randn(B, K, P, 4, generator=g) * 1.5
    w = None
    if weighted:
        w = 0.25 + 1.25 * torch.rand(B, P, generator=g)
        w[:, P // 3:P // 3 + max(1, P // 4)] = 0.0               # an all-zero region
    return x, w, dec


def _op(x, w, dec, K, P, strict, coef, first, outs):
    L = _lib.lib()
    rc = L.iodine_op_pixel_maps(None, _lib.ptr(x), _lib.ptr(w), _lib.ptr(dec), B, K, P, SIGMA, strict, coef, *[_lib.ptr(o) for o in outs], first)
    assert rc == 0, rc


@pytest.mark.parametrize('strict', [0, 1], ids=['default', 'strict'])
@pytest.mark.parametrize('K', [1, 2, 7, 16])
def test_kernels_against_float64(K, strict):
    """all four outputs at VGATE for every pixel count, with and without weights; a first launch followed by an accumulating one; gx exactly 0
    and gw the raw map where the weight is 0.  Measured worst: printed per (K, strict)"""
    worst = dict(ll=0.0, kll=0.0, gx=0.0, gw=0.0)
    for P, weighted in itertools.product(PIXELS, (False, True)):
        x, w, dec = _kernel_inputs(K, P, weighted)
        ll, kll, vx, vw = G.kernel_reference(x.double(), None if w is None else w.double(), dec.double(), SIGMA)
        xd, wd, dd = x.to(DEV), None if w is None else w.to(DEV), dec.to(DEV).contiguous()
        # (poisoned outputs: a pixel the kernel skipped would show)
        o = [torch.full(s, float('nan'), device=DEV) for s in ((B, 3, P), (B, K, 3, P), (B, 3, P), (B, P))]
        _op(xd, wd, dd, K, P, strict, 0.75, 1, o)
        _op(xd, wd, dd, K, P, strict, -0.5, 0, [None, None, o[2], o[3]])          # accumulates 0.75 v - 0.5 v
        torch.cuda.synchronize()
        got = [t.cpu() for t in o]
        for key, a, b in (('ll', got[0], ll), ('kll', got[1], kll), ('gx', got[2], 0.25 * vx), ('gw', got[3], 0.25 * vw)):
            assert torch.isfinite(a).all(), (key, K, P, weighted)
            worst[key] = max(worst[key], rel_err(a, b))
        if weighted:
            z = w == 0
            assert not got[2].permute(0, 2, 1)[z].any(), (K, P)                  # no gradient into an unobserved pixel: exactly 0
            assert rel_err(got[3][z], 0.25 * vw[z]) < VGATE                       # ... and the raw map into its weight
    print(f'[kernels K={K} strict={strict}] ' + ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))
    assert all(v < VGATE for v in worst.values()), worst


def test_kernel_null_outputs_and_refusals():
    K, P = 2, 65
    x, w, dec = _kernel_inputs(K, P, True)
    xd, wd, dd = x.to(DEV), w.to(DEV), dec.to(DEV).contiguous()
    shapes = ((B, 3, P), (B, K, 3, P), (B, 3, P), (B, P))
    full = [torch.zeros(s, device=DEV) for s in shapes]
    _op(xd, wd, dd, K, P, 0, 1.0, 1, full)
    for keep in itertools.product((False, True), repeat=4):
        o = [torch.zeros(s, device=DEV) if k else None for s, k in zip(shapes, keep)]
        _op(xd, wd, dd, K, P, 0, 1.0, 1, o)
        assert all(t is None or torch.equal(t, f) for t, f in zip(o, full)), keep
    L = _lib.lib()
    for bad in (dict(K=17), dict(K=0), dict(P=0), dict(x=None), dict(dec=None)):
        rc = L.iodine_op_pixel_maps(None, _lib.ptr(bad.get('x', xd)), _lib.ptr(wd), _lib.ptr(bad.get('dec', dd)), B, bad.get('K', K), bad.get('P', P),
                                    SIGMA, 0, 1.0, *[_lib.ptr(t) for t in full], 1)
        assert rc == 1, bad                                                       # IODINE_ERR_INVALID, nothing launched


# ---- 2. a training step --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(arch_key):
    return G.inputs(ARCHS[arch_key], B)


@functools.lru_cache(maxsize=None)
def _state(arch_key):
    a = ARCHS[arch_key]
    params, x, eps = _inputs(arch_key)
    p64 = {k: v.double() for k, v in params.items()}
    pm, plv, hidden, _, _ = R.s_loop(x.double(), None, eps.double(), p64, a, False, R.as_sigma(SIGMA))
    return (pm.detach(), plv.detach(), hidden[0].reshape(B, a.slots, -1), hidden[1].reshape(B, a.slots, -1))


# name -> (architecture, keywords of the reference, options of the module)
CASES = {
    'base': ('tiny', {}, {}),
    'base_exact_fp32': ('tiny', {}, {'conv_precision': 0}),
    'k1': ('k1', {}, {}),
    'k16': ('k16', {}, {}),
    's12_generic': ('s12', {}, {}),
    'dsprites': ('dsprites', {}, {}),
    'padded_l6': ('padded', {}, {}),
    'pixel_weights': ('tiny', dict(w='4d'), {}),
    'iw_beta': ('tiny', dict(iw=(0.5, 0.0, 2.0), beta=0.5), {}),
    'clip': ('tiny', dict(clip=True), {}),
    'clip_frame_weights': ('tiny', dict(clip=True, w='5d', iw=(0.5, 0.0, 2.0), beta=0.5), {}),
    'clip_shared_weight': ('tiny', dict(clip=True, w='4d'), {}),
    'from_state': ('tiny', dict(state=True), {}),
    'chunked': ('tiny', dict(w='4d'), {'batch_cap': 1}),
}


def _case_inputs(case):
    arch_key, kw, _ = CASES[case]
    a = ARCHS[arch_key]
    _, x, eps = _inputs(arch_key)
    E = a.iters + 1
    x = moving_clip(x, E) if kw.get('clip') else x
    w = {None: None, '4d': W.pattern(B, a.img_size), '5d': W.clip_pattern(B, E, a.img_size)}[kw.get('w')]
    return a, x, eps, w


@functools.lru_cache(maxsize=None)
def _reference(case):
    arch_key, kw, _ = CASES[case]
    a, x, eps, w = _case_inputs(case)
    params, _, _ = _inputs(arch_key)
    p64 = {k: v.double() for k, v in params.items()}
    return G.train_step_grads(x.double(), eps.double(), p64, a, SIGMA, beta=kw.get('beta', 1.0), iw=kw.get('iw'), w=w,
                              init=_state(arch_key) if kw.get('state') else None)


def _model(case, options=None):
    arch_key, kw, opts = CASES[case]
    params, _, _ = _inputs(arch_key)
    m = make_hip_model(ARCHS[arch_key], params, options={**opts, **(options or {})})
    m.beta, m.iter_weights, m.sigma = kw.get('beta', 1.0), kw.get('iw'), SIGMA
    return m


def _call(case, m, x_grad=True, w_grad=True, **fwd):
    """one training step of ``case`` -> (loss, x leaf, w leaf or None)"""
    arch_key, kw, _ = CASES[case]
    _, x, eps, w = _case_inputs(case)
    xd = x.to(DEV).requires_grad_(x_grad)
    wd = None
    if w is not None:
        wd = w.float().to(DEV).requires_grad_(w_grad)
        fwd['weights'] = wd
    if kw.get('state'):
        fwd['state'] = tuple(t.float().to(DEV) for t in _state(arch_key))
    m.zero_grad(set_to_none=True)
    return m(xd, eps.to(DEV), **fwd), xd, wd


def _check(case, m, loss, xd, wd, tag):
    ref = _reference(case)
    ref_loss = ref['out']['loss'].item()
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), ref['grads'][n].numpy())), n) for n, p in m.named_parameters() if p.grad is not None)
    assert xd.grad is not None and xd.grad.shape == xd.shape and xd.grad.dtype == xd.dtype
    ex = rel_l2(xd.grad.cpu().numpy(), ref['gx'].numpy())
    ew = None
    if wd is not None:
        assert wd.grad is not None and wd.grad.shape == wd.shape
        ew = rel_l2(wd.grad.cpu().numpy(), ref['gw'].numpy())
    print(f'[{tag}] loss {loss.item():.6f} vs {ref_loss:.6f}; x.grad {ex:.2e}; weights.grad {"-" if ew is None else format(ew, ".2e")}; '
          f'worst parameter gradient {worst[1]} {worst[0]:.2e}')
    assert abs(loss.item() - ref_loss) <= VGATE * abs(ref_loss), tag
    assert ex < GATE, (tag, ex)
    assert ew is None or ew < GATE, (tag, ew)
    assert worst[0] < GATE, (tag, worst)


@pytest.mark.parametrize('case', list(CASES))
def test_input_grad_of_a_training_step(case):
    m = _model(case)
    loss, xd, wd = _call(case, m)
    loss.backward()
    torch.cuda.synchronize()
    _check(case, m, loss, xd, wd, case)
    kw = CASES[case][1]
    if kw.get('clip') and kw.get('iw'):                                     # the zero-weight evaluation: an exact zero for its frame
        assert not xd.grad[:, 1].any() and not wd.grad[:, 1].any()
    if kw.get('w') == '4d' and not kw.get('clip'):
        for i, (y0, x0) in enumerate(W.rectangles(B, BASE.img_size)):        # unobserved pixels get no gradient
            assert not xd.grad[i, :, y0:y0 + 6, x0:x0 + 5].any()


def test_weight_shapes_dtypes_and_a_float64_image():
    """the gradient comes back in the caller's shape and dtype: weights (B, S, S), an image in float64; bool weights stay data"""
    m = _model('pixel_weights')
    _, x, eps, w = _case_inputs('pixel_weights')
    ref = _reference('pixel_weights')
    xd = x.double().to(DEV).requires_grad_(True)
    wd = w.float().to(DEV)[:, 0].clone().requires_grad_(True)
    m(xd, eps.to(DEV), weights=wd).backward()
    assert xd.grad.dtype == torch.float64 and wd.grad.shape == (B, BASE.img_size, BASE.img_size)
    assert rel_l2(xd.grad.cpu().numpy(), ref['gx'].numpy()) < GATE and rel_l2(wd.grad.cpu().numpy(), ref['gw'][:, 0].numpy()) < GATE
    xd.grad = None
    m(xd, eps.to(DEV), weights=(w > 0).to(DEV)).backward()                   # a mask: x still gets its gradient
    assert xd.grad is not None and torch.isfinite(xd.grad).all()


def test_auxiliary_cotangents_leave_x_grad_unchanged():
    m = _model('base')
    loss, xd, _ = _call('base', m)
    loss.backward()
    plain = xd.grad.clone()
    T = BASE.iters
    loss, xd, _ = _call('base', m, attach_state=True, attach_frames=[0, T])
    g = torch.Generator().manual_seed(3)
    wm = torch.randn(m.mask.shape, generator=g).to(DEV)
    aux = (wm * m.mask).sum() + (m.frames['mask'][0] ** 2).sum() + m.frames['z'][1].sum()
    (loss + aux).backward()
    assert torch.equal(xd.grad, plain)


def test_sigma_leaf_and_image_at_the_same_time():
    m = _model('base')
    s = torch.tensor(SIGMA, dtype=torch.float32, device=DEV, requires_grad=True)
    _, x, eps, _ = _case_inputs('base')
    xd = x.to(DEV).requires_grad_(True)
    m.sigma = s
    loss = m(xd, eps.to(DEV))
    loss.backward()
    params, _, _ = _inputs('tiny')
    _, _, g_auto, _ = R.train_step_grads(x.double(), eps.double(), {k: v.double() for k, v in params.items()}, BASE, SIGMA)
    es = abs(s.grad.item() - g_auto.item()) / abs(g_auto.item())
    ex = rel_l2(xd.grad.cpu().numpy(), _reference('base')['gx'].numpy())
    print(f'[sigma + x] sigma.grad {es:.2e}; x.grad {ex:.2e}')
    assert es < GATE and ex < GATE


# ---- 3. elbo / weighted_elbo -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['elbo', 'weighted', 'chunked'])
def test_input_grad_of_elbo(how):
    params, x, eps = _inputs('tiny')
    p64 = {k: v.double() for k, v in params.items()}
    w = W.pattern(B, BASE.img_size) if how != 'elbo' else None
    ref = G.elbo_grads(x.double(), eps[0].double(), p64, BASE, SIGMA, beta=0.5, w=w)
    m = make_hip_model(BASE, params, options={'batch_cap': 1} if how == 'chunked' else None)
    m.beta, m.sigma = 0.5, SIGMA
    xd = x.to(DEV).requires_grad_(True)
    wd = None if w is None else w.float().to(DEV).requires_grad_(True)
    e = m.elbo(xd, eps[0].to(DEV)) if w is None else m.weighted_elbo(xd, wd, eps[0].to(DEV))
    (2.0 * e).backward()
    ex = rel_l2(xd.grad.cpu().numpy(), 2.0 * ref['gx'].numpy())
    ew = 0.0 if w is None else rel_l2(wd.grad.cpu().numpy(), 2.0 * ref['gw'].numpy())
    worst = max(rel_l2(*grad_views(n, p.grad.cpu().numpy(), 2.0 * ref['grads'][n].numpy())) for n, p in m.named_parameters() if p.grad is not None)
    print(f'[elbo {how}] elbo {e.item():.6f} vs {ref["terms"]["elbo"].item():.6f}; x.grad {ex:.2e}; weights.grad {ew:.2e}; worst parameter gradient {worst:.2e}')
    assert abs(e.item() - ref['terms']['elbo'].item()) <= VGATE * abs(ref['terms']['elbo'].item())
    assert ex < GATE and ew < GATE and worst < GATE
    # a call that ran without the option left nothing to read
    m(x.to(DEV), eps.to(DEV))
    assert _lib.lib().iodine_last_input_grad(m._handle, None, _lib.ptr(torch.empty_like(xd)), None) == 3       # IODINE_ERR_STATE
    assert b'input_grad' in _lib.lib().iodine_last_error(m._handle)


# ---- 4. nothing asked, nothing changed ------------------------------------------------------------------------------------------------
def test_options_off_change_no_bit():
    params, x, eps = _inputs('tiny')

    def snapshot(m, x_grad=False, maps=False):
        m.likelihood_maps = maps
        m.zero_grad(set_to_none=True)
        loss = m(x.to(DEV).requires_grad_(x_grad), eps.to(DEV))
        loss.backward()
        out = {'loss': loss.detach().clone(), 'terms': m.elbo_terms.clone()}
        out.update({'g.' + n: p.grad.clone() for n, p in m.named_parameters()})
        pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
        out.update(pred=pred.clone(), mask=mask.clone(), mean=mean.clone(), pm=m.posterior.mean.clone(), rterms=m.elbo_terms.clone())
        assert (m.log_likelihood is not None) == maps and (m.K_log_likelihood is not None) == maps
        return out

    m = make_hip_model(BASE, params)
    a = snapshot(m)                                                         # a handle that never heard of the options
    L = _lib.lib()
    bytes0 = [L.iodine_workspace_bytes(m._handle, B, mode) for mode in (0, 1, 2)]
    for x_grad, maps in ((True, False), (False, True), (True, True), (False, False)):
        b = snapshot(m, x_grad, maps)
        differ = [k for k in a if not torch.equal(a[k], b[k])]
        assert not differ, (x_grad, maps, differ)
        if x_grad:                                                          # the accumulators are part of the plan while the bit is set ...
            assert L.iodine_workspace_bytes(m._handle, B, 1) > bytes0[1]
    # ... and only then
    assert [L.iodine_workspace_bytes(m._handle, B, mode) for mode in (0, 1, 2)] == bytes0


# ---- 5. the likelihood maps --------------------------------------------------------------------------------------------------------------
def _maps_check(m, ll_ref, kll_ref, tag):
    assert m.log_likelihood.dtype == torch.float32 and not m.log_likelihood.requires_grad
    assert m.log_likelihood.shape == ll_ref.shape and m.K_log_likelihood.shape == kll_ref.shape
    e1, e2 = rel_err(m.log_likelihood.cpu(), ll_ref), rel_err(m.K_log_likelihood.cpu(), kll_ref)
    print(f'[maps {tag}] log_likelihood {e1:.1e}, K_log_likelihood {e2:.1e}')
    assert e1 < VGATE and e2 < VGATE, (tag, e1, e2)


def test_maps_after_elbo_forward_and_weights():
    params, x, eps = _inputs('tiny')
    p64 = {k: v.double() for k, v in params.items()}
    m = make_hip_model(BASE, params)
    m.sigma, m.likelihood_maps = SIGMA, True
    ref = G.elbo_grads(x.double(), eps[0].double(), p64, BASE, SIGMA)
    m.elbo(x.to(DEV), eps[0].to(DEV))
    _maps_check(m, ref['ll_px'], ref['k_ll'], 'elbo')
    total = m.log_likelihood.sum((1, 2, 3)).mean().item()
    print(f'[maps elbo] sum of the map {total:.6f} vs reported LL {m.elbo_terms[-1, 2].item():.6f}')
    assert abs(total - m.elbo_terms[-1, 2].item()) <= VGATE * abs(m.elbo_terms[-1, 2].item())
    plain = (m.log_likelihood.clone(), m.K_log_likelihood.clone())
    m.weighted_elbo(x.to(DEV), W.pattern(B, BASE.img_size).float().to(DEV), eps[0].to(DEV))
    assert torch.equal(m.log_likelihood, plain[0]) and torch.equal(m.K_log_likelihood, plain[1])          # raw under weights
    r = _reference('base')
    loss, _, _ = _call('base', m, x_grad=False)
    _maps_check(m, r['out']['ll_px'], r['out']['k_ll'], 'forward')
    m.likelihood_maps = False
    m.elbo(x.to(DEV), eps[0].to(DEV))
    assert m.log_likelihood is None and m.K_log_likelihood is None


@pytest.mark.parametrize('how', ['still', 'clip', 'chunked'])
def test_maps_after_reconstruct(how):
    params, x, eps = _inputs('tiny')
    p64 = {k: v.double() for k, v in params.items()}
    T = BASE.iters
    xc = moving_clip(x, T) if how == 'clip' else x
    _, _, _, ts, _ = R.s_loop(xc.double(), None, eps.double(), p64, BASE, False, R.as_sigma(SIGMA))
    m = make_hip_model(BASE, params, options={'batch_cap': 1} if how == 'chunked' else None)
    m.sigma, m.likelihood_maps = SIGMA, True
    m.reconstruct(xc.to(DEV), eps.to(DEV))
    _maps_check(m, ts[-1]['ll_px'].detach(), ts[-1]['k_ll'].detach(), 'reconstruct ' + how)


def test_last_likelihood_on_a_fresh_handle_is_refused():
    params, _, _ = _inputs('tiny')
    m = make_hip_model(BASE, params)
    h = m._sync_params(torch.device(DEV))
    S = BASE.img_size
    out = torch.empty(1, 3, S, S, device=DEV)
    assert _lib.lib().iodine_last_likelihood(h, None, 1, _lib.ptr(out), None) == 3                             # IODINE_ERR_STATE
    assert _lib.lib().iodine_last_input_grad(h, None, _lib.ptr(out), None) == 3


# ---- 6. graph mode -----------------------------------------------------------------------------------------------------------------------
def test_graph_mode_for_three_steps():
    eager, graphed = _model('base'), _model('base', {'graph': 1})
    for step in range(3):                                                   # eager, captured, replayed
        outs = []
        for m in (eager, graphed):
            loss, xd, _ = _call('base', m)
            loss.backward()
            torch.cuda.synchronize()
            outs.append((loss.detach().clone(), xd.grad.clone(), [p.grad.clone() for p in m.parameters()]))
        (l0, x0, g0), (l1, x1, g1) = outs
        assert torch.equal(l0, l1) and torch.equal(x0, x1), step
        assert all(torch.equal(u, v) for u, v in zip(g0, g1)), step
    assert graphed.profile_read('graph_replays')[1] > 0


# ---- 7. the engine's --learn-input-gain ------------------------------------------------------------------------------------------------
def test_engine_learns_input_gain(tmp_path):
    """six parameters in their own param group of the fused Adam, reached through x.grad: they move, the loss stays finite"""
    import numpy as np
    from iodine_amd import IODINE, engine
    from iodine_amd.data import make_dataloader
    from iodine_amd.model import arch_namespace
    from iodine_amd.optim import make_optimizer
    torch.manual_seed(0)
    m = IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))).to(DEV)
    opt = make_optimizer(m, base_lr=3e-3)
    gain = engine.InputGain(torch.device(DEV))
    opt.add_param_group({'params': list(gain.parameters()), 'lr': 3e-3, 'weight_decay': 0.0})
    dl = make_dataloader(engine.SyntheticScenes(8, 16), batch_size=4, shuffle=False)
    ck = str(tmp_path / 'model.pth')
    losses = engine.train(m, opt, dl, torch.device(DEV), max_steps=6, print_every=1000, checkpoint_path=ck, input_gain=gain)
    assert len(losses) == 6 and np.isfinite(losses).all()
    assert (gain.gain.detach() != 1).all() and (gain.offset.detach() != 0).all()
    assert all(int(opt.state[p]['step']) == 6 for p in gain.parameters())
    saved = torch.load(ck, map_location='cpu')['input_gain']
    assert torch.equal(saved['gain'], gain.gain.detach().cpu())
