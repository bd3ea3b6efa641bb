"""Gradients into the image and the pixel weights, and the likelihood maps, without a device: the closed form the library implements
(input_grad_reference.py) against float64 autograd; the maps against the oracle; the ABI entries, the option and the module's host side.

Tiny architecture (O.tiny_arch(): K = 3, T = 2, S = 16, L = 8; B = 2).  Measured: closed form vs autograd <= 3e-16 rel-L2 on every case."""
import os
import re

import pytest
import torch

from iodine_amd import IODINE, _args, _lib, engine
from oracle import iodine_oracle as O
from util import hip_arch, rel_l2

import input_grad_reference as G
import sigma_reference as R
import weights_reference as W
from clip_reference import moving_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = O.tiny_arch()
B = 2
F64 = torch.float64


@pytest.fixture(scope='module')
def f64_inputs():
    return G.inputs(ARCH, B, dtype=F64)


def _state(params, x, eps):
    pm, plv, hidden, _, _ = R.s_loop(x, None, eps, params, ARCH, False, R.as_sigma(0.1))
    return (pm.detach(), plv.detach(), hidden[0].reshape(B, ARCH.slots, -1), hidden[1].reshape(B, ARCH.slots, -1))


# ---- 1. the interface (fails on the parent: the entries do not exist) -------------------------------------------------------------------
def test_header_binding_and_pad_adapter_carry_the_new_entries():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    api = open(os.path.join(ROOT, 'iodine_amd', 'csrc', 'iodine_api.cpp')).read()
    pad = open(os.path.join(ROOT, 'iodine_amd', 'csrc', 'iodine_pad.cpp')).read()
    assert '"input_grad"' in header and 'strcmp(key, "input_grad")' in api
    assert re.search(r'int iodine_last_input_grad\(iodine_handle\* h, void\* stream, float\* g_x, float\* g_w\);', header)
    assert re.search(r'int iodine_last_likelihood\(iodine_handle\* h, void\* stream, int count, float\* log_likelihood, float\* k_log_likelihood\);',
                     header)
    assert re.search(r'int iodine_op_pixel_maps\(void\* stream, const float\* x_nchw, const float\* w_or_null, const float\* dec_out_nhwc4', header)
    assert header.count('iodine.py:210-2') >= 3                             # each new entry cites the reference's lines
    for name in ('iodine_last_input_grad', 'iodine_last_likelihood', 'iodine_op_pixel_maps'):
        assert name in _lib.EXPORTS, name
    for name in ('pad_last_input_grad', 'pad_last_likelihood'):
        assert name in pad and name in api, name
    assert 'iodine_last_input_grad(h->shim->inner' in pad and 'iodine_last_likelihood(h->shim->inner' in pad
    L = _lib.lib()
    assert all(hasattr(L, n) for n in ('iodine_last_input_grad', 'iodine_last_likelihood', 'iodine_op_pixel_maps'))
    assert L.iodine_abi_version() == 3                                      # additive
    assert L.iodine_last_input_grad(None, None, None, None) == 1            # IODINE_ERR_INVALID: no handle
    assert L.iodine_last_likelihood(None, None, 1, None, None) == 1
    # the kernel-level entry refuses on the host, without a launch: slots 17, no image
    assert L.iodine_op_pixel_maps(None, None, None, None, 1, 3, 16, 0.1, 0, 1.0, None, None, None, None, 1) == 1
    one = torch.zeros(4)
    assert L.iodine_op_pixel_maps(None, _lib.ptr(one), None, _lib.ptr(one), 1, 17, 1, 0.1, 0, 1.0, None, None, None, None, 1) == 1


# ---- 2. the closed form is the gradient ------------------------------------------------------------------------------------------------
CASES = {
    'still': {},
    'weights': dict(w='4d'),
    'iw_beta': dict(iw=(0.5, 0.0, 2.0), beta=0.5),
    'clip': dict(clip=True),
    'clip_frame_weights': dict(clip=True, w='5d', iw=(0.5, 0.0, 2.0), beta=0.5),
    'clip_shared_weight': dict(clip=True, w='4d'),
    'from_state': dict(state=True),
}


@pytest.mark.parametrize('case', list(CASES))
def test_closed_form_equals_autograd(f64_inputs, case):
    params, x, eps = f64_inputs
    kw = CASES[case]
    E = ARCH.iters + 1
    xc = moving_clip(x, E) if kw.get('clip') else x
    w = {None: None, '4d': W.pattern(B, ARCH.img_size), '5d': W.clip_pattern(B, E, ARCH.img_size)}[kw.get('w')]
    r = G.train_step_grads(xc, eps, params, ARCH, 0.1, beta=kw.get('beta', 1.0), iw=kw.get('iw'), w=w,
                           init=_state(params, x, eps) if kw.get('state') else None)
    assert r['gx'].shape == xc.shape and float(r['gx'].abs().max()) > 0
    ex = rel_l2(r['cx'].numpy(), r['gx'].numpy())
    ew = rel_l2(r['cw'].numpy(), r['gw'].numpy()) if w is not None else 0.0
    print(f'[{case}] closed form vs autograd: x {ex:.1e}, w {ew:.1e}')
    assert ex < 1e-12 and ew < 1e-12
    if kw.get('iw'):                                                        # the zero-weight evaluation contributes an exact zero
        if kw.get('clip'):
            assert not r['gx'][:, 1].any() and not r['cx'][:, 1].any() and not r['gw'][:, 1].any()
    if w is not None and w.dim() == 4:                                      # the zero rectangle: no gradient into the image, the raw map into w
        for i, (y0, x0) in enumerate(W.rectangles(B, ARCH.img_size)):
            assert not r['gx'][i, ..., y0:y0 + 6, x0:x0 + 5].any()
            assert r['gw'][i, ..., y0:y0 + 6, x0:x0 + 5].abs().min() > 0


def test_auxiliary_terms_add_exactly_nothing(f64_inputs):
    """mean, mask, z, lambda_T and the LSTM state depend on x only through detached inputs"""
    params, x, eps = f64_inputs
    aux = lambda o: ((o['final_mask'] ** 2).sum() + o['final_z'].sum() + o['post_mean'].sum() + o['hidden'][0].sum()
                     + o['terms'][0]['mask'].sum() + o['terms'][1]['mean'].sum())
    a = G.train_step_grads(x, eps, params, ARCH, 0.1)
    b = G.train_step_grads(x, eps, params, ARCH, 0.1, aux=aux)
    assert torch.equal(a['gx'], b['gx'])


def test_elbo_closed_form(f64_inputs):
    params, x, eps = f64_inputs
    w = W.pattern(B, ARCH.img_size)
    r = G.elbo_grads(x, eps[0], params, ARCH, 0.1, beta=0.5, w=w)
    assert rel_l2(r['cx'].numpy(), r['gx'].numpy()) < 1e-12 and rel_l2(r['cw'].numpy(), r['gw'].numpy()) < 1e-12


def test_float32_floor_of_the_reference():
    """the float32 oracle's own distance from float64 is far below a third of GATE = 1e-3: the GPU tests hold the plain gates"""
    p, x, eps = G.inputs(ARCH, B)
    a = G.train_step_grads(x, eps, p, ARCH, 0.1)
    b = G.train_step_grads(x.double(), eps.double(), {k: v.double() for k, v in p.items()}, ARCH, 0.1)
    e = rel_l2(a['gx'].numpy(), b['gx'].numpy())
    print(f'float32 vs float64 reference, d loss / d x: {e:.1e}')
    assert e < 1e-3 / 3


# ---- 3. the maps are the oracle's ----------------------------------------------------------------------------------------------------------
def test_maps_equal_the_oracle(f64_inputs):
    params, x, eps = f64_inputs
    K = ARCH.slots
    pm = params['posterior.init_mean'][None, None].repeat(B, K, 1)
    plv = params['posterior.init_logvar'][None, None].repeat(B, K, 1)
    t = O.elbo_terms(x, pm, plv, eps[0], params, ARCH)
    r = G.elbo_grads(x, eps[0], params, ARCH, ARCH.sigma, w=W.pattern(B, ARCH.img_size))          # raw under weights
    assert torch.allclose(r['ll_px'], t['ll_px'].detach(), rtol=1e-13, atol=0) and torch.allclose(r['k_ll'], t['k_ll'].detach(), rtol=1e-13, atol=0)
    assert t['ll_px'].shape == (B, 3, ARCH.img_size, ARCH.img_size) and t['k_ll'].shape == (B, K, 3, ARCH.img_size, ARCH.img_size)
    assert abs(float(t['ll_px'].mean(0).sum() - t['ll'])) <= 1e-12 * abs(float(t['ll']))
    # ... and the kernel-level restatement on a raw decoder output agrees with both
    mean, logits = O.decoder(O.sample(pm, plv, eps[0]), params, ARCH)
    P = ARCH.img_size ** 2
    dec = torch.cat([torch.logit(mean), logits], dim=2).reshape(B, K, 4, P).permute(0, 1, 3, 2)
    w = W.pattern(B, ARCH.img_size)
    ll, kll, vx, vw = G.kernel_reference(x.reshape(B, 3, P), w.reshape(B, P), dec, ARCH.sigma)
    assert rel_l2(ll.numpy(), t['ll_px'].detach().reshape(B, 3, P).numpy()) < 1e-9
    assert rel_l2(kll.numpy(), t['k_ll'].detach().reshape(B, K, 3, P).numpy()) < 1e-9
    assert rel_l2((vx / B).numpy(), r['cx'].reshape(B, 3, P).numpy()) < 1e-9
    assert rel_l2((vw / B).numpy(), r['cw'].reshape(B, P).numpy()) < 1e-9


# ---- 4. the module's host side ---------------------------------------------------------------------------------------------------------------
def test_module_defaults_and_detached_helpers():
    m = IODINE(hip_arch(ARCH))
    assert m.likelihood_maps is False and m.log_likelihood is None and m.K_log_likelihood is None
    S = ARCH.img_size
    x = torch.rand(B, 3, S, S, requires_grad=True)
    w = torch.rand(B, 1, S, S, requires_grad=True)
    wc = _args.check_weights(w, x, S, 'forward')
    assert not wc.requires_grad and wc.dtype == torch.float32 and wc.shape == (B, S, S)          # the helper keeps returning data
    assert not _args.check_x(x, 3, S).requires_grad
    xi, wi = m._grad_inputs(x, w, _args.check_x(x, 3, S), wc)
    assert xi is x and wi is w                                              # the node takes the caller's tensors ...
    with torch.no_grad():
        xi, wi = m._grad_inputs(x, w, _args.check_x(x, 3, S), wc)
        assert xi is not x and wi is wc                                     # ... under grad mode only
    mask = torch.ones(B, S, S, dtype=torch.bool)
    assert m._grad_inputs(x.detach(), mask, x.detach(), _args.check_weights(mask, x, S, 'forward'))[1].dtype == torch.float32
    assert 'receives ``d loss / d w``; otherwise weights are data' in __import__('iodine_amd.model').model.__doc__


def test_parser_takes_the_flag_and_the_gain_is_six_parameters():
    ap = engine.make_parser()
    assert ap.parse_args(['--learn-input-gain']).learn_input_gain and not ap.parse_args([]).learn_input_gain
    g = engine.InputGain('cpu')
    assert sum(p.numel() for p in g.parameters()) == 6
    x = torch.rand(2, 3, 4, 4)
    assert torch.equal(g(x), x) and g(x).requires_grad                      # starts as the identity, attached to the six
    clip = torch.rand(2, 3, 3, 4, 4)
    assert torch.equal(g(clip), clip)


def test_train_steps_the_gain_through_x_grad():
    """a stand-in model whose loss depends on x: the six parameters move with the model's in one optimiser step"""
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))
            self.sigma = 0.1

        def forward(self, x):
            return self.w * (x ** 2).sum()

    m, g = Model(), engine.InputGain('cpu')
    opt = torch.optim.SGD([{'params': list(m.parameters())}, {'params': list(g.parameters())}], lr=0.01)
    before = [p.detach().clone() for p in g.parameters()]
    losses = engine.train(m, opt, [(torch.ones(1, 3, 2, 2),)] * 3, 'cpu', 3, log=lambda *a: None, input_gain=g)
    assert all(not torch.equal(p.detach(), b) for p, b in zip(g.parameters(), before))
    assert losses[0] > losses[-1]
