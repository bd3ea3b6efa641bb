"""The per-pixel mixture kernels' test entry point and reference, without a device: the float64 reference of tests/pixel_reference.py against
the oracle (O.elbo_terms, O.input_encoding, O.pixel_closed_form) and against autograd with sigma as a leaf (sigma_reference) on the tiny
architecture; the header, the binding and the refusals of iodine_op_pixel_encode; the conditioning of the case table: for every (case, tensor)
that tests/test_gpu_pixel.py compares, the float32 evaluation of the reference on the CPU is within a quarter of the gates' cap of float64.

Measured (CPU float32 against float64, worst over the cases, per (image, slot, channel) plane relative to the plane's largest element; scalars
relative to themselves): g 2.3e-6, sgrad 2.2e-6, LN(g_mean) 2.3e-6, mask_posterior 1.6e-6, LN(g_mask) 1.1e-6, LN(likelihood) 9.6e-7,
LN(leave-one-out) 8.6e-7, scal 4.8e-7, the statistics <= 4.5e-7, ll_img, kl <= 3.4e-7, pred, mask, mean <= 3.0e-7; image, logits and
coordinates 0.  The reference against the oracle: the ELBO terms and maps to 1e-12, gradients to 1e-10, the normalised channels to 1e-9."""
import ctypes as C
import os
import re

import pytest
import torch

from iodine_amd import _lib
from oracle import iodine_oracle as O

import pixel_reference as R
import sigma_reference as SR
import weights_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---- 1. the interface -----------------------------------------------------------------------------------------------------------------------
def _call(L, x, w, dec, pm, plv, lin, B, K, S, Lat, sigma, beta, flags, chmask, repeat, outs):
    arr = None if outs is None else (C.c_void_p * 12)(*[None if t is None else t.data_ptr() for t in outs])
    return L.iodine_op_pixel_encode(None, _lib.ptr(x), _lib.ptr(w), _lib.ptr(dec), _lib.ptr(pm), _lib.ptr(plv), _lib.ptr(lin), B, K, S, Lat, sigma, beta,
                                    flags, chmask, repeat, arr)


def test_header_binding_and_refusals():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    ops = open(os.path.join(ROOT, 'iodine_amd', 'csrc', 'iodine_testops.cpp')).read()
    assert re.search(r'int iodine_op_pixel_encode\(void\* stream, const float\* x_nchw, const float\* w_or_null, const float\* dec_out_nhwc4, '
                     r'const float\* pm, const float\* plv,\s+const float\* lin, int batch, int slots, int size, int latent, float sigma, float beta, '
                     r'int flags, unsigned chmask,\s+int repeat, float\* const\* out\);', header)
    assert 'iodine_op_pixel_encode' in _lib.EXPORTS
    # the production launchers, in the library's order
    body = ops[ops.index('int iodine_op_pixel_encode('):ops.index('int iodine_op_conv3x3_wgrad_f32(')]
    order = [body.index(n) for n in ('OpScratch scr(', 'launch_x_to_nhwc4(', 'launch_pixel_pass1(', 'launch_pixel_finalize_elbo(',
                                     'launch_pixel_sigma_grad(', 'launch_pixel_pass2(', 'launch_final_out(', 'return op_done(')]
    assert order == sorted(order)
    # ... where op_done synchronises and the scratch frees itself when the entry returns, behind that wait
    assert 'hipStreamSynchronize(' in ops[ops.index('int op_done('):ops.index('constexpr size_t META_BYTES')]
    assert 'hipFree(' in ops[ops.index('~OpScratch()'):].split('\n')[0]
    L = _lib.lib()
    assert hasattr(L, 'iodine_op_pixel_encode') and L.iodine_abi_version() == 3              # additive
    # refused on the host, before anything is allocated or launched (host tensors: a launch would not survive them)
    B, K, S, Lat = 1, 2, 2, 3
    t = lambda *s: torch.zeros(*s)
    x, dec, pm, plv, lin = t(B, 3, S * S), t(B, K, S * S, 4), t(B, K, Lat), t(B, K, Lat), t(S)
    outs = [t(64) for _ in range(12)]
    good = dict(x=x, w=None, dec=dec, pm=pm, plv=plv, lin=lin, B=B, K=K, S=S, Lat=Lat, sigma=0.1, beta=1.0, flags=0, chmask=R.CH_FULL, repeat=1,
                outs=outs)
    bad = [dict(K=0), dict(K=17), dict(K=-1), dict(S=0), dict(S=-3), dict(B=0), dict(Lat=0), dict(repeat=0), dict(sigma=0.0), dict(sigma=-0.1),
           dict(sigma=float('nan')), dict(x=None), dict(dec=None), dict(pm=None), dict(plv=None), dict(lin=None), dict(outs=None),
           dict(S=46341), dict(B=1 << 20, S=64), dict(K=16, S=2600),                          # an index product >= 2^31
           dict(outs=outs[:6] + [None] + outs[7:])]                                          # enc_sh without enc
    bad += [dict(outs=outs[:j] + [None] + outs[j + 1:]) for j in range(5)]                   # g, lnstat, ll_img, img_terms, scal are required
    for b in bad:
        assert _call(L, **{**good, **b}) == 1, b                                             # IODINE_ERR_INVALID
    assert b'iodine_op_pixel_encode' in L.iodine_last_error(None)


# ---- 2. the reference is the oracle's arithmetic --------------------------------------------------------------------------------------------
ARCH = O.tiny_arch()                                                                          # K = 3, S = 16, L = 8
B = 2


@pytest.fixture(scope='module')
def tiny():
    params, x, eps = SR.inputs(ARCH, B, dtype=F64)
    K, S = ARCH.slots, ARCH.img_size
    g = torch.Generator().manual_seed(11)
    pm = params['posterior.init_mean'][None, None].repeat(B, K, 1) + 0.3 * torch.randn(B, K, ARCH.dim_latent, generator=g, dtype=F64)
    plv = params['posterior.init_logvar'][None, None].repeat(B, K, 1) + 0.3 * torch.randn(B, K, ARCH.dim_latent, generator=g, dtype=F64)
    t = O.elbo_terms(x, pm, plv, eps[0], params, ARCH)
    t = {k: v.detach() for k, v in t.items()}
    P = S * S
    dec = torch.cat([torch.logit(t['mean']), t['logits']], dim=2).reshape(B, K, 4, P).permute(0, 1, 3, 2).contiguous()
    inp = dict(x=x.reshape(B, 3, P), w=None, dec=dec, pm=pm, plv=plv, lin=torch.linspace(-1, 1, S), sigma=ARCH.sigma, beta=1.0, use_ln=1)
    return params, x, eps, pm, plv, t, inp


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


def test_reference_equals_elbo_terms_and_closed_form(tiny):
    params, x, eps, pm, plv, t, inp = tiny
    K, S = ARCH.slots, ARCH.img_size
    r = R.evaluate(inp)
    assert _close(r['scal'], torch.stack([t['elbo'], t['kl'], t['ll']]))
    assert _close(r['ll_img'].mean(), t['ll']) and _close(r['kl_img'].mean(), t['kl'])
    assert _close(r['ll_px'].reshape(B, 3, S, S), t['ll_px']) and _close(r['k_ll'].reshape(B, K, 3, S, S), t['k_ll'])
    assert _close(r['mask'].reshape(B, K, 1, S, S), t['mask']) and _close(r['mean'].reshape(B, K, 3, S, S), t['mean'], 1e-10)
    assert _close(r['pred'].reshape(B, 3, S, S), (t['mask'] * t['mean']).sum(dim=1), 1e-10)
    cf = O.pixel_closed_form(x, t['mean'], t['logits'], ARCH.sigma)
    assert _close(r['g_mean'].reshape(B, K, 3, S, S), cf['g_mean'], 1e-10) and _close(r['g_mask'].reshape(B, K, 1, S, S), cf['g_mask'], 1e-10)
    g = r['g'].permute(0, 1, 3, 2).reshape(B, K, 4, S, S)
    assert _close(g[:, :, :3], cf['d_rgb'], 1e-10) and _close(g[:, :, 3:], cf['d_logit'], 1e-10)


def test_reference_equals_input_encoding(tiny):
    params, x, eps, pm, plv, t, inp = tiny
    K, S = ARCH.slots, ARCH.img_size
    r = R.evaluate(inp)
    z = torch.zeros_like(pm)
    g_mean, g_mask = r['g_mean'].reshape(B, K, 3, S, S), r['g_mask'].reshape(B, K, 1, S, S)
    enc, _ = O.input_encoding(x, t, pm, plv, g_mean, g_mask, z, z, ARCH)                      # (B, K, 17, S, S)
    mine = r['enc'].permute(0, 1, 3, 2).reshape(B, K, 17, S, S)
    for c in range(17):
        assert _close(mine[:, :, c], enc[:, :, c], 1e-9), (c, R.CHANNELS[c])
    # the statistics are those of the oracle's layernorm: re-normalising with them gives its channels
    loo_stat = r['lnstat'][:, :, 4:6]
    k_like = torch.exp(t['k_ll'].sum(dim=2, keepdim=True))
    loo = ((t['mask'] * k_like).sum(dim=1, keepdim=True) - t['mask'] * k_like) / (1 - t['mask'] + 1e-5)
    assert _close((loo - loo_stat[..., 0, None, None, None]) * loo_stat[..., 1, None, None, None], enc[:, :, 14:15], 1e-9)
    assert _close(r['lnstat'][:, :, 0], g_mean.mean(dim=(2, 3, 4)), 1e-10)                      # 3 P values
    assert _close(1 / r['lnstat'][:, :, 3] - 1e-5, g_mask.std(dim=(2, 3, 4), unbiased=False), 1e-9)
    # option stable_encoding: the reference's channel wherever nothing underflows
    assert _close(r['mask_post_stable'], r['enc'][..., 8], 1e-9)
    # without layer-norm the statistics are exactly {0, 1} and the channels raw
    raw = R.evaluate({**inp, 'use_ln': 0})
    assert torch.equal(raw['lnstat'], torch.tensor([0.0, 1.0], dtype=F64).repeat(B, K, 4))
    assert _close(raw['enc'][..., 12], r['g_mask'], 1e-12)


def test_weights_beta_and_sigma_grad_equal_autograd(tiny):
    """the weighted objective, beta and d LL / d sigma against sigma_reference.s_terms with sigma as a leaf"""
    params, x, eps, pm, plv, t, inp = tiny
    K, S = ARCH.slots, ARCH.img_size
    w = W.pattern(B, S)                                                                       # (B, 1, S, S), a zero rectangle per image
    sigma = SR.as_sigma(0.25, requires_grad=True)
    pl, pv = pm.clone().requires_grad_(True), plv.clone().requires_grad_(True)
    s = SR.s_terms(x, w, pl, pv, eps[0], params, ARCH, sigma, beta=0.5)
    g_auto, = torch.autograd.grad(s['ll'], sigma, retain_graph=True)
    g_mean, g_mask = torch.autograd.grad(B * s['elbo'], [s['mean'], s['mask']])
    r = R.evaluate({**inp, 'w': w.reshape(B, S * S), 'sigma': 0.25, 'beta': 0.5})
    assert _close(r['sgrad'][0], g_auto) and _close(r['scal'], torch.stack([s['elbo'], s['kl'], s['ll']]).detach())
    assert _close(r['g_mean'].reshape(B, K, 3, S, S), g_mean, 1e-10) and _close(r['g_mask'].reshape(B, K, 1, S, S), g_mask, 1e-10)
    zero = (w == 0).reshape(B, S * S)
    assert zero.any() and not r['g'].permute(0, 2, 1, 3)[zero].any()                          # no gradient from an unobserved pixel


def test_constant_planes_of_a_single_slot_are_stated_as_zero():
    r, _ = R.case_reference('near_k1_s17')
    assert not r['enc'][..., 12].any() and not r['enc'][..., 14].any() and bool((r['enc'][..., 8] == 1).all())
    assert not r['g'][..., 3].any()
    rw, _ = R.case_reference('near_k1_s9_w_kl3')
    assert rw['enc'][..., 12].abs().max() > 1 and not rw['enc'][..., 14].any()                # weighted: LN(g_mask) is a real comparison


# ---- 3. the case table ----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_paths():
    cs = R.CASES.values()
    assert {c['K'] for c in cs} == {1, 2, 3, 7, 11, 16}
    assert {c['S'] for c in cs} == {1, 2, 5, 8, 9, 16, 17, 23, 33, 64, 65, 68}
    assert {c['B'] for c in cs} == {1, 2, 3, 300}
    assert {3, 56, 448, 1024} <= {c['K'] * c['L'] for c in cs}
    assert {c['beta'] for c in cs} == {1.0, 0.5} and {c['use_ln'] for c in cs} == {0, 1}
    assert any(c['K'] == 16 and c['S'] * c['S'] > 512 for c in cs)                            # 99 statistics on several blocks
    assert any(c['K'] == 1 and c['weighted'] for c in cs) and any(c['K'] == 1 and not c['weighted'] for c in cs)
    assert {c['sigma'] for c in cs if c['family'] == 'far'} == {R.f32(0.1), R.f32(0.3)}
    assert 16 <= len(R.CASES) <= 20
    # the exclusions are the table's: by family and size, by name
    assert R.excluded('far_k2_s9') == R.FAR_EXCLUDED and R.excluded('far_k2_s9', 1) == R.FAR_EXCLUDED_STABLE
    assert R.excluded('near_k2_s5') == () and set(R.excluded('raw_k3_s1')) == set(R.LN_GROUPS + R.STATS)


def test_inputs_are_well_conditioned():
    """for every (case, tensor) compared on the device the float32 evaluation on the CPU is within a quarter of the cap of float64: a case
    that misses this is a badly chosen input"""
    worst = {}
    for case in R.CASES:
        _, errs = R.case_reference(case)
        for stable, e in errs.items():
            bad = {k: v for k, v in e.items() if not v <= R.GATE_CAP / 4}
            assert not bad, (case, stable, bad)
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
        compared = set(errs[0])
        assert {'g', 'll_img', 'kl_img', 'scal', 'sgrad', 'pred', 'mask', 'mean', 'logits', 'image', 'means', 'mask_logits', 'coord'} <= compared, case
        if R.CASES[case]['family'] == 'near' and R.CASES[case]['S'] >= 5:
            assert compared == set(R.SCALARS + R.PLANES + R.GROUPS + R.STATS), case              # all 17 channels and all four statistics
        assert 'mask_posterior' in errs[1]                                                    # the stable channel everywhere
    print('[pixel] CPU fp32 against fp64, worst over the cases: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    assert worst == R.cpu_floor()
    g4, g16 = R.gates(1), R.gates(0)
    assert all(g4[k] <= g16[k] <= R.GATE_CAP for k in g4)
