"""``model.likelihood = 'joint'`` without a device: the closed forms the kernels implement (pixel_terms.h, JOINT) against autograd of the
float64 reference (tests/joint_reference.py), the relation of the two forms (equal for one slot, different for more), the oracle under the
patch, the float32 floor that defines the gates of tests/test_gpu_joint.py, and the wrapper's plumbing (attribute, option, session, engine
flag) against a recording stub of the library."""
import contextlib
import math

import pytest
import torch

import joint_reference as J
import pixel_reference as R
import sigma_reference as SR
from iodine_amd import _lib, _session
from oracle import iodine_oracle as O

F64 = torch.float64


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


def _scene(K, weighted, B=2, S=5, sigma=0.1, seed=0):
    """float64 leaves of one evaluation: x (B, 3, P), w (B, P) or None, mean (B, K, 3, P), mask (B, K, 1, P)"""
    inp = R.make_inputs('near', B, K, S, 4, sigma, 1.0, 1, weighted, 0.5)
    dec = inp['dec'].double()
    mean = torch.sigmoid(dec[..., :3]).permute(0, 1, 3, 2).contiguous()
    mask = torch.softmax(dec[..., 3][:, :, None], dim=1)
    return inp['x'].double(), None if inp['w'] is None else inp['w'].double(), mean, mask


# ---- 1. the closed forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weighted', [False, True], ids=['unweighted', 'weighted'])
@pytest.mark.parametrize('K', [1, 2, 7, 16])
def test_closed_forms_equal_autograd(K, weighted):
    """g1, g2, d LL / d x, d LL / d w and sigma d LL / d sigma as pixel_terms.h orders them, against autograd of
    LL = sum_b sum_p w_p logsumexp_k(log(m_k + 1e-12) + sum_c l_kc) in float64"""
    x, w, mean, mask = _scene(K, weighted)
    sigma = 0.1
    xl, ml, kl = x.clone().requires_grad_(True), mean.clone().requires_grad_(True), mask.clone().requires_grad_(True)
    wl = (torch.ones_like(x[:, 0]) if w is None else w.clone()).requires_grad_(True)
    sl = torch.tensor(sigma, dtype=F64, requires_grad=True)
    k_ll = -(xl[:, None] - ml) ** 2 / (2 * sl ** 2) - torch.log(sl) - 0.5 * math.log(2 * math.pi)
    ll_px = J.joint_ll_px(kl, k_ll)                                       # (B, 1, P)
    total = (wl[:, None] * ll_px).sum()
    g_mean, g_mask, g_x, g_w, g_s = torch.autograd.grad(total, [ml, kl, xl, wl, sl])
    cf = J.closed_form(x, w, mean, mask, sigma)
    assert _close(cf['ll_px'], ll_px.detach())
    assert _close(cf['g1'], g_mean, 1e-11) and _close(cf['g2'], g_mask, 1e-11)
    assert _close(cf['gx'], g_x, 1e-11) and _close(cf['gw'], g_w, 1e-12)
    assert _close(cf['sgrad_sigma'].sum(), g_s * sigma, 1e-10)
    assert _close(cf['r'].sum(dim=1), (torch.ones_like(x[:, :1]) if w is None else w[:, None]), 1e-12)       # sum_k r_k = w
    if weighted:
        zero = w == 0
        assert zero.any() and not cf['g1'].permute(0, 3, 1, 2)[zero].any() and not cf['g2'].permute(0, 3, 1, 2)[zero].any()


# ---- 2. the two forms ----------------------------------------------------------------------------------------------------------------------
def test_one_slot_both_forms_agree():
    """K = 1: the forms differ only by 2 log(1 + 1e-12) per pixel"""
    for case in ('near_k1_s9_w_kl3', 'near_k1_s17'):
        inp = R.case_inputs(case)
        a, b = R.evaluate(inp), J.evaluate(inp)
        assert b['ll_px'].shape == (inp['x'].shape[0], 1, inp['x'].shape[2])
        assert _close(b['ll_px'][:, 0], a['ll_px'].sum(dim=1), 1e-9) and _close(b['ll_img'], a['ll_img'], 1e-9)
        assert _close(b['g'][..., :3], a['g'][..., :3], 1e-9) and _close(b['sgrad'], a['sgrad'], 1e-9)


def test_three_slots_the_forms_differ():
    """... so the two modes can never silently be the same code: more than 1 % apart in the likelihood and in its gradient"""
    inp = R.case_inputs('near_k3_s23_w_beta')
    a, b = R.evaluate(inp), J.evaluate(inp)
    rel = lambda u, v: float((u - v).abs().max() / v.abs().max())
    assert rel(b['ll_img'], a['ll_img']) > 0.01 and rel(b['g'], a['g']) > 0.01 and rel(b['sgrad'], a['sgrad']) > 0.01
    # what the form must not reach: channels 8 and 14 (joint over RGB in the reference already), the decode
    for k in ('pred', 'mask', 'mean', 'logits', 'kl_img', 'k_ll', 'mask_post_stable'):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a['enc'][..., 8], b['enc'][..., 8]) and torch.equal(a['enc'][..., 14], b['enc'][..., 14])
    assert torch.equal(a['lnstat'][..., 4:6], b['lnstat'][..., 4:6])


# ---- 3. the oracle under the patch -----------------------------------------------------------------------------------------------------------
ARCH = O.tiny_arch()
B = 2


def test_patched_oracle_runs_the_joint_model():
    params, x, eps = SR.inputs(ARCH, B, dtype=F64)
    plain, _ = O.train_step_grads(x, eps, params, ARCH)
    with J.patched():
        out, grads = O.train_step_grads(x, eps, params, ARCH)
        rec = O.reconstruct(x, eps, params, ARCH)
        det, gd, gs, _ = SR.train_step_grads(x, eps, params, ARCH, ARCH.sigma)
    assert O.elbo_terms is not J.joint_elbo_terms and SR.s_terms is not J.joint_s_terms                # the patch is gone
    assert abs(float(out['loss'] - plain['loss'])) > 0.01 * abs(float(plain['loss']))
    assert rec['lls'].shape == (ARCH.iters,) and all(torch.isfinite(g).all() for g in grads.values())
    # sigma_reference's restatement under its patch is the oracle under its patch
    assert _close(det['loss'], out['loss']) and all(_close(gd[n], grads[n], 1e-9) for n in grads)
    assert torch.isfinite(gs)
    # the evaluation of one scene: joint_reference.evaluate is joint_elbo_terms
    K, S, P = ARCH.slots, ARCH.img_size, ARCH.img_size ** 2
    pm = params['posterior.init_mean'][None, None].repeat(B, K, 1)
    plv = params['posterior.init_logvar'][None, None].repeat(B, K, 1)
    t = {k: v.detach() for k, v in J.joint_elbo_terms(x, pm, plv, eps[0], params, ARCH).items()}
    dec = torch.cat([torch.logit(t['mean']), t['logits']], dim=2).reshape(B, K, 4, P).permute(0, 1, 3, 2).contiguous()
    r = J.evaluate(dict(x=x.reshape(B, 3, P), w=None, dec=dec, pm=pm, plv=plv, lin=torch.linspace(-1, 1, S), sigma=ARCH.sigma, beta=1.0, use_ln=1))
    assert t['ll_px'].shape == (B, 1, S, S)
    assert _close(r['scal'], torch.stack([t['elbo'], t['kl'], t['ll']])) and _close(r['ll_px'].reshape(B, 1, S, S), t['ll_px'])
    z = torch.zeros_like(pm)
    enc, _ = O.input_encoding(x, t, pm, plv, r['g_mean'].reshape(B, K, 3, S, S), r['g_mask'].reshape(B, K, 1, S, S), z, z, ARCH)
    mine = r['enc'].permute(0, 1, 3, 2).reshape(B, K, 17, S, S)
    for c in range(17):
        assert _close(mine[:, :, c], enc[:, :, c], 1e-9), (c, R.CHANNELS[c])


# ---- 4. the float32 floor: what the gates of the GPU tests are multiples of --------------------------------------------------------------------
def test_float32_floor_of_the_joint_reference():
    """every compared (case, tensor) is conditioned to half the cap in float32 on the CPU - a kernel at twice the reference's own float32
    error still passes a capped gate; the comparison covers what pixel_reference covers for the case.  (test_pixel_cpu.py asserts a
    quarter for the per-channel form.  Here d LL / d sigma of near_k7_s8_kl448 is at 3.2e-6, a third of the cap: the scalar is the
    difference sum g1 (x - mu) - 3 sum w, and with one responsibility per slot the first sum is closer to the second.)"""
    assert set(J.GPU_CASES) <= set(R.CASES)
    for case in J.GPU_CASES:
        _, errs = J.case_reference(case)
        for stable in (0, 1):
            assert set(errs[stable]) == set(R.case_reference(case)[1][stable]), case
            bad = {k: v for k, v in errs[stable].items() if not v <= R.GATE_CAP / 2}
            assert not bad, (case, stable, bad)
    floor = J.cpu_floor()
    print('[joint] CPU fp32 against fp64, worst over the cases: ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(floor.items(), key=lambda kv: -kv[1])))
    for strict in (0, 1):
        g = J.gates(strict)
        assert set(g) == set(floor) and all(v <= R.GATE_CAP for v in g.values())


# ---- 5. the wrapper ----------------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from iodine_amd import IODINE
    from iodine_amd.model import arch_namespace
    ns = arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))
    for k, v in kw.items():
        setattr(ns, k, v)
    return IODINE(ns)


def test_likelihood_attribute():
    m = _model()
    assert m.likelihood == 'per_channel' and not m._joint()
    m.likelihood = 'joint'
    assert m._joint()
    for bad in ('Joint', 'rgb', None, 1):
        with pytest.raises(ValueError, match="'per_channel' or 'joint'"):
            m.likelihood = bad
    assert m.likelihood == 'joint'
    m.set_option('joint_likelihood', 0)
    assert m.likelihood == 'per_channel' and m._session.options['joint_likelihood'] == 0.0 and not m._session.joint
    m.set_option('joint_likelihood', 1)
    assert m.likelihood == 'joint' and m._session.joint
    assert _model(LIKELIHOOD='joint').likelihood == 'joint'
    with pytest.raises(ValueError):
        _model(LIKELIHOOD='both')
    assert 'likelihood' not in ''.join(m.state_dict().keys())             # the reference's layout


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name + (':' + args[1].decode() + f'={args[2]:g}' if name == 'iodine_set_option' else ''))
            return 0
        return fn


def test_session_sends_the_form_only_when_it_changes(monkeypatch):
    r = _Recorder()
    real_empty = torch.empty
    monkeypatch.setattr(_lib, 'lib', lambda: r)
    monkeypatch.setattr(torch.cuda, 'device', lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch, 'empty', lambda *a, device=None, **kw: real_empty(*a, **kw))
    monkeypatch.setattr(_session.Session, 'stream', lambda self: None)
    cfg = _lib.Config(dim_latent=8, iters=2, slots=3, img_size=16, img_channels=3, sigma=0.1)
    s = _session.Session(cfg, lambda: [])
    dev, obj = torch.device('cuda', 0), (0.1, 1.0, ())
    assert s.joint is False
    s.prepare(dev, 2, 0, 3, 2, 0, obj)
    assert not [c for c in r.calls if 'joint' in c]                       # the default form: nothing is sent
    r.calls.clear()
    s.prepare(dev, 2, 0, 3, 2, 0, obj, joint_likelihood=True)
    assert r.calls == ['iodine_set_option:joint_likelihood=1'] and s.joint
    r.calls.clear()
    s.prepare(dev, 2, 0, 3, 2, 0, obj, joint_likelihood=True)
    assert r.calls == []
    s.prepare(dev, 2, 0, 3, 2, 0, obj)
    assert r.calls == ['iodine_set_option:joint_likelihood=0'] and not s.joint
    r.calls.clear()
    s.prepare(dev, 2, 0, 3, 2, None, None, joint_likelihood=True)          # no objective: the step is skipped, like the other modes
    assert r.calls == [] and not s.joint
    t = _session.Session(cfg, lambda: [], {'joint_likelihood': 1})
    assert t.joint is True
    s.close(); t.close()


def test_engine_flag():
    from iodine_amd.engine import make_parser
    ap = make_parser()
    assert ap.parse_args([]).likelihood is None and ap.parse_args(['--likelihood', 'joint']).likelihood == 'joint'
    with pytest.raises(SystemExit):
        ap.parse_args(['--likelihood', 'rgb'])
    assert 'state_dict' in ap.format_help().split('--likelihood')[-1][:700]


def test_header_states_the_option_flags_and_shapes():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'iodine_hip.h')).read()
    assert '"joint_likelihood"' in h and '(count,1,S,S)' in h and 'bit 3' in h and 'bit 1' in h
