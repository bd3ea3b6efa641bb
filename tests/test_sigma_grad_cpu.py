"""A differentiable ``model.sigma`` and ``model.stable_encoding`` without a device: the float64 reference (sigma_reference.py) against autograd,
a finite difference and the oracle; the stable channel on the pinned 0 / 0 scene; the ABI entry, the two options and the engine flags.

Tiny architecture of the step tests (O.tiny_arch(): K = 3, T = 2, S = 16, L = 8; B = 2)."""
import math
import os
import re

import pytest
import torch

from iodine_amd import IODINE, _args, _lib, engine
from oracle import iodine_oracle as O
from util import hip_arch, rel_err

import sigma_reference as R
import weights_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = O.tiny_arch()
B = 2
F64 = torch.float64


@pytest.fixture(scope='module')
def f64_inputs():
    return R.inputs(ARCH, B, dtype=F64)


# ---- 1. the restatement with a tensor sigma is the oracle ------------------------------------------------------------------------------
def test_tensor_sigma_restates_the_oracle():
    """float32, arch.sigma: the same rounded operations except log(sigma) taken by torch instead of math - the loss agrees to a few ulp"""
    params, x, eps = R.inputs(ARCH, B)
    ref = O.train_forward(x, eps, params, ARCH)
    out = R.train_forward(x, eps, params, ARCH, R.as_sigma(ARCH.sigma, torch.float32))
    assert rel_err(out['loss'].detach(), ref['loss'].detach()) < 1e-6
    assert rel_err(out['post_mean'].detach(), ref['post_mean'].detach()) < 1e-5


# ---- 2. the closed form is the gradient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['plain', 'weights_beta_iw'])
def test_closed_form_equals_autograd_and_a_finite_difference(f64_inputs, case):
    params, x, eps = f64_inputs
    kw = {} if case == 'plain' else dict(beta=0.5, iw=[0.5, 0.0, 2.0], w=W.pattern(B, ARCH.img_size))
    out, _, g_auto, g_closed = R.train_step_grads(x, eps, params, ARCH, 0.1, **kw)
    assert out['ratio'] >= 2.0, out['ratio']                    # the scalar is not a cancellation
    assert abs(float(g_auto - g_closed)) <= 1e-10 * abs(float(g_auto)), (float(g_auto), float(g_closed))
    # A central difference agrees evaluation by evaluation at FIXED posteriors (the refinement inputs are detached, iodine.py:343: the
    # difference quotient of the whole loss would also see sigma move the encoding, which autograd - and the library - must not):
    # evaluation 0 from the initial posterior, evaluation T from lambda_T
    h = 1e-6
    K = ARCH.slots
    init = (params['posterior.init_mean'][None, None].repeat(B, K, 1), params['posterior.init_logvar'][None, None].repeat(B, K, 1))
    for e, (pm, plv) in ((0, init), (ARCH.iters, (out['post_mean'], out['post_logvar']))):
        ll = lambda s: R.s_terms(x, kw.get('w'), pm, plv, eps[e], params, ARCH, R.as_sigma(s))['ll']
        fd = float(ll(0.1 + h) - ll(0.1 - h)) / (2 * h)
        assert abs(fd - float(out['dll'][e])) <= 1e-6 * abs(fd), (e, fd, float(out['dll'][e]))


def test_elbo_closed_form(f64_inputs):
    params, x, eps = f64_inputs
    terms, _, g_auto, g_closed, ratio = R.elbo_grads(x, eps[0], params, ARCH, 0.1, beta=0.5, w=W.pattern(B, ARCH.img_size))
    assert ratio >= 2.0
    assert abs(float(g_auto - g_closed)) <= 1e-10 * abs(float(g_auto))


def test_auxiliary_terms_add_exactly_nothing(f64_inputs):
    """mean, mask, z, lambda_T and the LSTM state do not depend on sigma except through detached inputs: d aux / d sigma is exactly 0"""
    params, x, eps = f64_inputs
    aux = lambda o: ((o['final_mask'] ** 2).sum() + o['final_z'].sum() + o['post_mean'].sum() + o['hidden'][0].sum()
                     + o['terms'][0]['mask'].sum() + o['terms'][1]['mean'].sum())
    _, _, g_plain, _ = R.train_step_grads(x, eps, params, ARCH, 0.1)
    _, _, g_aux, _ = R.train_step_grads(x, eps, params, ARCH, 0.1, aux=aux)
    assert float(g_plain) == float(g_aux)


# ---- 3. the stable channel ---------------------------------------------------------------------------------------------------------
def test_stable_equals_plain_where_plain_is_finite(f64_inputs):
    params, x, eps = f64_inputs
    tp, ts = [], []
    a = R.reconstruct(x, eps, params, ARCH, 0.1, trace=tp)
    b = R.reconstruct(x, eps, params, ARCH, 0.1, stable=True, trace=ts)
    assert torch.isfinite(tp[0]['enc']).all()
    for p, s in zip(tp, ts):
        assert rel_err(s['enc'][:, :, 8], p['enc'][:, :, 8]) < 1e-12
        assert float((s['enc'][:, :, 8].sum(1) - 1).abs().max()) < 1e-12
    for k in ('pred', 'mask', 'post_mean', 'elbos'):
        assert rel_err(b[k], a[k]) < 1e-9, k


def test_stable_is_finite_on_the_pinned_scene():
    """The 0 / 0 is a float32 underflow: exp returns 0 below s_k = sum_c l_kc = -103.98 (half the smallest denormal, 2^-150), and on this
    scene every slot of image 0 is below it.  The float32 restatement hits it and its stable form does not; in float64 nothing
    underflows, there the two forms agree - the stable float64 reference is what the plain one would be without the underflow."""
    arch, params, x, eps = R.pinned_scene(torch.float32)
    tp, ts = [], []
    plain = R.reconstruct(x, eps, params, arch, arch.sigma, trace=tp)
    stable = R.reconstruct(x, eps, params, arch, arch.sigma, stable=True, trace=ts)
    assert torch.isnan(tp[0]['enc'][0, :, 8]).all() and not torch.isfinite(plain['pred'][0]).any()      # the edge is hit
    assert float(torch.exp(torch.tensor(-103.98))) == 0.0 and float(torch.exp(torch.tensor(-103.96))) > 0.0     # where float32 exp gives up
    assert all(torch.isfinite(t['enc']).all() for t in ts)
    assert all(torch.isfinite(stable[k]).all() for k in ('pred', 'mask', 'mean', 'post_mean', 'elbos'))
    assert rel_err(stable['pred'][1], plain['pred'][1]) < 1e-5              # the other image is untouched
    q = {k: v.detach() for k, v in params.items()}
    s32 = R.as_sigma(arch.sigma, torch.float32)
    loss = R.train_forward(x, eps, q, arch, s32, stable=True)['loss']
    assert torch.isfinite(loss) and not torch.isfinite(R.train_forward(x, eps, q, arch, s32)['loss'])
    arch, params, x, eps = R.pinned_scene(F64)
    a = R.reconstruct(x, eps, params, arch, arch.sigma)
    b = R.reconstruct(x, eps, params, arch, arch.sigma, stable=True)
    for k in ('pred', 'mask', 'post_mean', 'elbos'):
        assert torch.isfinite(b[k]).all() and rel_err(b[k], a[k]) < 1e-9, k
    assert rel_err(stable['pred'], b['pred']) < 1e-3 and rel_err(stable['post_mean'], b['post_mean']) < 1e-3


# ---- 4. the interface ---------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_options_and_the_entry():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    api = open(os.path.join(ROOT, 'iodine_amd', 'csrc', 'iodine_api.cpp')).read()
    pad = open(os.path.join(ROOT, 'iodine_amd', 'csrc', 'iodine_pad.cpp')).read()
    for opt in ('sigma_grad', 'stable_encoding'):
        assert f'"{opt}"' in header and f'strcmp(key, "{opt}")' in api, opt
    assert re.search(r'int iodine_last_sigma_grad\(iodine_handle\* h, void\* stream, float\* out, int n\);', header)
    assert 'iodine_last_sigma_grad' in _lib.EXPORTS and 'pad_last_sigma_grad' in pad
    L = _lib.lib()
    assert hasattr(L, 'iodine_last_sigma_grad') and L.iodine_abi_version() == 3
    assert L.iodine_last_sigma_grad(None, None, None, 1) == 1                 # IODINE_ERR_INVALID: no handle


def test_module_reads_a_tensor_sigma_and_the_attribute():
    m = IODINE(hip_arch(ARCH))
    assert m.stable_encoding is False and m._sigma_input() == ()
    assert [n for n, _ in m.named_parameters()] == list(O.param_shapes(ARCH).keys())       # no new module parameter
    log_sigma = torch.tensor(-2.0, requires_grad=True)
    m.sigma = log_sigma.exp()
    assert m._sigma_input() == (m.sigma,) and abs(_args.read_objective(m.sigma, m.beta, m.iter_weights, 2)[0] - 0.1353352832) < 1e-7
    with torch.no_grad():
        assert m._sigma_input() == ()
    m.sigma = m.sigma.detach()
    assert m._sigma_input() == ()                                            # a tensor that does not require grad: today's path
    m.set_option('stable_encoding', 1)
    assert m.stable_encoding is True


def test_parser_takes_the_two_flags():
    ap = engine.make_parser()
    a = ap.parse_args(['--learn-sigma', '--stable-encoding'])
    assert a.learn_sigma and a.stable_encoding
    a = ap.parse_args([])
    assert not a.learn_sigma and not a.stable_encoding
    ls = engine.make_log_sigma(0.1, 'cpu')
    assert ls.requires_grad and ls.dtype == torch.float32 and ls.dim() == 0 and abs(float(ls.detach().exp()) - 0.1) < 1e-7


def test_train_sets_sigma_before_every_step_logs_it_and_saves_log_sigma(tmp_path):
    from iodine_amd.checkpoint import load_checkpoint

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))
            self.sigma, self.seen = 0.1, []

        def forward(self, x):
            self.seen.append(self.sigma)
            return self.w * x.sum() + self.sigma ** 2

    m = Model()
    ls = engine.make_log_sigma(0.1, 'cpu')
    opt = torch.optim.SGD([{'params': list(m.parameters())}, {'params': [ls]}], lr=0.1)
    lines, ck = [], str(tmp_path / 'c.pth')
    engine.train(m, opt, [(torch.ones(1),)] * 3, 'cpu', 3, print_every=1, log=lines.append, checkpoint_path=ck, log_sigma=ls)
    assert len(m.seen) == 3 and all(torch.is_tensor(s) and s.requires_grad for s in m.seen)
    assert m.seen[0].item() > m.seen[1].item() > m.seen[2].item()                 # d loss / d log_sigma = 2 sigma^2 > 0: sigma shrinks
    assert all(', sigma: 0.' in l for l in lines)
    assert isinstance(m.sigma, float) and abs(m.sigma - math.exp(ls.item())) < 1e-7
    extra = load_checkpoint(ck, Model())                                         # the entry rides along; the model entry loads as before
    assert torch.equal(extra['log_sigma'], ls.detach()) and extra['iteration'] == 3
    m.seen = []
    engine.train(m, opt, [(torch.ones(1),)] * 2, 'cpu', 2, log=lambda *a: None)   # without it model.sigma is left alone
    assert m.seen == [m.sigma, m.sigma]


def test_resume_with_and_without_a_saved_log_sigma(tmp_path):
    """engine.resume: an older checkpoint (no log_sigma) under --learn-sigma, a checkpoint written with it under --learn-sigma, and the
    same checkpoint without the flag - refused in words instead of a param-group mismatch"""
    from iodine_amd.checkpoint import save_checkpoint
    net = lambda: torch.nn.Linear(2, 1)

    def run(m, opt, ls=None):
        m.zero_grad()
        loss = m(torch.ones(1, 2)).sum() + (0 if ls is None else ls.exp())
        loss.backward()
        opt.step()

    old, new = str(tmp_path / 'old.pth'), str(tmp_path / 'new.pth')
    m = net()
    opt = torch.optim.Adam([{'params': [p]} for p in m.parameters()], lr=0.1)
    run(m, opt)
    save_checkpoint(old, m, opt, epoch=0, iteration=1)
    # 1. older checkpoint, --learn-sigma: the state loads into the model's groups, log_sigma gets a fresh group behind them
    m1, ls1 = net(), engine.make_log_sigma(0.1, 'cpu')
    o1 = torch.optim.Adam([{'params': [p]} for p in m1.parameters()], lr=0.1)
    extra = engine.resume(old, m1, o1, ls1, 0.1)
    assert extra == {'epoch': 0, 'iteration': 1} and len(o1.param_groups) == 3 and o1.param_groups[2]['params'][0] is ls1
    assert all(torch.equal(a, b) for a, b in zip(m1.state_dict().values(), m.state_dict().values()))
    assert abs(float(ls1.detach().exp()) - 0.1) < 1e-7 and len(o1.state) == 2
    run(m1, o1, ls1)
    save_checkpoint(new, m1, o1, epoch=0, iteration=2, log_sigma=ls1.detach().cpu())
    # 2. written with --learn-sigma, resumed with it: value and optimizer state of the scalar come back
    m2, ls2 = net(), engine.make_log_sigma(0.3, 'cpu')
    o2 = torch.optim.Adam([{'params': [p]} for p in m2.parameters()], lr=0.1)
    extra = engine.resume(new, m2, o2, ls2, 0.1)
    assert torch.equal(ls2.detach(), ls1.detach()) and extra['iteration'] == 2
    assert len(o2.param_groups) == 3 and torch.equal(o2.state[ls2]['exp_avg'], o1.state[ls1]['exp_avg'])
    # 3. ... and without it: a clear refusal, nothing loaded half-way into the optimizer
    m3 = net()
    o3 = torch.optim.Adam([{'params': [p]} for p in m3.parameters()], lr=0.1)
    with pytest.raises(ValueError, match='written with --learn-sigma.*resume it with --learn-sigma'):
        engine.resume(new, m3, o3)
    assert len(o3.param_groups) == 2 and len(o3.state) == 0
    # 4. no log_sigma anywhere: load_checkpoint, as before
    assert engine.resume(old, m3, o3) == {'epoch': 0, 'iteration': 1} and len(o3.state) == 2
