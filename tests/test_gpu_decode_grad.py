"""Autograd through ONE decode(z) / elbo(x) (iodine_decode_backward / iodine_elbo_backward, kernels_render.hip) against the CPU oracle
run in fp64 with torch.autograd.grad: the rendering-backward kernel on its own, decode and elbo end to end on every decoder path, and the
call-order contract.  Gates: kernel level 3e-6 of the output-tensor maximum (as tests/test_gpu_ops.py), gradients rel-L2 <= 1e-3 per
tensor.  Every case prints its worst tensor."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iodine_amd import _lib, synth
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-3


# ---- 1. kernel level -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _render_case(K, P):
    """inputs (fp32) and the fp64 autograd reference of every combination of upstream gradients, computed once per shape"""
    B = 2
    gen = torch.Generator().manual_seed(100 * K + P)
    o = torch.randn(B, K, 4, P, generator=gen) * 2
    o[:, :, 3] = (torch.rand(B, K, P, generator=gen) - 0.5) * 60         # logits spread to +-30: some masks saturate
    gs = (torch.randn(B, 3, P, generator=gen), torch.randn(B, K, 1, P, generator=gen), torch.randn(B, K, 3, P, generator=gen))
    refs = {}
    for use in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        od = o.double().requires_grad_(True)
        mean, mask = torch.sigmoid(od[:, :, :3]), F.softmax(od[:, :, 3:], dim=1)
        pred = (mask * mean).sum(1)
        loss = sum((g.double() * t).sum() for g, t, u in zip(gs, (pred, mask, mean), use) if u)
        refs[use] = torch.autograd.grad(loss, od)[0]
    return o, gs, refs


@pytest.mark.parametrize('strict', [0, 1], ids=['default', 'strict'])
@pytest.mark.parametrize('P', [16 * 16, 24 * 24])
@pytest.mark.parametrize('K', [1, 2, 7, 16])
def test_render_bwd_kernel_matches_fp64_autograd(K, P, strict):
    o, gs, refs = _render_case(K, P)
    B = o.shape[0]
    dec = o.permute(0, 1, 3, 2).contiguous().to(DEV)                      # [N][P][4]
    gd = [g.contiguous().to(DEV) for g in gs]
    for use, ref in refs.items():
        out = torch.full((B * K, P, 4), float('nan'), device=DEV)
        ptrs = [_lib.ptr(g) if u else None for g, u in zip(gd, use)]
        _lib.check(_lib.lib().iodine_op_render_bwd(None, _lib.ptr(dec), ptrs[0], ptrs[1], ptrs[2], _lib.ptr(out), B, K, P, strict), None,
                   'iodine_op_render_bwd')
        got = out.cpu().view(B, K, P, 4).permute(0, 1, 3, 2)
        e = rel_err(got, ref)
        print(f'[render_bwd K={K} P={P} strict={strict} use={use}] {e:.2e}')
        assert e < 3e-6, (use, e)
        if K == 1:
            assert torch.equal(got[:, :, 3], torch.zeros_like(got[:, :, 3])) and not torch.signbit(got[:, :, 3]).any()


# ---- shared set-up ------------------------------------------------------------------------------------------------------------
def _params(arch, seed=11):
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    return {k: torch.from_numpy(v) for k, v in pn.items()}


BASE = O.tiny_arch()                                                       # S = 16, 32 channels, L = 8, K = 3
CASES = {
    # name: (arch, library options, slots of z, cotangents used (pred, mask, mean))
    'prec1': (BASE, {'conv_precision': 1}, 3, (1, 1, 1)),
    'prec0': (BASE, {'conv_precision': 0}, 3, (1, 1, 1)),
    'tile_f16': (BASE, {'conv_variant': 1}, 3, (1, 1, 1)),
    'tile_f32': (BASE, {'conv_variant': 1, 'conv_precision': 0}, 3, (1, 1, 1)),
    'unfused': (BASE, {'fuse_l0': 0, 'out_bwd_fused': 0}, 3, (1, 1, 1)),
    'S24_generic': (dataclasses.replace(BASE, img_size=24), {}, 3, (1, 1, 1)),
    'k5_gen0': (dataclasses.replace(BASE, dec_kernel=5), {'gen_conv_precision': 0}, 3, (1, 1, 1)),
    'k5_gen1': (dataclasses.replace(BASE, dec_kernel=5), {'gen_conv_precision': 1}, 3, (1, 1, 1)),
    'latent6_padded': (dataclasses.replace(BASE, dim_latent=6), {}, 3, (1, 1, 1)),
    'K1_from_z': (BASE, {}, 1, (1, 1, 1)),
    'K5_from_z': (BASE, {}, 5, (1, 1, 1)),
    'wgrad_accum': (BASE, {'wgrad_accum': 1}, 3, (1, 1, 1)),
    'mask_only': (BASE, {}, 3, (0, 1, 0)),
}


def _decode_inputs(arch, K, B=2, seed=3):
    S, L = arch.img_size, arch.dim_latent
    z = torch.from_numpy(synth.normal((B, K, L), seed=seed))
    cots = (torch.from_numpy(synth.normal((B, 3, S, S), seed=seed + 1)), torch.from_numpy(synth.normal((B, K, 1, S, S), seed=seed + 2)),
            torch.from_numpy(synth.normal((B, K, 3, S, S), seed=seed + 3)))
    return z, cots


def _oracle_render(z, q, arch):
    mean, logits = O.decoder(z, q, arch)
    mask = F.softmax(logits, dim=1)
    return (mask * mean).sum(1), mask, mean


def _oracle_decode_grads(arch, params, z, cots, use):
    q = {k: v.double().requires_grad_(True) for k, v in params.items()}
    zz = z.double().requires_grad_(True)
    outs = _oracle_render(zz, q, arch)
    loss = sum((c.double() * t).sum() for c, t, u in zip(cots, outs, use) if u)
    names = [n for n in q if n.startswith('decoder.')]
    gr = torch.autograd.grad(loss, [zz] + [q[n] for n in names])
    return gr[0], dict(zip(names, gr[1:]))


def _hip_decode_loss(m, z, cots, use):
    outs = m.decode(z)
    return sum((c.to(DEV) * t).sum() for c, t, u in zip(cots, outs, use) if u), outs


def _worst(pairs):
    """[(name, got, ref)] -> (worst rel-L2, its name) with the per-tensor views of util.grad_views"""
    return max((rel_l2(*grad_views(n, g.detach().cpu().numpy(), r.detach().cpu().numpy())), n) for n, g, r in pairs)


# ---- 2. decode end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_decode_gradients_match_fp64_oracle(name):
    arch, opts, K, use = CASES[name]
    params = _params(arch)
    z, cots = _decode_inputs(arch, K)
    ref_dz, ref = _oracle_decode_grads(arch, params, z, cots, use)
    m = make_hip_model(arch, params, options=opts)
    zd = z.to(DEV).requires_grad_(True)
    loss, outs = _hip_decode_loss(m, zd, cots, use)
    assert all(o.grad_fn is not None for o in outs)
    loss.backward()
    torch.cuda.synchronize()
    assert m.K == arch.slots                                              # K came from z; the module's slot count is left alone
    got = dict(m.named_parameters())
    worst = _worst([('z', zd.grad, ref_dz)] + [(n, got[n].grad, r) for n, r in ref.items()])
    print(f'[decode {name}] worst tensor {worst[1]} {worst[0]:.2e}')
    assert worst[0] <= GATE, worst
    for n, p in got.items():                                              # nothing outside the decoder is touched by a decode
        if not n.startswith('decoder.'):
            assert p.grad is None or not p.grad.any(), n


# ---- 3. elbo end to end ----------------------------------------------------------------------------------------------------
ELBO_CASES = ['prec1', 'prec0', 'tile_f16', 'tile_f32', 'unfused', 'S24_generic', 'k5_gen0', 'k5_gen1', 'latent6_padded', 'wgrad_accum']


def _elbo_inputs(arch, B=2, seed=7):
    K, L = arch.slots, arch.dim_latent
    x = torch.from_numpy(synth.make_images(B, arch.img_size, seed=seed))
    eps = torch.from_numpy(synth.normal((B, K, L), seed=seed + 1))
    pm = 0.5 * torch.from_numpy(synth.normal((B, K, L), seed=seed + 2))
    plv = 0.3 * torch.from_numpy(synth.normal((B, K, L), seed=seed + 3))
    return x, eps, pm, plv


def _oracle_elbo_grads(arch, params, x, eps, pm, plv):
    """d ELBO / d (posterior tensors, parameters); pm None = the initial posterior (init_mean / init_logvar repeated, iodine.py:607-618)"""
    q = {k: v.double().requires_grad_(True) for k, v in params.items()}
    B, K = x.shape[0], arch.slots
    if pm is None:
        pmm, plvv = q['posterior.init_mean'][None, None].repeat(B, K, 1), q['posterior.init_logvar'][None, None].repeat(B, K, 1)
        names = [n for n in q if n.startswith(('decoder.', 'posterior.'))]
    else:
        pmm, plvv = pm.double().requires_grad_(True), plv.double().requires_grad_(True)
        names = [n for n in q if n.startswith('decoder.')]
    elbo = O.elbo_terms(x.double(), pmm, plvv, eps.double(), q, arch)['elbo']
    wrt = [q[n] for n in names] + ([] if pm is None else [pmm, plvv])
    gr = torch.autograd.grad(elbo, wrt)
    return elbo.detach(), dict(zip(names, gr)), (None if pm is None else gr[len(names):])


@pytest.mark.parametrize('name', ELBO_CASES)
def test_elbo_gradients_match_fp64_oracle(name):
    arch, opts, _, _ = CASES[name]
    params = _params(arch)
    x, eps, pm, plv = _elbo_inputs(arch)
    ref_elbo, ref, ref_post = _oracle_elbo_grads(arch, params, x, eps, pm, plv)
    m = make_hip_model(arch, params, options=opts)
    with torch.no_grad():
        m.posterior.mean, m.posterior.logvar = pm.to(DEV), plv.to(DEV)
        plain = m.elbo(x.to(DEV), eps.to(DEV)).clone()
        bytes0 = m._workspace.numel()
    m.posterior.mean, m.posterior.logvar = pm.to(DEV).requires_grad_(True), plv.to(DEV).requires_grad_(True)
    elbo = m.elbo(x.to(DEV), eps.to(DEV))
    assert elbo.grad_fn is not None and torch.equal(elbo.detach(), plain)          # the same bits as the non-differentiable call
    assert abs(elbo.item() - ref_elbo.item()) <= 1e-4 * abs(ref_elbo.item())
    L = _lib.lib()
    assert bytes0 == L.iodine_workspace_bytes(m._handle, 2, 0) <= L.iodine_workspace_bytes(m._handle, 2, 2) <= L.iodine_workspace_bytes(m._handle, 2, 1)
    elbo.backward()
    torch.cuda.synchronize()
    got = dict(m.named_parameters())
    worst = _worst([('posterior.mean', m.posterior.mean.grad, ref_post[0]), ('posterior.logvar', m.posterior.logvar.grad, ref_post[1])] +
                   [(n, got[n].grad, r) for n, r in ref.items()])
    print(f'[elbo {name}] worst tensor {worst[1]} {worst[0]:.2e}')
    assert worst[0] <= GATE, worst
    for n, p in got.items():
        if not n.startswith('decoder.'):
            assert p.grad is None or not p.grad.any(), n


@pytest.mark.parametrize('name', ['prec1', 'latent6_padded', 'S24_generic'])
def test_elbo_from_the_initial_posterior_and_a_non_unit_upstream(name):
    """posterior.init_mean / init_logvar receive the (B, K) sums; (3 * elbo).backward() checks the device-side scale"""
    arch, opts, _, _ = CASES[name]
    params = _params(arch)
    x, eps, _, _ = _elbo_inputs(arch)
    _, ref, _ = _oracle_elbo_grads(arch, params, x, eps, None, None)
    m = make_hip_model(arch, params, options=opts)
    assert m.posterior.mean is None
    elbo = m.elbo(x.to(DEV), eps.to(DEV), differentiable=True)
    (3 * elbo).backward()
    torch.cuda.synchronize()
    got = dict(m.named_parameters())
    worst = _worst([(n, got[n].grad, 3 * r) for n, r in ref.items()])
    print(f'[elbo init-posterior {name}] worst tensor {worst[1]} {worst[0]:.2e}')
    assert worst[0] <= GATE, worst
    assert got['posterior.init_mean'].grad is not None and got['refine.mlp.layers.0.weight'].grad is None


# ---- 4. contract -----------------------------------------------------------------------------------------------------------
def _model(opts=None, arch=BASE):
    params = _params(arch)
    return make_hip_model(arch, params, options=opts), params


def test_plain_decode_is_unchanged_and_bitwise_equal_to_the_differentiable_one():
    m, _ = _model()
    z, _ = _decode_inputs(BASE, 3)
    plain = m.decode(z.to(DEV))
    L = _lib.lib()
    assert all(o.grad_fn is None and not o.requires_grad for o in plain)
    assert m._ws_key[1] == 0 and m._workspace.numel() == L.iodine_workspace_bytes(m._handle, 2, 0)     # the inference workspace, as before
    with torch.no_grad():
        assert all(o.grad_fn is None for o in m.decode(z.to(DEV).requires_grad_(True)))
    assert all(o.grad_fn is None for o in m.decode(z.to(DEV).requires_grad_(True), differentiable=False))
    diff = m.decode(z.to(DEV).requires_grad_(True))
    forced = m.decode(z.to(DEV), differentiable=True)                     # decoder-only: graph into the parameters
    assert all(o.grad_fn is not None for o in diff) and all(o.grad_fn is not None for o in forced)
    assert all(torch.equal(a.detach(), b) for a, b in zip(diff, plain)) and all(torch.equal(a.detach(), b) for a, b in zip(forced, plain))
    b0, b2, b1 = (L.iodine_workspace_bytes(m._handle, 2, mode) for mode in (0, 2, 1))
    assert 0 < b0 <= b2 <= b1


def test_stale_and_repeated_backward_raise():
    m, _ = _model()
    z, cots = _decode_inputs(BASE, 3)
    x = torch.from_numpy(synth.make_images(2, BASE.img_size, seed=1)).to(DEV)
    loss, _ = _hip_decode_loss(m, z.to(DEV).requires_grad_(True), cots, (1, 1, 1))
    m.reconstruct(x)                                                      # re-uses the workspace
    with pytest.raises(RuntimeError, match='stale decode'):
        loss.backward()
    loss, _ = _hip_decode_loss(m, z.to(DEV).requires_grad_(True), cots, (1, 1, 1))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='stale decode'):
        loss.backward()
    m.posterior.mean, m.posterior.logvar = (torch.zeros(2, 3, BASE.dim_latent, device=DEV).requires_grad_(True) for _ in range(2))
    e = m.elbo(x)
    m.decode(z.to(DEV))
    with pytest.raises(RuntimeError, match='stale elbo'):
        e.backward()
    # the library's own check (the C ABI without the wrapper's serial): nothing saved -> IODINE_ERR_STATE
    rc = _lib.lib().iodine_decode_backward(m._handle, None, 2, None, None, None, None, None, 0)
    assert rc == 3 and b'save_for_backward' in _lib.lib().iodine_last_error(m._handle)
    rc = _lib.lib().iodine_elbo_backward(m._handle, None, None, None, None, None, 0)
    assert rc == 3


def test_chunked_decode_and_elbo_match_the_unchunked_call():
    m, params = _model()
    B = 5
    z, cots = _decode_inputs(BASE, 3, B=B)
    zd = z.to(DEV).requires_grad_(True)
    loss, outs = _hip_decode_loss(m, zd, cots, (1, 1, 1))
    loss.backward()
    ref = [zd.grad.clone()] + [p.grad.clone() for n, p in m.named_parameters() if n.startswith('decoder.')]
    m.zero_grad(set_to_none=True)
    m.set_option('batch_cap', 2)
    zc = z.to(DEV).requires_grad_(True)
    loss_c, outs_c = _hip_decode_loss(m, zc, cots, (1, 1, 1))
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(outs_c, outs))          # bitwise per image
    loss_c.backward()
    got = [zc.grad] + [p.grad for n, p in m.named_parameters() if n.startswith('decoder.')]
    worst = _worst([(str(i), a, b) for i, (a, b) in enumerate(zip(got, ref))])
    assert worst[0] <= GATE, worst                                        # equal to summation order
    # elbo: batch mean over chunks
    x, eps, pm, plv = _elbo_inputs(BASE, B=B)
    res = []
    for cap in (0, 2):
        m.set_option('batch_cap', cap)
        m.zero_grad(set_to_none=True)
        m.posterior.mean, m.posterior.logvar = pm.to(DEV).requires_grad_(True), plv.to(DEV).requires_grad_(True)
        e = m.elbo(x.to(DEV), eps.to(DEV))
        (2 * e).backward()
        res.append((e.detach(), [m.posterior.mean.grad, m.posterior.logvar.grad] + [p.grad for n, p in m.named_parameters() if n.startswith('decoder.')]))
    assert abs(res[0][0].item() - res[1][0].item()) <= 1e-6 * abs(res[0][0].item())
    worst = _worst([(str(i), a, b) for i, (a, b) in enumerate(zip(res[1][1], res[0][1]))])
    assert worst[0] <= GATE, worst


def test_graph_mode_replays_differentiable_decode_steps():
    z, cots = _decode_inputs(BASE, 3)
    m0, _ = _model()
    z0 = z.to(DEV).requires_grad_(True)
    _hip_decode_loss(m0, z0, cots, (1, 1, 1))[0].backward()
    g0 = [z0.grad] + [p.grad for n, p in m0.named_parameters() if n.startswith('decoder.')]
    m, _ = _model()
    m.set_option('graph', 1)
    keep, caps = [], []
    with torch.cuda.stream(torch.cuda.Stream()):
        for step in range(3):
            zs = z.clone().to(DEV).requires_grad_(True)                   # fresh caller tensors every step
            junk = torch.empty(1000 + 37 * step, device=DEV)
            m.zero_grad(set_to_none=True)
            _hip_decode_loss(m, zs, [c.clone() for c in cots], (1, 1, 1))[0].backward()
            keep.append(([zs.grad] + [p.grad for n, p in m.named_parameters() if n.startswith('decoder.')], junk))
            caps.append(m.profile_read('graph_captures', reset=False)[1])
        torch.cuda.synchronize()
    for grads, _ in keep:
        assert all(torch.equal(a, b) for a, b in zip(grads, g0))
    assert caps[1] == caps[2] == 2                                        # decode + its backward: captured on the second step, replayed after


def test_backward_accumulates_into_grad():
    m, _ = _model()
    z, cots = _decode_inputs(BASE, 3)
    zd = z.to(DEV).requires_grad_(True)
    _hip_decode_loss(m, zd, cots, (1, 1, 1))[0].backward()
    g1 = [zd.grad.clone()] + [p.grad.clone() for n, p in m.named_parameters() if n.startswith('decoder.')]
    (0.5 * _hip_decode_loss(m, zd, cots, (1, 1, 1))[0]).backward()         # no zero_grad: .grad accumulates
    g2 = [zd.grad] + [p.grad for n, p in m.named_parameters() if n.startswith('decoder.')]
    for a, b in zip(g2, g1):
        assert rel_l2(a.cpu().numpy(), 1.5 * b.cpu().numpy()) < 1e-6


def test_three_step_test_time_optimisation_of_z_tracks_the_oracle():
    """SGD on z against MSE(pred, target): the paper's plain gradient ascent baseline in miniature.  Losses within rel 2e-5 of the fp64
    oracle trajectory (the gate style of test_training_trajectory_matches_reference) and monotonically decreasing."""
    arch, lr, steps = BASE, 4.0, 3
    params = _params(arch)
    z0, _ = _decode_inputs(arch, 3)
    target = torch.from_numpy(synth.make_images(2, arch.img_size, seed=9))
    q = {k: v.double() for k, v in params.items()}
    zr, ref = z0.double(), []
    for _ in range(steps + 1):
        zr = zr.detach().requires_grad_(True)
        loss = ((_oracle_render(zr, q, arch)[0] - target.double()) ** 2).mean()
        ref.append(loss.item())
        zr = zr - lr * torch.autograd.grad(loss, zr)[0]
    assert all(b < a for a, b in zip(ref, ref[1:])), ref                   # (the set-up itself: this step size descends)
    m = make_hip_model(arch, params)
    zd, td, got = z0.to(DEV), target.to(DEV), []
    for _ in range(steps + 1):
        zd = zd.detach().requires_grad_(True)
        loss = ((m.decode(zd)[0] - td) ** 2).mean()
        got.append(loss.item())
        loss.backward()
        zd = zd - lr * zd.grad
    print(f'[z optimisation] hip {got} oracle {ref}')
    assert all(b < a for a, b in zip(got, got[1:])), got
    assert np.abs(np.array(got) - np.array(ref)).max() <= 2e-5 * np.abs(ref).max(), (got, ref)
