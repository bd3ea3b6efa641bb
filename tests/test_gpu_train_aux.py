"""Auxiliary losses on the training forward's final state: ``loss = model(x, attach_state=True)`` leaves ``model.z / mean / mask /
mask_logits`` and ``model.posterior.mean / logvar`` attached to the graph like the reference (iodine.py:137,171-187,642-651), and one
``backward()`` of any combination of them goes through iodine_train_backward_aux.  Ground truth: the oracle in float64 (tests/aux_reference.py);
gate: rel-L2 < 1e-3 per parameter gradient, the project's gate for oracle-vs-HIP gradients (tests/test_gpu_train.py).

All cases run the tiny architecture (K = 3, T = 2, S = 16, L = 8, B = 2) unless the case is about another shape."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from iodine_amd import _lib, synth
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

import aux_reference as A
from clip_reference import moving_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-3
BASE = O.tiny_arch()
B = 2


def _inputs(arch, seed=50, clip=False, kind='uniform'):
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    x = synth.make_images(B, arch.img_size, seed=seed + 1, kind=kind)
    x = torch.from_numpy(x[0] if kind == 'blobs' else x)
    if clip:
        x = moving_clip(x, arch.iters + 1)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=seed + 2))
    return params, x, eps


def _hip_grads(m, x, eps, W, g_loss=0.0):
    """.grad of every parameter after (g_loss * loss + aux).backward() on a fresh attached forward (None stays None)"""
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV), attach_state=True)
    total = A.hip_aux(m, W) if W else 0.0
    if g_loss:
        total = total + g_loss * loss
    total.backward()
    torch.cuda.synchronize()
    return {n: p.grad for n, p in m.named_parameters()}


def _check(got, ref, names, tag):
    """every refine.* / decoder.* gradient against the float64 oracle.  decoder.conv.bias[3], the mask-logit bias, is compared only where a
    cotangent on the logits themselves makes it well defined: the softmax is invariant to a common offset, so through ``mask`` (and
    through the loss) its gradient is mathematically zero and both sides hold rounding noise there (util.grad_views)."""
    bad = []
    for n, r in ref.items():
        if not n.startswith(('refine.', 'decoder.')):
            continue
        a = got[n].cpu().numpy()
        r = np.zeros_like(a, dtype=np.float64) if r is None else r.numpy()
        if 'mask_logits' not in names:
            a, r = grad_views(n, a, r)
        e = rel_l2(a, r)
        if not e < GATE:
            bad.append((n, e))
    worst = max((rel_l2(got[n].cpu().numpy(), r.numpy()), n) for n, r in ref.items() if r is not None and n != 'decoder.conv.bias')
    print(f'[{tag}] worst rel-L2 {worst[0]:.2e} ({worst[1]})')
    assert not bad, (tag, bad)


def _init_grads_zero(got):
    for n in ('posterior.init_mean', 'posterior.init_logvar'):
        assert got[n] is None or not got[n].any(), n


# ---- 3. aux alone, all six tensors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [1, 0], ids=['split_f16x3', 'exact_fp32'])
def test_aux_alone_matches_oracle(prec):
    params, x, eps = _inputs(BASE)
    W = A.aux_weights(BASE, B, seed=60)
    m = make_hip_model(BASE, params, options={'conv_precision': prec})
    got = _hip_grads(m, x, eps, W)
    _check(got, A.oracle_grads(x, eps, params, BASE, W), W, f'aux alone, conv_precision {prec}')
    _init_grads_zero(got)


# ---- 4. one tensor at a time ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def base_case():
    params, x, eps = _inputs(BASE)
    return params, x, eps, A.aux_weights(BASE, B, seed=60), make_hip_model(BASE, params)


@pytest.mark.parametrize('names', [(n,) for n in A.TENSORS] + [('mask', 'mask_logits')], ids=lambda t: '+'.join(t))
def test_single_cotangents_match_oracle(base_case, names):
    params, x, eps, W, m = base_case
    Wn = {n: W[n] for n in names}
    got = _hip_grads(m, x, eps, Wn)
    _check(got, A.oracle_grads(x, eps, params, BASE, Wn), Wn, 'only ' + '+'.join(names))
    _init_grads_zero(got)


# ---- 5. loss + aux --------------------------------------------------------------------------------------------------------------
def test_loss_plus_aux_matches_oracle_and_is_additive(base_case):
    params, x, eps, W, m = base_case
    both = _hip_grads(m, x, eps, W, 1.0)
    ref = A.oracle_grads(x, eps, params, BASE, W, 1.0)
    _check(both, ref, W, 'loss + aux')
    for n in ('posterior.init_mean', 'posterior.init_logvar'):               # (through the loss they are not zero)
        assert rel_l2(both[n].cpu().numpy(), ref[n].numpy()) < GATE, n
    both = {n: g.clone() for n, g in both.items()}
    g_loss = {n: g.clone() for n, g in _hip_grads(m, x, eps, {}, 1.0).items()}
    g_aux = {n: g.clone() for n, g in _hip_grads(m, x, eps, W).items()}
    half = _hip_grads(m, x, eps, W, 0.5)                                     # grad_loss must not scale the auxiliary part
    for n in both:
        e1 = rel_l2(both[n].cpu().numpy(), (g_loss[n] + g_aux[n]).cpu().numpy())
        e2 = rel_l2(half[n].cpu().numpy(), (0.5 * g_loss[n] + g_aux[n]).cpu().numpy())
        assert e1 < 1e-5 and e2 < 1e-5, (n, e1, e2)


# ---- 6. unchanged behaviour, bitwise -----------------------------------------------------------------------------------------------
def test_attach_state_changes_no_bit(base_case):
    params, x, eps, _, _ = base_case
    runs = []
    for attach in (False, True):
        m = make_hip_model(BASE, params)
        loss = m(x.to(DEV), eps.to(DEV), attach_state=attach) if attach else m(x.to(DEV), eps.to(DEV))
        ts = A.hip_tensors(m)
        if attach:
            assert all(t.requires_grad and t.grad_fn is not None for t in ts.values())
        else:
            assert not any(t.requires_grad for t in ts.values())
            ts['mask'].cpu().numpy()                                         # what existing callers do with them
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), m.elbo_terms.clone(), {k: t.detach().clone() for k, t in ts.items()},
                     {n: p.grad.clone() for n, p in m.named_parameters()}))
    (l0, e0, t0, g0), (l1, e1, t1, g1) = runs
    assert torch.equal(l0, l1) and torch.equal(e0, e1)
    assert all(torch.equal(t0[k], t1[k]) for k in t0)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    m = make_hip_model(BASE, params)
    with torch.no_grad():                                                    # a no-op without grad mode
        m(x.to(DEV), eps.to(DEV), attach_state=True)
    assert not any(t.requires_grad for t in A.hip_tensors(m).values())
    assert all(torch.equal(t, t0[k]) for k, t in A.hip_tensors(m).items())


# ---- 7. edges -------------------------------------------------------------------------------------------------------------------
EDGES = {
    # name: (arch, library options, clip?)
    'T1': (dataclasses.replace(BASE, iters=1), {}, False),
    # one slot has to explain a whole image: on uniform-noise images some pixel's summed log-likelihood underflows in float32 and the
    # reference's un-stabilised mask posterior is 0 / 0 there (iodine.py:286-293, tests/test_gpu_boundary.py) - float32 arithmetic, which
    # the library reproduces and a float64 ground truth cannot.  So this case runs the 'blobs' scene, like 'one_slot' of
    # tests/test_gpu_edge_cases.py; the finite-forward assertion below keeps the inputs honest
    'K1': (dataclasses.replace(BASE, slots=1), {}, False),
    'padded_L6_H30': (dataclasses.replace(BASE, dim_latent=6, ref_mlp=30), {}, False),
    'k5_gen0': (dataclasses.replace(BASE, dec_kernel=5), {'gen_conv_precision': 0}, False),
    'k5_gen1': (dataclasses.replace(BASE, dec_kernel=5), {'gen_conv_precision': 1}, False),
    'head_unfused': (BASE, {'head_fused': 0}, False),
    'head_fused': (BASE, {'head_fused': 1}, False),
    'tile_f16': (BASE, {'conv_variant': 1}, False),
    'clip': (BASE, {}, True),
}


@pytest.mark.parametrize('name', list(EDGES))
def test_edges_match_oracle(name):
    arch, options, clip = EDGES[name]
    params, x, eps = _inputs(arch, seed=70, clip=clip, kind='blobs' if name == 'K1' else 'uniform')
    W = A.aux_weights(arch, B, seed=71)
    m = make_hip_model(arch, params, options=options)
    got = _hip_grads(m, x, eps, W)
    assert bool(torch.isfinite(m.elbo_terms).all()), 'the forward itself is not finite on these inputs'
    _check(got, A.oracle_grads(x, eps, params, arch, W), W, name)
    _init_grads_zero(got)
    if name == 'K1':                                                         # one slot: mask = 1 whatever the logits are
        only = _hip_grads(m, x, eps, {'mask': W['mask']})
        assert all(g is None or not g.any() for g in only.values())
    # d(out) / d(loss) first, then the auxiliary decoder gradients with factor 1: the order on every decoder path, and the unfused
    # launch sequence's own device-side scaling of the ELBO seeds
    if name in ('head_unfused', 'tile_f16', 'k5_gen0', 'k5_gen1', 'padded_L6_H30'):
        got = _hip_grads(m, x, eps, W, 0.5)
        _check(got, A.oracle_grads(x, eps, params, arch, W, 0.5), W, name + ', 0.5 loss + aux')


def test_graph_replay_over_three_steps():
    params, _, _ = _inputs(BASE)
    m = make_hip_model(BASE, params, options={'graph': 1})
    for step in range(3):                                                    # eager, captured, replayed - fresh inputs every step
        _, x, eps = _inputs(BASE, seed=80 + 3 * step)
        W = A.aux_weights(BASE, B, seed=90 + step)
        got = _hip_grads(m, x, eps, W, 1.0)
        _check(got, A.oracle_grads(x, eps, params, BASE, W, 1.0), W, f'graph step {step}')
    assert m.profile_read('graph_replays')[1] > 0


# ---- 8. the rendering backward with a logits cotangent, at op level ----------------------------------------------------------------
def _render_case(K, P, seed=5):
    Bn = 2
    o = torch.from_numpy(synth.normal((Bn, K, 4, P), seed=seed)).double() * 2.0          # (exact in float32: what the kernel reads)
    gs = [torch.from_numpy(synth.normal(s, seed=seed + 1 + i)) for i, s in enumerate(((Bn, 3, P), (Bn, K, 1, P), (Bn, K, 3, P), (Bn, K, 1, P)))]
    od = o.clone().requires_grad_(True)
    mean, logits = torch.sigmoid(od[:, :, :3]), od[:, :, 3:]
    mask = torch.softmax(logits, dim=1)
    pred = (mask * mean).sum(1)
    loss = sum((g.double() * t).sum() for g, t in zip(gs, (pred, mask, mean, logits)))
    return o, gs, torch.autograd.grad(loss, od)[0]


@pytest.mark.parametrize('strict', [0, 1], ids=['default', 'strict'])
@pytest.mark.parametrize('P', [256, 24 * 24])                              # 576: not a multiple of the block's 256 pixels
@pytest.mark.parametrize('K', [1, 3, 16])
def test_render_bwd_logits_kernel_matches_fp64_autograd(K, P, strict):
    o, gs, ref = _render_case(K, P)
    Bn = o.shape[0]
    dec = o.float().permute(0, 1, 3, 2).contiguous().to(DEV)                  # [N][P][4]
    gd = [g.contiguous().to(DEV) for g in gs]
    L = _lib.lib()
    out = torch.full((Bn * K, P, 4), float('nan'), device=DEV)
    _lib.check(L.iodine_op_render_bwd_logits(None, _lib.ptr(dec), *[_lib.ptr(g) for g in gd], _lib.ptr(out), Bn, K, P, strict), None,
               'iodine_op_render_bwd_logits')
    got = out.cpu().view(Bn, K, P, 4).permute(0, 1, 3, 2)
    e = rel_err(got, ref)
    print(f'[render_bwd_logits K={K} P={P} strict={strict}] {e:.2e}')
    assert e < 3e-6, e                                                       # the bound of test_render_bwd_kernel_matches_fp64_autograd
    if K == 1:                                                               # one slot: only the logits' own cotangent is left, exactly
        assert torch.equal(got[:, :, 3:], gs[3])
    # without the logits cotangent: the existing kernel, bit for bit
    a, b = torch.full_like(out, float('nan')), torch.full_like(out, float('nan'))
    _lib.check(L.iodine_op_render_bwd_logits(None, _lib.ptr(dec), *[_lib.ptr(g) for g in gd[:3]], None, _lib.ptr(a), Bn, K, P, strict), None)
    _lib.check(L.iodine_op_render_bwd(None, _lib.ptr(dec), *[_lib.ptr(g) for g in gd[:3]], _lib.ptr(b), Bn, K, P, strict), None)
    assert torch.equal(a, b)


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------
def test_second_backward_is_a_stale_forward(base_case):
    params, x, eps, W, m = base_case
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV), attach_state=True)
    aux = A.hip_aux(m, W)
    aux.backward()
    with pytest.raises(RuntimeError, match='stale forward'):
        loss.backward()


def test_attach_state_above_max_batch_is_refused(base_case):
    params, x, eps, _, _ = base_case
    m = make_hip_model(BASE, params, options={'batch_cap': 1})
    with pytest.raises(RuntimeError, match=r'max_batch\(training=True\) = 1'):
        m(x.to(DEV), eps.to(DEV), attach_state=True)
    with torch.no_grad():                                                    # without grad mode nothing is attached: the chunked path runs
        m(x.to(DEV), eps.to(DEV), attach_state=True)
    with pytest.raises(RuntimeError, match='state'):
        m(x.to(DEV), eps.to(DEV), state=(None,) * 4, attach_state=True)


def test_cabi_without_cotangents_is_the_plain_backward_bitwise(base_case):
    params, x, eps, _, _ = base_case
    m = make_hip_model(BASE, params)
    L = _lib.lib()
    n = sum(p.numel() for p in m.parameters())
    gl = torch.full((), 0.75, device=DEV)
    flats = []
    for entry in ('flat', 'aux'):
        with torch.no_grad():
            m(x.to(DEV), eps.to(DEV))
        flat = torch.full((n,), float('nan'), device=DEV)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if entry == 'flat':
            rc = L.iodine_train_backward_flat(m._handle, st, _lib.ptr(gl), _lib.ptr(flat), 0)
        else:
            rc = L.iodine_train_backward_aux(m._handle, st, _lib.ptr(gl), None, None, None, None, None, None, _lib.ptr(flat), 0)
        _lib.check(rc, m._handle, entry)
        torch.cuda.synchronize()
        flats.append(flat)
    assert torch.equal(flats[0], flats[1]) and bool(flats[0].any())
    # consumed like the plain backward: a second call is refused with IODINE_ERR_STATE (3), with or without cotangents
    z = torch.zeros((B, BASE.slots, BASE.dim_latent), device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = flats[1].clone()
    assert L.iodine_train_backward_aux(m._handle, st, _lib.ptr(gl), None, None, None, None, None, None, _lib.ptr(flats[1]), 0) == 3
    assert L.iodine_train_backward_aux(m._handle, st, None, None, None, None, _lib.ptr(z), None, None, _lib.ptr(flats[1]), 0) == 3
    torch.cuda.synchronize()
    assert torch.equal(flats[1], before)


# ---- 10. one flat buffer ----------------------------------------------------------------------------------------------------------
def test_gradients_form_one_flat_buffer_with_aux(base_case):
    from iodine_amd import parallel
    params, x, eps, W, m = base_case
    grads = list(_hip_grads(m, x, eps, W, 1.0).values())
    flat = parallel._shared_flat_view(grads)
    assert flat is not None and flat.numel() == sum(p.numel() for p in m.parameters())
    before = [g.clone() for g in grads]
    flat.mul_(2.0)
    assert all(torch.equal(g, 2.0 * b) for g, b in zip(grads, before))
