"""Per-frame auxiliary losses: ``model(x, attach_frames=...)`` leaves chosen ELBO evaluations of the training forward attached to the graph
(``model.frames``), and one ``backward()`` of the loss plus terms on any of them goes through iodine_train_backward_frames.

Ground truth: the float64 composition of tests/frames_reference.py.  Gate: rel-L2 < 1e-3 per ``refine.* / decoder.*`` gradient tensor, the
project's gate for auxiliary gradients (tests/test_gpu_train_aux.py), with its handling of the mask-logit bias (util.grad_views) where no
cotangent on the logits is present; test_train_frames_cpu pins float32 arithmetic on these inputs at ~2e-6.

BASE: the tiny architecture (16 px, K = 3, T = 2, B = 2); WS: 32 px, 64 channels, T = 3 - weight-stationary convs, the fused first
refinement layer, the fused head."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from iodine_amd import _lib, synth
from iodine_amd.engine import clip_backward
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

import frames_reference as F
import train_state_reference as S
from clip_reference import moving_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-3
BASE = O.tiny_arch()
WS = O.tiny_arch(slots=3, iters=3, img_size=32, chan=64)
B = 2
KEYS = F.TENSORS


def _inputs(arch, seed=50, clip=False, kind='uniform'):
    """built like tests/test_gpu_train_aux.py::_inputs"""
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    x = synth.make_images(B, arch.img_size, seed=seed + 1, kind=kind)
    x = torch.from_numpy(x[0] if kind == 'blobs' else x)
    if clip:
        x = moving_clip(x, arch.iters + 1)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=seed + 2))
    return params, x, eps


def _hip_grads(m, x, eps, W, g_loss=0.0, frames=None, **kw):
    """.grad of every parameter after (g_loss * loss + aux).backward() on a fresh forward with the evaluations of W attached"""
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV), attach_frames=sorted({i for i, _ in W}) if frames is None else frames, **kw)
    total = F.hip_aux(m, W) if W else 0.0
    if g_loss:
        total = total + g_loss * loss
    total.backward()
    torch.cuda.synchronize()
    return {n: p.grad for n, p in m.named_parameters()}


def _check(got, ref, W, tag, init=False):
    """every refine.* / decoder.* gradient (init: posterior.init_* too) against the float64 reference"""
    logits = any(n == 'mask_logits' for _, n in W)
    bad, worst = [], (0.0, '')
    for n, r in ref.items():
        if not n.startswith(('refine.', 'decoder.') + (('posterior.',) if init else ())):
            continue
        a = np.zeros(tuple(r.shape if r is not None else ()), dtype=np.float64) if got[n] is None else got[n].cpu().numpy()
        r = np.zeros_like(a, dtype=np.float64) if r is None else r.numpy()
        if not logits:
            a, r = grad_views(n, a, r)
        e = rel_l2(a, r)
        if n != 'decoder.conv.bias':
            worst = max(worst, (e, n))
        if not e < GATE:
            bad.append((n, e))
    print(f'[{tag}] worst rel-L2 {worst[0]:.2e} ({worst[1]})')
    assert not bad, (tag, bad)


def _refine_exactly_zero(got):
    for n, g in got.items():
        if n.startswith('refine.'):
            assert g is None or not g.any(), n


# ---- 1. all frames, all six tensors, aux alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,arch,prec', [('base_f16x3', BASE, 1), ('base_fp32', BASE, 0), ('ws_f16x3', WS, 1)],
                         ids=['base_f16x3', 'base_fp32', 'ws_f16x3'])
def test_all_frames_aux_alone_matches_oracle(name, arch, prec):
    params, x, eps = _inputs(arch)
    W = F.weights(arch, B, 60, range(arch.iters + 1))
    m = make_hip_model(arch, params, options={'conv_precision': prec})
    got = _hip_grads(m, x, eps, W)
    ref, _, _ = F.grads(x, eps, params, arch, W)
    assert all(ref[n].any() for n in ('posterior.init_mean', 'posterior.init_logvar'))
    _check(got, ref, W, 'all frames, ' + name, init=True)


# ---- 2. one frame, one kind ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def base_case():
    params, x, eps = _inputs(BASE)
    return params, x, eps, F.weights(BASE, B, 60, range(BASE.iters + 1)), make_hip_model(BASE, params)


@pytest.mark.parametrize('i', [0, 1, BASE.iters])
def test_single_frame_matches_oracle(base_case, i):
    params, x, eps, W, m = base_case
    Wi = {k: w for k, w in W.items() if k[0] == i}
    got = _hip_grads(m, x, eps, Wi)
    _check(got, F.grads(x, eps, params, BASE, Wi)[0], Wi, f'frame {i} alone', init=True)
    if i == 0:
        _refine_exactly_zero(got)
    else:
        assert all(got[n] is None or not got[n].any() for n in ('posterior.init_mean', 'posterior.init_logvar'))


@pytest.mark.parametrize('kind', KEYS)
def test_single_kind_on_frame_1_matches_oracle(base_case, kind):
    params, x, eps, W, m = base_case
    Wk = {(1, kind): W[(1, kind)]}
    got = _hip_grads(m, x, eps, Wk)
    _check(got, F.grads(x, eps, params, BASE, Wk)[0], Wk, 'frame 1, only ' + kind)


# ---- 3. loss + aux ------------------------------------------------------------------------------------------------------------------------
def test_loss_plus_aux_matches_oracle_and_is_additive(base_case):
    params, x, eps, W, m = base_case
    both = _hip_grads(m, x, eps, W, 1.0)
    _check(both, F.grads(x, eps, params, BASE, W, 1.0)[0], W, 'loss + aux', init=True)
    both = {n: g.clone() for n, g in both.items()}
    g_loss = {n: g.clone() for n, g in _hip_grads(m, x, eps, {}, 1.0, frames=True).items()}
    g_aux = {n: g.clone() for n, g in _hip_grads(m, x, eps, W).items()}
    half = _hip_grads(m, x, eps, W, 0.5)                                     # grad_loss must not scale the auxiliary part
    for n in both:
        e1 = rel_l2(both[n].cpu().numpy(), (g_loss[n] + g_aux[n]).cpu().numpy())
        e2 = rel_l2(half[n].cpu().numpy(), (0.5 * g_loss[n] + g_aux[n]).cpu().numpy())
        assert e1 < 1e-5 and e2 < 1e-5, (n, e1, e2)


# ---- 4. unchanged behaviour, bitwise ------------------------------------------------------------------------------------------------------
def _plain_run(params, x, eps, **kw):
    m = make_hip_model(BASE, params)
    loss = m(x.to(DEV), eps.to(DEV), **kw)
    state = dict(z=m.z, mean=m.mean, mask=m.mask, mask_logits=m.mask_logits, post_mean=m.posterior.mean, post_logvar=m.posterior.logvar)
    frames = m.frames
    loss.backward()
    torch.cuda.synchronize()
    return (m, loss.detach().clone(), m.elbo_terms.clone(), {k: t.detach().clone() for k, t in state.items()},
            {n: p.grad.clone() for n, p in m.named_parameters()}, frames)


def test_attach_frames_changes_no_bit(base_case):
    params, x, eps, W, _ = base_case
    T = BASE.iters
    m0, l0, e0, t0, g0, f0 = _plain_run(params, x, eps)
    assert f0 is None and m0.frames is None
    for af in (True, ()):
        _, l1, e1, t1, g1, f1 = _plain_run(params, x, eps, attach_frames=af)
        assert torch.equal(l0, l1) and torch.equal(e0, e1)
        assert all(torch.equal(t0[k], t1[k]) for k in t0)
        assert all(torch.equal(g0[n], g1[n]) for n in g0)
        assert f1['index'] == (tuple(range(T + 1)) if af is True else ())
        assert all(f1[k].shape[0] == len(f1['index']) for k in KEYS)
    # entry T of every tensor is the attach_state tensor of the same inputs
    _, _, _, ta, _, _ = _plain_run(params, x, eps, attach_state=True)
    _, _, _, _, _, f1 = _plain_run(params, x, eps, attach_frames=True)
    assert all(f1[k].requires_grad and f1[k].grad_fn is not None for k in KEYS)
    assert all(torch.equal(f1[k][T], ta[k]) and torch.equal(f1[k][T], t0[k]) for k in KEYS)
    # under no_grad: the same values, detached; a forward without the argument clears model.frames
    m = make_hip_model(BASE, params)
    with torch.no_grad():
        m(x.to(DEV), eps.to(DEV), attach_frames=True)
    assert all(not m.frames[k].requires_grad and torch.equal(m.frames[k], f1[k]) for k in KEYS)
    with torch.no_grad():
        m(x.to(DEV), eps.to(DEV))
    assert m.frames is None


def test_cotangents_on_final_state_and_on_frame_T_add(base_case):
    params, x, eps, W, m = base_case
    T = BASE.iters
    Wm = W[(T, 'mask')].to(DEV, torch.float32)
    W2 = F.weights(BASE, B, 61, [T])[(T, 'mask')].to(DEV, torch.float32)
    Wz = W[(T, 'z')].to(DEV, torch.float32)

    def run(terms):
        m.zero_grad(set_to_none=True)
        m(x.to(DEV), eps.to(DEV), attach_state=True, attach_frames=[T])
        terms(m).backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    split = run(lambda m: (Wm * m.mask).sum() + (W2 * m.frames['mask'][0]).sum() + (Wz * m.z).sum() + (Wz * m.frames['z'][0]).sum())
    one = run(lambda m: ((Wm + W2) * m.mask).sum() + (2 * Wz * m.z).sum())
    for n in one:
        e = rel_l2(*grad_views(n, split[n].cpu().numpy(), one[n].cpu().numpy()))
        assert e < 1e-6, (n, e)


# One autograd node serves every un-chunked forward: whatever outputs are asked for, ``loss.backward()`` alone computes the plain step.
MATRIX = [(a, f, s) for s in (False, True) for a in (False, True) for f in (None, (), (1,), True)]
MATRIX_IDS = [f"{'state' if s else 'init'}-{'attach' if a else 'plain'}-frames_{f}" for a, f, s in MATRIX]


def _step(m, x, eps, state, **kw):
    """(loss, ELBO terms, {name: .grad or None}) of one forward + ``loss.backward()``"""
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV), state=state, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), m.elbo_terms.clone(), {n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()}


def _same_step(got, ref, tag):
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), tag
    for n, g in ref[2].items():
        assert (got[2][n] is None) == (g is None), (tag, n)
        assert g is None or torch.equal(got[2][n], g), (tag, n)


@pytest.fixture(scope='module')
def matrix_case(base_case):
    """an eager and a graph-mode model, a detached state a forward over other inputs kept, the plain step from it and from the initial posterior"""
    params, x, eps, _, _ = base_case
    m = make_hip_model(BASE, params)
    _, x2, eps2 = _inputs(BASE, seed=90)
    with torch.no_grad():
        m(x2.to(DEV), eps2.to(DEV), keep_state=True)
    state = tuple(t.detach() for t in m.refinement_state())
    plain = {s: _step(m, x, eps, state if s else None) for s in (False, True)}
    for s, (_, _, g) in plain.items():
        assert all((g[n] is None) == (s and n.startswith('posterior.')) for n in g)
        assert all(bool(t.any()) for n, t in g.items() if t is not None and (n.endswith('.weight') or n.startswith('posterior.')))
    assert not torch.equal(plain[False][0], plain[True][0])
    return m, make_hip_model(BASE, params, options={'graph': 1}), state, plain


def _frames_as_asked(m, frames):
    if frames is None:
        assert m.frames is None
        return
    index = tuple(range(BASE.iters + 1)) if frames is True else frames
    assert m.frames['index'] == index and all(m.frames[k].shape[0] == len(index) for k in KEYS)


@pytest.mark.parametrize('attach,frames,from_state', MATRIX, ids=MATRIX_IDS)
def test_outputs_asked_for_change_no_bit_of_the_plain_step(base_case, matrix_case, attach, frames, from_state):
    _, x, eps, _, _ = base_case
    m, _, state, plain = matrix_case
    got = _step(m, x, eps, state if from_state else None, attach_state=attach, attach_frames=frames)
    _frames_as_asked(m, frames)
    _same_step(got, plain[from_state], 'eager')


@pytest.mark.parametrize('attach,frames,from_state', MATRIX, ids=MATRIX_IDS)
def test_outputs_asked_for_change_no_bit_under_graph_replay(base_case, matrix_case, attach, frames, from_state):
    _, x, eps, _, _ = base_case
    _, mg, state, plain = matrix_case
    for step in range(3):                                                    # eager or captured, then replayed
        got = _step(mg, x, eps, state if from_state else None, attach_state=attach, attach_frames=frames)
        _frames_as_asked(mg, frames)
        _same_step(got, plain[from_state], f'graph step {step}')
    assert mg.profile_read('graph_replays')[1] > 0


# ---- 5. values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arch', [BASE, WS], ids=['base', 'ws'])
def test_attached_values_match_the_fp32_oracle(arch):
    params, x, eps = _inputs(arch, clip=True)
    m = make_hip_model(arch, params)
    with torch.no_grad():
        m(x.to(DEV), eps.to(DEV), attach_frames=True)
    q = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ref = F.forward(x, eps, q, arch)['evals']
    # the tolerances tests/test_gpu_clip_frames.py uses for trajectory entries; it has no figure for the logits: 1e-4, its tighter one
    errs = {k: max(rel_err(m.frames[k][i].cpu(), t[k].detach()) for i, t in enumerate(ref)) for k in KEYS}
    print(' '.join(f'{k} {e:.2e}' for k, e in errs.items()))
    for k, e in errs.items():
        assert e < (1e-4 if k == 'mask_logits' else 2e-4), (k, e)


# ---- 6. edges -----------------------------------------------------------------------------------------------------------------------------
EDGES = {
    # name: (arch, library options, clip?)
    'T1': (dataclasses.replace(BASE, iters=1), {}, False),
    'K1': (dataclasses.replace(BASE, slots=1), {}, False),                   # on the 'blobs' scene: see EDGES of tests/test_gpu_train_aux.py
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
    W = F.weights(arch, B, 71, range(arch.iters + 1))
    m = make_hip_model(arch, params, options=options)
    got = _hip_grads(m, x, eps, W, 0.5)
    assert bool(torch.isfinite(m.elbo_terms).all()), 'the forward itself is not finite on these inputs'
    _check(got, F.grads(x, eps, params, arch, W, 0.5)[0], W, name + ', 0.5 loss + aux', init=True)


def test_pixel_weights_edge(base_case):
    params, x, eps, W, m = base_case
    w = torch.rand((B, 1, BASE.img_size, BASE.img_size), generator=torch.Generator().manual_seed(5), dtype=torch.float64) + 0.25
    w[:, :, 3:9, 2:7] = 0.0
    got = _hip_grads(m, x, eps, W, 1.0, weights=w.float().to(DEV))
    _check(got, F.grads(x, eps, params, BASE, W, 1.0, pixel_w=w)[0], W, 'weights=', init=True)


@functools.lru_cache(maxsize=None)
def _entry_state():
    """a (lambda, h, c) to start from: what a forward over other inputs leaves (float64 reference, exact in float32)"""
    params, x, eps = _inputs(BASE, seed=90)
    q = {k: v.double().requires_grad_(True) for k, v in params.items()}
    return tuple(t.detach().float() for t in F.forward(x.double(), eps.double(), q, BASE)['state'])


def test_forward_from_a_detached_state(base_case):
    params, x, eps, W, m = base_case
    state = _entry_state()
    W0 = {k: w for k, w in W.items() if k[0] == 0}
    got = _hip_grads(m, x, eps, W0, state=tuple(t.to(DEV) for t in state))
    assert got['posterior.init_mean'] is None and got['posterior.init_logvar'] is None
    _refine_exactly_zero(got)
    _check(got, F.grads(x, eps, params, BASE, W0, init=state)[0], W0, 'frame 0 from a detached state')
    got = _hip_grads(m, x, eps, W, 1.0, state=tuple(t.to(DEV) for t in state))
    _check(got, F.grads(x, eps, params, BASE, W, 1.0, init=state)[0], W, 'all frames + loss from a detached state')


def test_forward_from_a_state_that_requires_grad(base_case):
    params, x, eps, W, m = base_case
    state = _entry_state()
    leaves = tuple(t.to(DEV).requires_grad_(True) for t in state)
    Wp = {(0, 'post_mean'): W[(0, 'post_mean')]}
    _hip_grads(m, x, eps, Wp, state=leaves)
    assert rel_l2(leaves[0].grad.cpu().numpy(), Wp[(0, 'post_mean')].numpy()) < 1e-6
    assert leaves[1].grad is None or not leaves[1].grad.any()
    leaves = tuple(t.to(DEV).requires_grad_(True) for t in state)
    got = _hip_grads(m, x, eps, W, 1.0, state=leaves)
    ref, gs, _ = F.grads(x, eps, params, BASE, W, 1.0, init=state)
    _check(got, ref, W, 'all frames + loss from a state with grad')
    for n, l, r in zip(('post_mean', 'post_logvar', 'h', 'c'), leaves, gs):
        e = rel_l2(l.grad.cpu().numpy(), r.numpy())
        assert e < GATE, (n, e)


def test_subset_list_on_T3():
    arch = dataclasses.replace(BASE, iters=3)
    params, x, eps = _inputs(arch, seed=70)
    W = F.weights(arch, B, 71, [1])
    m = make_hip_model(arch, params)
    got = _hip_grads(m, x, eps, W, frames=[1])
    assert m.frames['index'] == (1,) and m.frames['mask'].shape[0] == 1
    _check(got, F.grads(x, eps, params, arch, W)[0], W, 'subset [1] on T = 3')


# ---- 7. graph mode ------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_over_three_steps():
    params, _, _ = _inputs(BASE)
    m = make_hip_model(BASE, params, options={'graph': 1})
    for step in range(3):                                                    # eager, captured, replayed - fresh inputs every step
        _, x, eps = _inputs(BASE, seed=80 + 3 * step)
        W = F.weights(BASE, B, 90 + step, range(BASE.iters + 1))
        got = _hip_grads(m, x, eps, W, 1.0)
        _check(got, F.grads(x, eps, params, BASE, W, 1.0)[0], W, f'graph step {step}', init=True)
    assert m.profile_read('graph_replays')[1] > 0


# ---- 8. refusals and order ----------------------------------------------------------------------------------------------------------------
def test_bad_lists_are_refused_before_any_launch(base_case):
    params, x, eps, W, m = base_case
    T = BASE.iters
    m(x.to(DEV), eps.to(DEV)).backward()
    serial = m._call_serial
    for bad in ([T + 1], [-1], [1, 1], [0.5], 'ab', 3, [True]):
        with pytest.raises(ValueError):
            m(x.to(DEV), eps.to(DEV), attach_frames=bad)
    assert m._call_serial == serial                                          # no library call was made
    m(x.to(DEV), eps.to(DEV), attach_frames=[T, 0])                          # sorted
    assert m.frames['index'] == (0, T)
    # the library itself: refused with IODINE_ERR_INVALID, and the saved forward stays
    L = _lib.lib()
    n = sum(p.numel() for p in m.parameters())
    flat = torch.zeros((n,), device=DEV)
    gz = torch.zeros((2, B, BASE.slots, BASE.dim_latent), device=DEV)
    ptrs = (C.c_void_p * 6)(gz.data_ptr(), None, None, None, None, None)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda idx, k, p: L.iodine_train_backward_frames(m._handle, st, None, None, None, None, None, None, None, None, None,
                                                            _lib.ptr(flat), 0, None, idx, k, p)
    for idx in ((1, 0), (1, 1), (0, T + 1), (-1, 0)):
        assert call((C.c_int * 2)(*idx), 2, ptrs) == 1, idx
    assert call((C.c_int * 2)(0, 1), -1, ptrs) == 1
    assert call(None, 2, ptrs) == 1 and call((C.c_int * 2)(0, 1), 2, None) == 1
    assert call((C.c_int * 2)(0, 1), 2, ptrs) == 0                           # ... and this one differentiates it
    torch.cuda.synchronize()


def test_second_backward_is_a_stale_forward(base_case):
    params, x, eps, W, m = base_case
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV), attach_frames=True)
    F.hip_aux(m, W).backward()
    with pytest.raises(RuntimeError, match='stale forward'):
        loss.backward()


def test_attach_frames_above_max_batch_is_refused(base_case):
    params, x, eps, _, _ = base_case
    m = make_hip_model(BASE, params, options={'batch_cap': 1})
    with pytest.raises(RuntimeError, match=r'attach_frames.*max_batch\(training=True\) = 1'):
        m(x.to(DEV), eps.to(DEV), attach_frames=[0])


def test_cabi_without_frames_is_the_seq_backward_bitwise_and_redecode_hides_the_elbo_outputs(base_case):
    params, x, eps, W, _ = base_case
    m = make_hip_model(BASE, params)
    L = _lib.lib()
    K, Lz, H, S_ = BASE.slots, BASE.dim_latent, BASE.ref_mlp, BASE.img_size
    n = sum(p.numel() for p in m.parameters())
    gl = torch.full((), 0.75, device=DEV)
    gh = torch.from_numpy(synth.normal((B, K, H), seed=7)).to(DEV)
    gm = W[(1, 'mask')].float().to(DEV).contiguous()
    flats = []
    none = (C.c_void_p * 6)(None, None, None, None, None, None)
    for entry in ('seq', 'frames', 'frames_no_cotangent'):
        with torch.no_grad():
            m(x.to(DEV), eps.to(DEV))
        flat = torch.full((n,), float('nan'), device=DEV)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = (m._handle, st, _lib.ptr(gl), None, _lib.ptr(gm), None, None, None, None, _lib.ptr(gh), None, _lib.ptr(flat), 0, None)
        if entry == 'seq':
            rc = L.iodine_train_backward_seq(*args)
        elif entry == 'frames':
            rc = L.iodine_train_backward_frames(*args, None, 0, None)
        else:                                                                # a list, but no cotangent on it: nothing to add
            rc = L.iodine_train_backward_frames(*args, (C.c_int * 2)(0, 1), 2, none)
        _lib.check(rc, m._handle, entry)
        torch.cuda.synchronize()
        flats.append(flat)
    assert torch.equal(flats[0], flats[1]) and torch.equal(flats[0], flats[2]) and bool(flats[0].any())
    # no re-decode so far: the final elbo()'s outputs are still readable
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mask = torch.empty((B, K, 1, S_, S_), device=DEV)
    assert L.iodine_last_elbo_outputs(m._handle, st, B, None, None, _lib.ptr(mask), None, None) == 0
    # a backward that decodes evaluation 1 again: iodine_last_elbo_outputs refuses, the posterior and the LSTM state stay readable
    with torch.no_grad():
        m(x.to(DEV), eps.to(DEV))
    ptrs = (C.c_void_p * 6)(None, None, gm.data_ptr(), None, None, None)
    rc = L.iodine_train_backward_frames(m._handle, st, _lib.ptr(gl), None, None, None, None, None, None, None, None, _lib.ptr(flats[1]), 0,
                                        None, (C.c_int * 1)(1), 1, ptrs)
    _lib.check(rc, m._handle, 'iodine_train_backward_frames')
    assert L.iodine_last_elbo_outputs(m._handle, st, B, None, None, _lib.ptr(mask), None, None) == 3
    pm = torch.empty((B, K, Lz), device=DEV)
    hh = torch.empty((B, K, H), device=DEV)
    assert L.iodine_last_posterior(m._handle, st, B, _lib.ptr(pm), None) == 0
    assert L.iodine_last_train_state(m._handle, st, B, _lib.ptr(hh), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(pm, m.posterior.mean)


# ---- 9. engine.clip_backward(frame_loss=...) -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip_case():
    Bc, K, T = 3, 3, S.T
    a = S.arch(K)
    p, clip, eps = S.inputs(a, Bc)
    shp = (Bc, K, 1, a.img_size, a.img_size)
    Wf = [torch.from_numpy(np.random.default_rng(700 + f).standard_normal(shp)) for f in range(2 * T + 1)]
    return a, p, clip, eps, Wf


@pytest.mark.parametrize('bptt', ['exact', 'truncated'])
def test_clip_backward_with_frame_loss(bptt):
    a, p, clip, eps, Wf = _clip_case()
    T = S.T
    m = make_hip_model(a, p)
    m.iter_weights = S.W_CHUNK
    seen, parts = [], []

    def frame_loss(f, t):
        seen.append(f)
        assert set(t) == set(KEYS) and t['mask'].shape == Wf[f].shape
        parts.append((Wf[f].to(DEV, torch.float32) * t['mask']).sum())
        return parts[-1]
    m.zero_grad(set_to_none=True)
    loss, terms, aux_total = clip_backward(m, clip.to(DEV), eps.to(DEV), bptt=bptt, frame_loss=frame_loss)
    torch.cuda.synchronize()
    assert sorted(seen) == list(range(2 * T + 1))                            # each frame scored once
    assert tuple(terms.shape) == (2 * T + 1, 3)
    if bptt == 'exact':
        ref, _, _ = F.grads(clip, eps, p, a, {(f, 'mask'): Wf[f] for f in range(2 * T + 1)}, 1.0, w=S.W_LONG)
    else:
        W1 = {(i, 'mask'): Wf[i] for i in range(T + 1)}
        W2 = {(i, 'mask'): Wf[T + i] for i in range(1, T + 1)}
        g1, _, o1 = F.grads(clip[:, :T + 1], eps[:T + 1], p, a, W1, 1.0, w=S.W_CHUNK)
        g2, _, o2 = F.grads(clip[:, T:], eps[T:], p, a, W2, 1.0, w=S.W_LATER, init=tuple(t.detach() for t in o1['state']))
        ref = {n: (g1[n] if g1[n] is not None else 0) + (g2[n] if g2[n] is not None else 0) for n in g1}
    got = {n: q.grad for n, q in m.named_parameters()}
    _check(got, ref, {(0, 'mask'): None}, 'clip_backward ' + bptt, init=True)
    total = float(sum(float(t.detach()) for t in parts))                     # the sum over the five frames
    assert abs(float(aux_total) - total) <= 1e-5 * max(1.0, abs(total)), (float(aux_total), total)
