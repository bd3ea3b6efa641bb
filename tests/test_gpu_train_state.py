"""Training from a carried state: ``forward(x, state=..., keep_state=..., attach_state=...)``, iodine_train_forward_seq /
iodine_train_backward_seq / iodine_last_train_state and ``engine.clip_backward`` (truncated and exact BPTT over a clip).

Ground truth: the float64 composition of tests/train_state_reference.py (the oracle's pieces; test_train_state_cpu pins that its exact
composition IS the long forward).  Gate: rel-L2 < 1e-3 per gradient tensor, the project's gate for oracle-vs-HIP gradients
(tests/test_gpu_train.py, test_gpu_train_aux.py), with their ``decoder.conv.bias`` handling (util.grad_views).

Shapes: the tiny architecture (S = 16, L = 8, 32 channels) at T = 2 iterations per chunk, the moving clip of 5 frames of
tests/clip_reference.py (seeds 131 / 132 / 133); B = 3, K = 3 (N = 9 rows: odd, so the head kernel's 2-row blocks end in a tail block) and
(B, K) = (1, 1).

Reported, not gated (exact BPTT by recomputation against ONE long forward at T = 4, both on the GPU, B = 3 / K = 3, default options):
worst rel-L2 over the parameters 9.98e-08 (refine.mlp.layers.0.weight) - the two runs differ by summation order only."""
import ctypes as C
import functools

import pytest
import torch

from iodine_amd import _lib
from iodine_amd.engine import clip_backward
from util import grad_views, make_hip_model, rel_l2

import train_state_reference as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-3
T = S.T

# name: (arch overrides, library options)
CONFIGS = {
    'split_f16x3': ({}, {}),
    'exact_fp32': ({}, {'conv_precision': 0}),
    'head_unfused': ({}, {'head_fused': 0}),
    'padded_L6_H30': (dict(dim_latent=6, ref_mlp=30), {}),
    'padded_unfused': (dict(dim_latent=6, ref_mlp=30), {'head_fused': 0}),
}
HEAD_CONFIGS = ('split_f16x3', 'head_unfused', 'padded_L6_H30', 'padded_unfused')


@functools.lru_cache(maxsize=None)
def _case(B, K, arch_kw=()):
    """inputs and float64 references of one (B, K, arch), computed once and shared (nothing below writes into them)"""
    a = S.arch(K, **dict(arch_kw))
    p, clip, eps = S.inputs(a, B)
    state = tuple(t.float() for t in S.state_after_first_chunk(clip, eps, p, a))       # chunk 2's entry state, exact in float32
    return dict(a=a, p=p, clip=clip, eps=eps, state=state)


@functools.lru_cache(maxsize=None)
def _ref(B, K, arch_kw, what):
    c = _case(B, K, arch_kw)
    if what == 'long':
        return S.long_grads(c['clip'], c['eps'], c['p'], c['a'])[1]
    if what == 'truncated':
        return S.chunked_grads(c['clip'], c['eps'], c['p'], c['a'], exact=False)[2]
    raise KeyError(what)


def _model(c, options=None, weights=S.W_CHUNK):
    m = make_hip_model(c['a'], c['p'], options=options)
    m.iter_weights = weights
    return m


def _dev(c):
    return c['clip'].to(DEV), c['eps'].to(DEV)


def _param_errs(m, ref):
    out = []
    for n, p in m.named_parameters():
        g = torch.zeros_like(p) if p.grad is None else p.grad
        out.append((n, rel_l2(*grad_views(n, g.cpu().numpy(), ref[n].numpy()))))
    return out


def _check_params(m, ref, tag):
    errs = _param_errs(m, ref)
    print(f'[{tag}] worst rel-L2 {max(e for _, e in errs):.2e}')
    bad = [(n, e) for n, e in errs if not e < GATE]
    assert not bad, (tag, bad)


def _check_state_grads(leaves, ref, tag):
    errs = [(n, rel_l2(torch.zeros_like(l).cpu().numpy() if l.grad is None else l.grad.cpu().numpy(), r.numpy()))
            for n, l, r in zip(('post_mean', 'post_logvar', 'h', 'c'), leaves, ref)]
    print(f'[{tag}] state gradients', ' '.join(f'{n} {e:.2e}' for n, e in errs))
    bad = [(n, e) for n, e in errs if not e < GATE]
    assert not bad, (tag, bad)


def _leaves(c):
    return tuple(t.to(DEV).clone().requires_grad_(True) for t in c['state'])


# ---- 1. values: T = 4 equals T = 2 followed by T = 2 from the state ------------------------------------------------------------------
@pytest.mark.parametrize('B,K', [(3, 3), (1, 1)])
def test_value_chain_is_the_long_forward_bitwise(B, K):
    c = _case(B, K)
    clip, eps = _dev(c)
    m = _model(c, weights=None)
    with torch.no_grad():
        m.n_iters = 2 * T
        m(clip, eps, keep_state=True)
        long_terms, long_state = m.elbo_terms.clone(), m.refinement_state()
        long_post = (m.posterior.mean.clone(), m.posterior.logvar.clone())
        m.n_iters = T
        m(clip[:, :T + 1], eps[:T + 1], keep_state=True)
        t1, st = m.elbo_terms.clone(), m.refinement_state()
        m(clip[:, T:], eps[T:], state=st, keep_state=True)
        t2 = m.elbo_terms.clone()
    assert torch.equal(long_terms[:T + 1], t1) and torch.equal(long_terms[T:], t2)
    assert torch.equal(m.posterior.mean, long_post[0]) and torch.equal(m.posterior.logvar, long_post[1])
    assert all(torch.equal(a, b) for a, b in zip(m.refinement_state(), long_state))
    assert torch.equal(long_state[0], long_post[0]) and bool(long_state[2].any()) and bool(long_state[3].any())
    # h / c as the reference's (B * K, H)
    with torch.no_grad():
        m(clip[:, T:], eps[T:], state=(st[0], st[1], st[2].reshape(B * K, -1), st[3].reshape(B * K, -1)))
    assert torch.equal(m.elbo_terms, t2)


# ---- 2. the zero state is the initial state --------------------------------------------------------------------------------------------
def test_zero_state_gives_the_bits_of_the_plain_forward():
    c = _case(3, 3)
    clip, eps = _dev(c)
    x, e = clip[:, :T + 1], eps[:T + 1]
    m = _model(c)
    m.zero_grad(set_to_none=True)
    loss = m(x, e)
    terms = m.elbo_terms.clone()
    loss.backward()
    plain = {n: p.grad.clone() for n, p in m.named_parameters()}
    a = c['a']
    B, K = 3, 3
    state = (m.posterior.init_mean.detach()[None, None].repeat(B, K, 1), m.posterior.init_logvar.detach()[None, None].repeat(B, K, 1),
             torch.zeros(B, K, a.ref_mlp, device=DEV), torch.zeros(B, K, a.ref_mlp, device=DEV))
    m.zero_grad(set_to_none=True)
    loss2 = m(x, e, state=state)
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(m.elbo_terms, terms)
    loss2.backward()
    for n, p in m.named_parameters():
        if n.startswith('posterior.'):
            assert p.grad is None, n                        # not part of a forward from a state
        else:
            assert torch.equal(p.grad, plain[n]), n


# ---- 3. + 6. clip_backward: truncated and exact BPTT against the float64 compositions ---------------------------------------------------
def _clip_grads(c, options, bptt):
    clip, eps = _dev(c)
    m = _model(c, options)
    m.zero_grad(set_to_none=True)
    loss, terms = clip_backward(m, clip, eps, bptt=bptt)
    torch.cuda.synchronize()
    assert m.iter_weights == S.W_CHUNK and tuple(terms.shape) == (2 * T + 1, 3)
    return m, loss, terms


@pytest.mark.parametrize('name', list(CONFIGS))
def test_truncated_gradients_match_the_reference(name):
    arch_kw, options = CONFIGS[name]
    kw = tuple(sorted(arch_kw.items()))
    c = _case(3, 3, kw)
    m, _, _ = _clip_grads(c, options, 'truncated')
    _check_params(m, _ref(3, 3, kw, 'truncated'), 'truncated, ' + name)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_exact_gradients_match_the_long_forward(name):
    arch_kw, options = CONFIGS[name]
    kw = tuple(sorted(arch_kw.items()))
    c = _case(3, 3, kw)
    m, _, _ = _clip_grads(c, options, 'exact')
    _check_params(m, _ref(3, 3, kw, 'long'), 'exact, ' + name)


def test_one_slot_one_image():
    c = _case(1, 1)
    m, _, _ = _clip_grads(c, {}, 'truncated')
    _check_params(m, _ref(1, 1, (), 'truncated'), 'truncated, B1 K1')
    m, _, _ = _clip_grads(c, {}, 'exact')
    _check_params(m, _ref(1, 1, (), 'long'), 'exact, B1 K1')


def test_the_two_modes_differ_and_recomputation_repeats_the_bits():
    c = _case(3, 3)
    clip, eps = _dev(c)
    mt, loss_t, terms_t = _clip_grads(c, {}, 'truncated')       # (its forwards are pass 1 of the exact mode: the same calls)
    me, loss_e, terms_e = _clip_grads(c, {}, 'exact')
    assert torch.equal(terms_t, terms_e) and torch.equal(loss_t, loss_e)
    gt, ge = mt.refine.lstm.weight_hh.grad.cpu().numpy(), me.refine.lstm.weight_hh.grad.cpu().numpy()
    d = rel_l2(gt, ge)
    print('refine.lstm.weight_hh: truncated vs exact rel-L2', d)
    assert d > 0.05
    # reported: exact BPTT by recomputation against one long forward at T = 4 on the GPU
    ml = _model(c, weights=S.W_LONG)
    ml.n_iters = 2 * T
    ml.zero_grad(set_to_none=True)
    ml(clip, eps).backward()
    errs = [(rel_l2(*grad_views(n, p.grad.cpu().numpy(), q.grad.cpu().numpy())), n)
            for (n, p), (_, q) in zip(me.named_parameters(), ml.named_parameters())]
    print('HIP exact vs HIP long forward: worst rel-L2 %.2e (%s)' % max(errs))
    assert torch.equal(terms_e, ml.elbo_terms)


# ---- 4. gradients of the state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', HEAD_CONFIGS)
def test_state_gradients_match_the_reference(name):
    arch_kw, options = CONFIGS[name]
    c = _case(3, 3, tuple(sorted(arch_kw.items())))
    clip, eps = _dev(c)
    m = _model(c, options)
    for w, tag in ((S.W_CHUNK, 'w0 != 0'), (S.W_LATER, 'w0 = 0')):
        m.iter_weights = w
        m.zero_grad(set_to_none=True)
        leaves = _leaves(c)
        m(clip[:, T:], eps[T:], state=leaves).backward()
        gp, gs, _ = S.second_chunk_grads(c['clip'], c['eps'], c['p'], c['a'], c['state'], w)
        _check_state_grads(leaves, gs, f'{name}, {tag}')
        _check_params(m, gp, f'{name}, {tag}')
        assert m.posterior.init_mean.grad is None and m.posterior.init_logvar.grad is None
        if w[0] == 0:
            assert not leaves[0].grad.any() and not leaves[1].grad.any()
        else:
            assert bool(leaves[0].grad.any()) and bool(leaves[1].grad.any())


def test_one_slot_state_gradients():
    c = _case(1, 1)
    clip, eps = _dev(c)
    m = _model(c)
    leaves = _leaves(c)
    m(clip[:, T:], eps[T:], state=leaves).backward()
    gp, gs, _ = S.second_chunk_grads(c['clip'], c['eps'], c['p'], c['a'], c['state'], S.W_CHUNK)
    _check_state_grads(leaves, gs, 'B1 K1')
    _check_params(m, gp, 'B1 K1')


# ---- 5. cotangents on lstm_hidden ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', HEAD_CONFIGS)
@pytest.mark.parametrize('g_loss', [0.0, 1.0], ids=['aux_alone', 'loss_plus_aux'])
def test_lstm_hidden_cotangents_match_the_reference(name, g_loss):
    arch_kw, options = CONFIGS[name]
    c = _case(3, 3, tuple(sorted(arch_kw.items())))
    a = c['a']
    clip, eps = _dev(c)
    g = torch.Generator().manual_seed(7)
    W_h, W_c = (torch.randn(3, 3, a.ref_mlp, generator=g, dtype=torch.float64) for _ in range(2))
    m = _model(c, options)
    m.zero_grad(set_to_none=True)
    leaves = _leaves(c)
    loss = m(clip[:, T:], eps[T:], state=leaves, attach_state=True)
    h, cc = m.lstm_hidden
    assert tuple(h.shape) == (9, a.ref_mlp) and h.requires_grad and cc.requires_grad
    aux = (W_h.float().to(DEV) * h.view(3, 3, -1)).sum() + (W_c.float().to(DEV) * cc.view(3, 3, -1)).sum()
    (aux + g_loss * loss if g_loss else aux).backward()
    gp, gs, out = S.second_chunk_grads(c['clip'], c['eps'], c['p'], c['a'], c['state'], S.W_CHUNK, g_loss, W_h, W_c)
    assert rel_l2(h.detach().view(3, 3, -1).cpu().numpy(), out['state'][2].detach().numpy()) < 2e-4
    assert rel_l2(cc.detach().view(3, 3, -1).cpu().numpy(), out['state'][3].detach().numpy()) < 2e-4
    _check_state_grads(leaves, gs, f'{name}, g_loss {g_loss}')
    _check_params(m, gp, f'{name}, g_loss {g_loss}')


def test_attach_state_changes_no_bit_and_sets_lstm_hidden():
    c = _case(3, 3)
    clip, eps = _dev(c)
    x, e = clip[:, :T + 1], eps[:T + 1]
    m = _model(c)
    m(x, e, keep_state=True)
    plain = (m.elbo_terms.clone(),) + m.refinement_state()
    assert m.lstm_hidden is None
    m(x, e, attach_state=True, keep_state=True)
    assert torch.equal(m.elbo_terms, plain[0]) and all(torch.equal(s, t) for s, t in zip(m.refinement_state(), plain[1:]))
    assert torch.equal(m.lstm_hidden[0].detach().view(3, 3, -1), plain[3]) and m.lstm_hidden[0].grad_fn is not None


# ---- 7. the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_cabi_null_arguments_are_the_existing_entries_bitwise():
    c = _case(3, 3)
    clip, eps = _dev(c)
    x, e = clip[:, :T + 1].contiguous(), eps[:T + 1].contiguous()
    m = _model(c, weights=None)
    with torch.no_grad():
        m(x, e)                                              # parameters, run shape, frames and workspace on the handle
    L, h = _lib.lib(), m._handle
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = sum(p.numel() for p in m.parameters())
    gl = torch.full((), 0.75, device=DEV)
    runs = []
    for new in (False, True):
        loss, terms = torch.zeros((), device=DEV), torch.zeros(T + 1, 3, device=DEV)
        flat = torch.full((n,), float('nan'), device=DEV)
        if new:
            _lib.check(L.iodine_train_forward_seq(h, st, 3, _lib.ptr(x), _lib.ptr(e), None, _lib.ptr(loss), _lib.ptr(terms)), h)
            _lib.check(L.iodine_train_backward_seq(h, st, _lib.ptr(gl), None, None, None, None, None, None, None, None, _lib.ptr(flat), 0, None), h)
        else:
            _lib.check(L.iodine_train_forward(h, st, 3, _lib.ptr(x), _lib.ptr(e), _lib.ptr(loss), _lib.ptr(terms)), h)
            _lib.check(L.iodine_train_backward_aux(h, st, _lib.ptr(gl), None, None, None, None, None, None, _lib.ptr(flat), 0), h)
        torch.cuda.synchronize()
        runs.append((loss, terms, flat))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and bool(runs[0][2].any())
    # the gradient of a state that the saved forward did not start from: IODINE_ERR_STATE, and the saved forward stays
    loss, flat = torch.zeros((), device=DEV), torch.zeros(n, device=DEV)
    _lib.check(L.iodine_train_forward_seq(h, st, 3, _lib.ptr(x), _lib.ptr(e), None, _lib.ptr(loss), None), h)
    gs = [torch.zeros(3, 3, d, device=DEV) for d in (c['a'].dim_latent, c['a'].dim_latent, c['a'].ref_mlp, c['a'].ref_mlp)]
    ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in gs])
    assert L.iodine_train_backward_seq(h, st, _lib.ptr(gl), None, None, None, None, None, None, None, None, _lib.ptr(flat), 0, ptrs) == 3
    assert b'g_state' in L.iodine_last_error(h)
    hh = torch.zeros(3, 3, c['a'].ref_mlp, device=DEV)
    assert L.iodine_last_train_state(h, st, 3, _lib.ptr(hh), None) == 0 and L.iodine_last_refine_state(h, st, 3, _lib.ptr(hh), None) == 3
    assert L.iodine_train_backward_seq(h, st, _lib.ptr(gl), None, None, None, None, None, None, None, None, _lib.ptr(flat), 0, None) == 0
    assert L.iodine_train_backward_seq(h, st, _lib.ptr(gl), None, None, None, None, None, None, None, None, _lib.ptr(flat), 0, None) == 3
    half = (C.c_void_p * 4)(gs[0].data_ptr(), gs[1].data_ptr(), None, None)
    assert L.iodine_train_forward_seq(h, st, 3, _lib.ptr(x), _lib.ptr(e), half, _lib.ptr(loss), None) == 1
    assert b'four' in L.iodine_last_error(h)
    torch.cuda.synchronize()
    assert torch.equal(flat, runs[0][2])


# ---- 8. refusals and bookkeeping -------------------------------------------------------------------------------------------------------
def test_refusals_and_bookkeeping():
    c = _case(3, 3)
    clip, eps = _dev(c)
    x, e = clip[:, T:], eps[T:]
    state = tuple(t.to(DEV) for t in c['state'])
    m = _model(c)
    for bad in (tuple(t[:2] for t in state), tuple(t[:, :2] for t in state), state[:3], (state[0], state[1], state[2][..., :4], state[3]),
                (state[0], state[1], state[2].reshape(3, -1), state[3])):
        with pytest.raises(RuntimeError, match='state'):
            m(x, e, state=bad)
    m(x, e, state=state)
    with pytest.raises(RuntimeError, match='keep_state'):
        m.refinement_state()
    leaves = _leaves(c)
    loss = m(x, e, state=leaves, attach_state=True)
    (m.lstm_hidden[0].sum() + loss).backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='stale forward'):
        loss.backward()
    m.set_option('batch_cap', 2)
    with pytest.raises(RuntimeError, match=r'requires grad.*max_batch\(training=True\) = 2'):
        m(x, e, state=_leaves(c))
    with pytest.raises(RuntimeError, match=r'max_batch\(training=True\) = 2'):
        m(x, e, state=state, attach_state=True)
    m.set_option('batch_cap', 0)


def test_chunked_batch_from_a_detached_state():
    c = _case(3, 3)
    clip, eps = _dev(c)
    x, e = clip[:, T:], eps[T:]
    state = tuple(t.to(DEV) for t in c['state'])
    runs = []
    for cap in (0, 2):
        m = _model(c, {'batch_cap': cap})
        m.zero_grad(set_to_none=True)
        loss = m(x, e, state=state, keep_state=True)
        loss.backward()
        assert m.posterior.init_mean.grad is None
        named = [('loss', loss.detach()), ('elbo_terms', m.elbo_terms.clone())] + list(zip(('pm', 'plv', 'h', 'c'), m.refinement_state()))
        runs.append(named + [(n, p.grad.clone()) for n, p in m.named_parameters() if not n.startswith('posterior.')])
    for (n, a), (_, b) in zip(*runs):
        e = rel_l2(*grad_views(n, a.cpu().numpy(), b.cpu().numpy()))
        assert e < 1e-6, (n, e)


# ---- 9. graph mode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bptt', ['truncated', 'exact'])
def test_graph_replay_over_three_clip_steps(bptt):
    c = _case(3, 3)
    clip, eps = _dev(c)
    eager, graphed = _model(c), _model(c, {'graph': 1})
    for step in range(3):                                    # eager, captured, replayed - another clip every step
        xs, es = torch.roll(clip, step, dims=-1), torch.roll(eps, step, dims=0)
        outs = []
        for m in (eager, graphed):
            m.zero_grad(set_to_none=True)
            loss, terms = clip_backward(m, xs, es, bptt=bptt)
            outs.append([loss, terms] + [p.grad.clone() for p in m.parameters()])
        assert all(torch.equal(a, b) for a, b in zip(*outs)), step
    assert graphed.profile_read('graph_replays')[1] > 0
