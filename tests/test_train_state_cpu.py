"""Training from a carried state, CPU side: the mathematics the GPU tests rely on (float64, the oracle's pieces composed in
tests/train_state_reference.py), the chunk arithmetic of ``engine.clip_chunks`` and the C ABI of the new entry points.

Two chunks of T = 2 against one forward at T = 4 with the same per-evaluation weights, moving clip of 5 frames, B = 3 and (B, K) = (1, 1)."""
import os
import re

import pytest
import torch

from iodine_amd import _lib
from iodine_amd.engine import clip_chunks
from util import rel_l2

import train_state_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(3, 3), (1, 1)]


@pytest.fixture(scope='module', params=CASES, ids=lambda bk: 'B%d_K%d' % bk)
def case(request):
    B, K = request.param
    a = S.arch(K)
    p, clip, eps = S.inputs(a, B, torch.float64)
    long_out, long_g = S.long_grads(clip, eps, p, a)
    return dict(a=a, p=p, clip=clip, eps=eps, long_out=long_out, long_g=long_g,
                exact=S.chunked_grads(clip, eps, p, a, exact=True), trunc=S.chunked_grads(clip, eps, p, a, exact=False))


def test_exact_composition_is_the_long_forward(case):
    o1, o2, g = case['exact']
    long_elbos = case['long_out']['elbos']
    # evaluation by evaluation the same numbers; the boundary frame is evaluated by both chunks
    assert all(torch.equal(a, b) for a, b in zip(o1['elbos'], long_elbos[:S.T + 1]))
    assert all(torch.equal(a, b) for a, b in zip(o2['elbos'], long_elbos[S.T:]))
    # ... so the clip loss, summed in the long forward's order, is the long forward's loss
    assert torch.equal(S.weighted_loss(o1['elbos'] + o2['elbos'][1:], S.W_LONG), case['long_out']['loss'])
    assert abs(float((o1['loss'] + o2['loss'] - case['long_out']['loss']).detach())) <= 1e-12 * abs(float(case['long_out']['loss'].detach()))
    errs = {n: rel_l2(g[n].numpy(), case['long_g'][n].numpy()) for n in g}
    print(max(errs.values()))
    assert all(e <= 1e-12 for e in errs.values()), errs


def test_truncated_composition_differs_in_the_refinement_network_only(case):
    o1, o2, g = case['trunc']
    long_g = case['long_g']
    assert all(torch.equal(a, b) for a, b in zip(o1['elbos'] + o2['elbos'][1:], case['long_out']['elbos']))      # the same loss
    for n in g:
        e = rel_l2(g[n].numpy(), long_g[n].numpy())
        if n.startswith(('decoder.', 'posterior.')):
            assert e <= 1e-12, (n, e)
    e = rel_l2(g['refine.lstm.weight_hh'].numpy(), long_g['refine.lstm.weight_hh'].numpy())
    print('refine.lstm.weight_hh: truncated vs exact rel-L2', e)
    assert e > 0.05


def test_state_gradient_reaches_lambda_through_evaluation_0_only(case):
    a, p, clip, eps = case['a'], case['p'], case['clip'], case['eps']
    state = S.state_after_first_chunk(clip, eps, p, a)
    _, gs, _ = S.second_chunk_grads(clip, eps, p, a, state, S.W_CHUNK)
    assert all(float(g.abs().max()) > 0 for g in gs)
    _, gs0, _ = S.second_chunk_grads(clip, eps, p, a, state, S.W_LATER)
    assert not gs0[0].any() and not gs0[1].any() and gs0[2].any() and gs0[3].any()


def test_clip_chunks():
    assert clip_chunks(3, 2) == [(0, 3)]
    assert clip_chunks(5, 2) == [(0, 3), (2, 5)]
    assert clip_chunks(11, 5) == [(0, 6), (5, 11)]
    assert clip_chunks(4, 1) == [(0, 2), (1, 3), (2, 4)]
    for F, T in ((1, 2), (2, 2), (4, 2), (6, 2), (0, 1), (5, 0), (5, -1), (5.5, 2), (5, 2.5)):
        with pytest.raises(ValueError):
            clip_chunks(F, T)


def _declaration(header, name):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    assert '#define IODINE_ABI_VERSION 3' in header
    new = ('iodine_train_forward_seq', 'iodine_train_backward_seq', 'iodine_last_train_state')
    for name in new:
        assert name in _lib.EXPORTS
    assert _declaration(header, 'iodine_train_forward_seq') == [
        'iodine_handle* h', 'void* stream', 'int batch', 'const float* x', 'const float* eps', 'const float* const* state_in', 'float* loss',
        'float* elbo_iter']
    assert _declaration(header, 'iodine_train_backward_seq') == [
        'iodine_handle* h', 'void* stream', 'const float* grad_loss_dev', 'const float* g_mean', 'const float* g_mask', 'const float* g_logits',
        'const float* g_z', 'const float* g_post_mean', 'const float* g_post_logvar', 'const float* g_lstm_h', 'const float* g_lstm_c',
        'float* flat_grads', 'int accumulate', 'float* const* g_state']
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.iodine_abi_version() == 3
        assert len(L.iodine_train_forward_seq.argtypes) == 8 and len(L.iodine_train_backward_seq.argtypes) == 14
        assert len(L.iodine_last_train_state.argtypes) == 5
