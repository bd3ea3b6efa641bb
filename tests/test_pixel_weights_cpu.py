"""Per-pixel observation weights (``weights=``) without a device: the reference restatement against the oracle, the power of the chosen
weight pattern to tell wrong compositions from the right one, the host-side refusals, the chunk slicing of clip weights, the ABI entry and
the engine flag.

Separations measured in float64 with the pattern of weights_reference.pattern (generator seed 5) on the inputs of objective_reference
(seed 211) at B = 2 - worst parameter-gradient rel-L2 of the training step, wrong composition vs the right one:

    architecture                        (a)     (b)     (c)     (d)
    tiny (K 3, T 2, S 16, L 8)          0.20    0.51    0.076   0.30
    generic (5, 5)                      0.18    0.39    0.12    0.30
    fused, tiny_arch(3, 2, 32, chan=64) 0.088   0.19    0.051   0.18

against the GPU gate 1e-3.  reconstruct (util.rel_err, max-norm): the posterior mean under (a) is off by 0.18 / 0.17 / 0.052 and under (c) by
1.5e-2 / 1.5e-2 / 5.2e-3 against the gate 2e-4; (b) and (d) show in the reported LL, 0.15 .. 0.32 against the gate 1e-4 ((b) leaves the
trajectory alone, and the layer norm takes (d)'s common scale out of the gradients again: posterior mean 2.6e-4 on tiny).  The tests assert
>= 10 x the gate, not these figures."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from iodine_amd import IODINE, _args, _lib, engine
from iodine_amd.model import arch_namespace
from oracle import iodine_oracle as O
from util import grad_views, rel_err, rel_l2

import weights_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2
GRAD_GATE, POST_GATE, TERM_GATE = 1e-3, 2e-4, 1e-4       # the GPU tests' gates: parameter-gradient rel-L2, inference tensors, ELBO terms
ARCHS = {
    'tiny': O.tiny_arch(),
    'generic': dataclasses.replace(O.tiny_arch(), ref_kernel=5, dec_kernel=5),
    'fused': O.tiny_arch(3, 2, 32, chan=64),
}


# ---- 1. at w = 1 the restatement IS the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize('arch_key', ['tiny', 'generic'])
def test_unit_weights_pin_the_oracle(arch_key):
    a = ARCHS[arch_key]
    params, x, eps = W.inputs(a, B)
    ones = torch.ones(B, 1, a.img_size, a.img_size)
    ref, gref = O.train_step_grads(x, eps, params, a)
    out, g = W.train_step_grads(x, ones, eps, params, a)
    for k in ('loss', 'elbos', 'kls', 'lls', 'post_mean', 'post_logvar', 'final_mask', 'final_mean'):
        assert torch.equal(out[k], ref[k]), k
    for n in gref:
        assert torch.equal(g[n], gref[n]), n
    rref = O.reconstruct(x, eps, params, a)
    rec = W.reconstruct(x, ones, eps, params, a)
    for k in rref:
        assert torch.equal(rec[k], rref[k]), k
    # the clip form with a per-frame weight of ones is the same computation again
    clip = x[:, None].expand(B, a.iters + 1, *x.shape[1:]).contiguous()
    out5, g5 = W.train_step_grads(clip, ones[:, None].expand(B, a.iters + 1, 1, a.img_size, a.img_size), eps, params, a)
    assert torch.equal(out5['loss'], ref['loss']) and all(torch.equal(g5[n], gref[n]) for n in gref)


def test_the_pattern_is_the_documented_one():
    w = W.pattern(B, 16)
    assert w.dtype == torch.float64 and tuple(w.shape) == (B, 1, 16, 16)
    assert W.rectangles(B, 16) == [(3, 2), (8, 9)]
    for i, (y0, x0) in enumerate(W.rectangles(B, 16)):
        assert float(w[i, :, y0:y0 + 6, x0:x0 + 5].abs().max()) == 0.0
        rest = w[i].clone()
        rest[:, y0:y0 + 6, x0:x0 + 5] = 1.0
        assert float(rest.min()) >= 0.25 and float(rest.max()) <= 1.5
    assert int((w == 0).sum()) == B * 30
    assert tuple(W.clip_pattern(B, 3, 16).shape) == (B, 3, 1, 16, 16)


# ---- 2. the pattern tells wrong builds from the right one --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def f64_steps():
    """{arch: (right outputs, right gradients, inputs)} in float64, computed once"""
    out = {}
    for key, a in ARCHS.items():
        params, x, eps = W.inputs(a, B, dtype=torch.float64)
        w = W.pattern(B, a.img_size)
        out[key] = (W.train_step_grads(x, w, eps, params, a), (params, x, eps, w))
    return out


@pytest.mark.parametrize('wrong', W.WRONG)
@pytest.mark.parametrize('arch_key', list(ARCHS))
def test_a_wrong_composition_of_the_training_step_is_visible(f64_steps, arch_key, wrong):
    """the worst parameter gradient of every wrong composition differs from the right one by >= 10 x the GPU gate"""
    a = ARCHS[arch_key]
    (_, good), (params, x, eps, w) = f64_steps[arch_key]
    _, bad = W.train_step_grads(x, w, eps, params, a, wrong=wrong)
    errs = {n: rel_l2(*grad_views(n, bad[n].numpy(), good[n].numpy())) for n in good}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f'({wrong}) {arch_key}: worst parameter gradient {worst[0]} {worst[1]:.3g}')
    assert worst[1] >= 10 * GRAD_GATE


@pytest.mark.parametrize('arch_key', list(ARCHS))
def test_a_wrong_composition_of_inference_is_visible(arch_key):
    """reconstruct: (a) and (c) move the posterior mean by >= 10 x its gate; (b) leaves the trajectory alone and (d) nearly so (the
    layer norm takes a common scale of the gradients out again): both show in the reported LL, by >= 10 x the gate of the ELBO terms"""
    a = ARCHS[arch_key]
    params, x, eps = W.inputs(a, B, dtype=torch.float64)
    w = W.pattern(B, a.img_size)
    good = W.reconstruct(x, w, eps, params, a)
    for wrong in ('a', 'c'):
        bad = W.reconstruct(x, w, eps, params, a, wrong=wrong)
        e = rel_err(bad['post_mean'], good['post_mean'])
        print(f'({wrong}) {arch_key}: posterior mean {e:.3g}')
        assert e >= 10 * POST_GATE, wrong
    for wrong in ('b', 'd'):
        bad = W.reconstruct(x, w, eps, params, a, wrong=wrong)
        e = rel_err(bad['lls'], good['lls'])
        print(f'({wrong}) {arch_key}: reported LL {e:.3g}')
        assert e >= 10 * TERM_GATE, wrong
        if wrong == 'b':
            assert torch.equal(bad['post_mean'], good['post_mean'])


def test_zero_weight_pixels_do_not_reach_the_objective():
    """the image inside the zero rectangles changes the per-pixel log-likelihood but not the weighted one, exactly"""
    a = ARCHS['tiny']
    params, x, eps = W.inputs(a, B, dtype=torch.float64)
    w = W.pattern(B, a.img_size)
    x2 = x.clone()
    for i, (y0, x0) in enumerate(W.rectangles(B, a.img_size)):
        x2[i, :, y0:y0 + 6, x0:x0 + 5] = 1.0 - x2[i, :, y0:y0 + 6, x0:x0 + 5]
    pm = params['posterior.init_mean'][None, None].repeat(B, a.slots, 1)
    plv = params['posterior.init_logvar'][None, None].repeat(B, a.slots, 1)
    t1, t2 = (W.w_terms(v, w, pm, plv, eps[0], params, a) for v in (x, x2))
    assert torch.equal(t1['ll'], t2['ll']) and not torch.equal(t1['ll_px'], t2['ll_px'])


# ---- 3. host validation, before any library call ----------------------------------------------------------------------------------
def _module(K=3, T=2):
    return IODINE(arch_namespace(8, T, K, 16, (32, 2, 32), (32, 2)))     # tiny arch, parameters on the CPU


def _calls(m, x, w):
    return (lambda: m.reconstruct(x, weights=w), lambda: m.encode(x, weights=w), lambda: m.weighted_elbo(x, w), lambda: m(x, weights=w))


@pytest.mark.parametrize('shape', [(1, 1, 16, 15), (2, 1, 16, 16), (1, 3, 16, 16), (16, 16), (1, 2, 1, 16, 16), (1, 1, 1, 1, 16, 16)], ids=str)
def test_a_wrong_weight_shape_is_refused_on_the_host(shape):
    m = _module()
    x = torch.zeros(1, 3, 16, 16)
    for call in _calls(m, x, torch.ones(shape)):
        with pytest.raises(RuntimeError, match=r'weights.*shape'):
            call()
    assert m._handle is None                                            # nothing reached the library


def test_per_frame_weights_need_a_clip():
    m = _module()
    x = torch.zeros(1, 3, 16, 16)
    for call in _calls(m, x, torch.ones(1, 2, 1, 16, 16)):
        with pytest.raises(RuntimeError, match=r'one weight image per frame.*single images'):
            call()
    # a clip takes them, with the frame count of the call: T for reconstruct, T + 1 for forward
    with pytest.raises(RuntimeError, match=r'weights must have shape'):
        m.reconstruct(torch.zeros(1, 2, 3, 16, 16), weights=torch.ones(1, 3, 1, 16, 16))
    with pytest.raises(RuntimeError, match=r'weights must have shape'):
        m(torch.zeros(1, 3, 3, 16, 16), weights=torch.ones(1, 2, 1, 16, 16))
    assert m._handle is None


@pytest.mark.parametrize('value', [1.0, [[1.0]], np.ones((1, 16, 16), dtype=np.float32), 'ones'], ids=lambda v: type(v).__name__)
def test_weights_that_are_no_tensor_are_refused(value):
    m = _module()
    x = torch.zeros(1, 3, 16, 16)
    for call in _calls(m, x, value):
        with pytest.raises(RuntimeError, match=r'weights must be a tensor'):
            call()
    with pytest.raises(RuntimeError, match=r'dtype'):
        m.reconstruct(x, weights=torch.ones(1, 16, 16, dtype=torch.int64))
    assert m._handle is None


def test_valid_weights_pass_the_host_checks():
    m = _module()
    x = torch.zeros(2, 3, 16, 16)
    for w in (torch.ones(2, 1, 16, 16), torch.ones(2, 16, 16, dtype=torch.float64), torch.ones(2, 16, 16, dtype=torch.bool),
              torch.ones(2, 1, 16, 16, dtype=torch.uint8), torch.ones(2, 16, 16, dtype=torch.float16),
              torch.ones(2, 1, 16, 16, requires_grad=True)):
        out = _args.check_weights(w, x, 16, 'forward')
        assert out.dtype == torch.float32 and tuple(out.shape) == (2, 16, 16) and out.is_contiguous() and not out.requires_grad
    clip = torch.zeros(2, 3, 3, 16, 16)
    assert tuple(_args.check_weights(torch.ones(2, 3, 1, 16, 16), clip, 16, 'forward').shape) == (2, 3, 16, 16)
    assert tuple(_args.check_weights(torch.ones(2, 3, 16, 16), clip, 16, 'forward').shape) == (2, 3, 16, 16)
    assert tuple(_args.check_weights(torch.ones(2, 1, 16, 16), clip, 16, 'forward').shape) == (2, 16, 16)     # a 4-D weight: every frame
    assert _args.check_weights(None, x, 16, 'forward') is None
    v = torch.rand(2, 3, 1, 16, 16)
    assert torch.equal(_args.check_weights(v.transpose(3, 4), clip, 16, 'forward'), v.transpose(3, 4)[:, :, 0])
    with pytest.raises(RuntimeError, match='ROCm device'):              # valid weights go on to the device check
        m.reconstruct(x, weights=torch.ones(2, 1, 16, 16))


# ---- 4. clip chunks ------------------------------------------------------------------------------------------------------------------
def test_clip_weight_chunks_are_index_exact():
    Bc, T, S = 2, 2, 4
    F = 3 * T + 1
    chunks = engine.clip_chunks(F, T)
    assert chunks == [(0, 3), (2, 5), (4, 7)]
    w5 = torch.arange(Bc * F * S * S, dtype=torch.float32).view(Bc, F, 1, S, S)
    shape = (Bc, F, 3, S, S)
    for lo, hi in chunks:
        for w in (w5, w5[:, :, 0]):
            part = engine.clip_weights(w, shape, (lo, hi))
            assert part.shape[1] == T + 1 and torch.equal(part, w[:, lo:hi])
            assert part.data_ptr() == w[:, lo].data_ptr()                # a view: frame lo of the clip's weights, the boundary frame included
    # consecutive chunks share their boundary frame, like the clip
    assert torch.equal(engine.clip_weights(w5, shape, chunks[0])[:, -1], engine.clip_weights(w5, shape, chunks[1])[:, 0])
    w4 = torch.rand(Bc, 1, S, S)
    assert engine.clip_weights(w4, shape, chunks[1]) is w4 and engine.clip_weights(w4[:, 0], shape, chunks[2]).shape == (Bc, S, S)
    assert engine.clip_weights(None, shape, chunks[0]) is None
    for bad in (torch.ones(Bc, F - 1, 1, S, S), torch.ones(Bc, S), torch.ones(Bc + 1, 1, S, S)):
        with pytest.raises(ValueError, match='weights must have shape'):
            engine.clip_weights(bad, shape, chunks[0])
    with pytest.raises(ValueError, match='tensor'):
        engine.clip_weights([1.0], shape, chunks[0])


def test_border_weights():
    w = engine.border_weights(2, 8, 2)
    assert tuple(w.shape) == (2, 1, 8, 8) and w.dtype == torch.float32
    assert float(w.sum()) == 2 * 16 and float(w[:, :, 2:6, 2:6].min()) == 1.0 and float(w[:, :, :2].max()) == 0.0
    assert float(engine.border_weights(1, 8, 0).min()) == 1.0
    for bad in (4, -1, 1.5, True):
        with pytest.raises(ValueError, match='border'):
            engine.border_weights(1, 8, bad)


# ---- 5. ABI, engine, documents ----------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_set_pixel_weights():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    assert re.search(r'\bint iodine_set_pixel_weights\(iodine_handle\* h, const float\* w_dev, int per_frame\);', header)
    assert 'ONE-SHOT' in header
    assert 'iodine_set_pixel_weights' in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, 'iodine_set_pixel_weights')
    assert L.iodine_set_pixel_weights(None, None, 0) == 1               # IODINE_ERR_INVALID on a null handle, no device touched
    assert L.iodine_abi_version() == 3                                  # additive: the ABI version stays
    for doc in ('README.md', 'DESIGN.md'):
        assert 'weights=' in open(os.path.join(ROOT, doc)).read(), doc


def test_engine_parser_takes_ignore_border():
    ap = engine.make_parser()
    assert ap.parse_args([]).ignore_border == 0
    assert ap.parse_args(['--ignore-border', '3']).ignore_border == 3


def test_train_passes_border_weights_to_the_model():
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))
            self.seen = []

        def forward(self, x, weights=None):
            self.seen.append(weights)
            return self.w * x.sum()

    m = Model()
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    data = [(torch.ones(2, 3, 8, 8),)] * 2
    engine.train(m, opt, data, 'cpu', 2, log=lambda *a: None, ignore_border=1)
    assert len(m.seen) == 2 and all(torch.equal(w, engine.border_weights(2, 8, 1)) for w in m.seen)
    m.seen = []
    engine.train(m, opt, data, 'cpu', 1, log=lambda *a: None)
    assert m.seen == [None]
