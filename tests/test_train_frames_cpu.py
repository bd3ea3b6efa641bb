"""Per-frame auxiliary losses, CPU side: the C ABI of the two new entry points and the mathematics the GPU tests rely on (the float64
reference of tests/frames_reference.py): it is the aux reference on the final evaluation, the detach points give the structural zeros
the library's gradient path is built on, and float32 arithmetic on the test inputs sits far below the GPU gate."""
import os
import re

import pytest
import torch

from iodine_amd import _lib, synth
from oracle import iodine_oracle as O
from util import rel_l2

import aux_reference as A
import frames_reference as F
from clip_reference import moving_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2
BASE = O.tiny_arch()
WS = O.tiny_arch(slots=3, iters=3, img_size=32, chan=64)


def _inputs(arch, seed=50, clip=True):
    """built like tests/test_gpu_train_aux.py::_inputs"""
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    x = torch.from_numpy(synth.make_images(B, arch.img_size, seed=seed + 1))
    if clip:
        x = moving_clip(x, arch.iters + 1)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=seed + 2))
    return params, x, eps


def _declaration(header, name):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    assert '#define IODINE_ABI_VERSION 3' in header
    for name in ('iodine_train_forward_frames', 'iodine_train_backward_frames'):
        assert name in _lib.EXPORTS
    seq_f, seq_b = _declaration(header, 'iodine_train_forward_seq'), _declaration(header, 'iodine_train_backward_seq')
    assert _declaration(header, 'iodine_train_forward_frames') == seq_f + ['const int* frame_idx', 'int n_frames', 'float* const* frames_out']
    assert _declaration(header, 'iodine_train_backward_frames') == seq_b + ['const int* frame_idx', 'int n_frames',
                                                                            'const float* const* g_frames']
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.iodine_abi_version() == 3
        assert len(L.iodine_train_forward_frames.argtypes) == 11 and len(L.iodine_train_backward_frames.argtypes) == 17


@pytest.mark.parametrize('clip', [False, True], ids=['image', 'clip'])
def test_final_frame_alone_is_the_aux_reference(clip):
    params, x, eps = _inputs(BASE, clip=clip)
    T = BASE.iters
    Wa = A.aux_weights(BASE, B, seed=60)
    ref = A.oracle_grads(x, eps, params, BASE, Wa, 1.0)
    got, _, _ = F.grads(x, eps, params, BASE, {(T, n): w for n, w in Wa.items()}, 1.0)
    for n in ref:
        e = rel_l2(got[n].numpy(), ref[n].numpy())
        assert e <= 1e-12, (n, e)


@pytest.mark.parametrize('arch', [BASE, WS], ids=['base', 'ws'])
def test_structural_facts_of_the_detach_points(arch):
    params, x, eps = _inputs(arch)
    W0 = F.weights(arch, B, 61, [0])
    g0, _, _ = F.grads(x, eps, params, arch, W0)
    for n, g in g0.items():
        if n.startswith('refine.'):                                          # frame 0 alone: nothing reaches the refinement network
            assert g is None or not g.any(), n
        else:                                                                # ... the decoder and the initial posterior receive it
            assert g is not None and g.any(), n
    g1, _, _ = F.grads(x, eps, params, arch, {(1, 'mask'): F.weights(arch, B, 61, [1])[(1, 'mask')]})
    for n, g in g1.items():                                                  # a mask cotangent on frame 1: through delta_0 to everything
        if n == 'refine.lstm.weight_hh' or n.startswith('posterior.'):       # but weight_hh (h_0 = 0) and the initial posterior
            assert g is None or not g.any(), n
        else:
            assert g is not None and g.any(), n


@pytest.mark.parametrize('arch', [BASE, WS], ids=['base', 'ws'])
def test_float32_oracle_is_far_below_the_gpu_gate(arch):
    params, x, eps = _inputs(arch)
    W = F.weights(arch, B, 60, range(arch.iters + 1))
    g64, _, _ = F.grads(x, eps, params, arch, W)
    g32, _, _ = F.grads(x, eps, params, arch, W, dtype=torch.float32)
    errs = {n: rel_l2(g32[n].numpy(), g64[n].numpy()) for n in g64}
    print(max((e, n) for n, e in errs.items()))
    assert all(e < 1e-4 for e in errs.values()), errs
