"""Auxiliary losses on the training forward's final state, CPU side: the C ABI of iodine_train_backward_aux and the gradient path the GPU tests'
float64 ground truth takes (tests/aux_reference.py)."""
import os
import re

import torch

from iodine_amd import _lib, synth
from oracle import iodine_oracle as O

import aux_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(header, name):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
    assert m, f'{name} is not declared in include/iodine_hip.h'
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_library_exports_the_aux_backward_and_the_header_declares_it():
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in ('iodine_train_backward_aux', 'iodine_op_render_bwd_logits'):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert _declaration(header, 'iodine_train_backward_aux') == [
        'iodine_handle* h', 'void* stream', 'const float* grad_loss_dev', 'const float* g_mean', 'const float* g_mask', 'const float* g_logits',
        'const float* g_z', 'const float* g_post_mean', 'const float* g_post_logvar', 'float* flat_grads', 'int accumulate']
    assert len(L.iodine_train_backward_aux.argtypes) == 11
    # the existing rendering backward keeps its signature; the new op-level entry is the same with g_logits behind g_mean
    old, new = _declaration(header, 'iodine_op_render_bwd'), _declaration(header, 'iodine_op_render_bwd_logits')
    assert new == old[:5] + ['const float* g_logits'] + old[5:]
    # documented like its neighbours, with the reference lines it stands for
    doc = header[:header.index('int iodine_train_backward_aux(')]
    doc = doc[doc.rindex('/*'):]
    assert 'iodine.py:137,171-187,642-651' in doc and 'IODINE_ERR_STATE' in doc and 'NULL' in doc


def test_oracle_aux_gradient_path():
    """What section 1 of the design claims, on the ground truth itself: an auxiliary term on the final evaluation's tensors reaches the
    decoder weights and, through delta_{T-1} and the T refinement iterations, the refinement network - and nothing reaches
    posterior.init_mean / init_logvar (lambda_T = detach(lambda_{T-1}) + delta_{T-1}, detached refinement inputs)."""
    arch = O.tiny_arch()                                                       # K = 3, T = 2, S = 16, L = 8
    pn = synth.make_params(O.param_shapes(arch), seed=41, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    x = torch.from_numpy(synth.make_images(2, arch.img_size, seed=42))
    eps = torch.from_numpy(synth.make_eps(arch.iters, 2, arch.slots, arch.dim_latent, seed=43))
    W = A.aux_weights(arch, 2, seed=44)
    g = A.oracle_grads(x, eps, params, arch, W)                                # aux alone
    for n in ('posterior.init_mean', 'posterior.init_logvar'):
        assert g[n] is None or not g[n].any(), n
    for n, v in g.items():
        if n.startswith(('refine.', 'decoder.')):
            assert v is not None and float(v.abs().max()) > 0, n
    # only lambda_T's cotangents: the decoder is not on the path, the refinement network is
    g = A.oracle_grads(x, eps, params, arch, {n: W[n] for n in ('post_mean', 'post_logvar')})
    assert all(g[n] is None or not g[n].any() for n in g if n.startswith(('decoder.', 'posterior.')))
    assert all(float(g[n].abs().max()) > 0 for n in g if n.startswith('refine.'))
    # the restated forward is the oracle's: same loss, same attached tensors
    _, loss, ts = A.oracle_forward(x, eps, params, arch)
    ref = O.train_forward(x.double(), eps.double(), {k: v.double() for k, v in params.items()}, arch)
    assert torch.equal(loss, ref['loss']) and torch.equal(ts['mask'], ref['final_mask']) and torch.equal(ts['post_mean'], ref['post_mean'])
