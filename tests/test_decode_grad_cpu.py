"""CPU-side checks of the differentiable decode(z) / elbo(x) surface: exported symbols, header, ABI version, and the
rendering-backward formulas that kernels_render.hip restates, against fp64 autograd."""
import os
import re

import torch
import torch.nn.functional as F

from iodine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('iodine_decode_backward', 'iodine_elbo_backward', 'iodine_op_render_bwd')


def test_new_symbols_are_exported_and_declared_and_the_abi_version_stays():
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
    assert L.iodine_abi_version() == 3
    assert '#define IODINE_ABI_VERSION 3' in header
    assert '"save_for_backward"' in header and '"render_bwd"' in header
    # (iodine_workspace_bytes needs a handle, and iodine_create allocates on a device: the mode ordering 0 <= 2 <= 1 is asserted in
    # tests/test_gpu_decode_grad.py)


def test_module_signatures_take_the_differentiable_argument():
    import inspect
    from iodine_amd import IODINE
    assert list(inspect.signature(IODINE.decode).parameters) == ['self', 'z', 'differentiable']
    assert list(inspect.signature(IODINE.elbo).parameters) == ['self', 'x', 'eps', 'differentiable']
    assert inspect.signature(IODINE.decode).parameters['differentiable'].default is None
    assert inspect.signature(IODINE.elbo).parameters['differentiable'].default is None


def render_bwd_formulas(o, g_pred, g_mask, g_mean):
    """The closed forms of kernels_render.hip.  o (B,K,4,P) = decoder output (rgb logits, mask logit); gradients NCHW-shaped with the
    pixels flattened: g_pred (B,3,P), g_mask (B,K,1,P), g_mean (B,K,3,P); None = zero.  Returns d / d o, (B,K,4,P)."""
    mu = torch.sigmoid(o[:, :, :3])
    m = F.softmax(o[:, :, 3:], dim=1)
    gp = torch.zeros_like(mu[:, 0]) if g_pred is None else g_pred
    dmu = gp[:, None] * m + (0 if g_mean is None else g_mean)
    do = dmu * mu * (1 - mu)
    dm = (gp[:, None] * mu).sum(2, keepdim=True) + (0 if g_mask is None else g_mask)
    dlogit = m * (dm - (m * dm).sum(1, keepdim=True))
    return torch.cat((do, dlogit), 2)


def render_bwd_autograd(o, g_pred, g_mask, g_mean):
    o = o.detach().clone().requires_grad_(True)
    mean = torch.sigmoid(o[:, :, :3])
    mask = F.softmax(o[:, :, 3:], dim=1)
    pred = (mask * mean).sum(1)
    loss = sum((g * t).sum() for g, t in ((g_pred, pred), (g_mask, mask), (g_mean, mean)) if g is not None)
    return torch.autograd.grad(loss, o)[0]


def test_render_backward_formulas_equal_fp64_autograd():
    gen = torch.Generator().manual_seed(5)
    for K in (1, 2, 7, 16):
        B, P = 2, 37
        o = torch.randn(B, K, 4, P, generator=gen, dtype=torch.float64) * 3
        o[:, :, 3] *= 10                                   # logits spread to +-30: some masks saturate
        gs = (torch.randn(B, 3, P, generator=gen, dtype=torch.float64), torch.randn(B, K, 1, P, generator=gen, dtype=torch.float64),
              torch.randn(B, K, 3, P, generator=gen, dtype=torch.float64))
        for use in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            sel = tuple(g if u else None for g, u in zip(gs, use))
            got, ref = render_bwd_formulas(o, *sel), render_bwd_autograd(o, *sel)
            assert (got - ref).abs().max() <= 1e-12 * max(1.0, ref.abs().max().item()), (K, use)
            if K == 1:
                assert torch.all(ref[:, :, 3].abs() < 1e-15)
