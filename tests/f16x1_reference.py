"""CPU emulation of option conv_precision 2: what the one-product form of the weight-stationary decoder kernel
(conv3x3_ws_f16x3_kernel<.., NPROD = 1>, kernels_convws.hip) computes, in the style of the other *_reference.py files.

The mode is conv_precision 1 except in that kernel, where a product is ONE fp16 MFMA of the two operands' rounded values:

  * activations (and, in the data gradient, incoming gradients): per 8 x 16 cell the maximum |x| over all channels, the maximum of that
    over the 3 x 3 cell neighbourhood (clamped at the borders) - the kernel's ``tmax`` side buffer -, the power of two that brings it into
    [2^12, 2^13) (``fresh_scale``), fp16 to nearest even at that scale: ``round_cells``;
  * weights: the power of two of ``weight_scale_block`` per tensor (max |w| into [2^12, 2^13)), fp16 to nearest even: ``round_weights``
    (the hi half of the existing pack);
  * accumulation, bias, ELU / ELU', row sums: as before (fp32 on the device, the caller's dtype here);
  * the weight and bias gradients are the library's unchanged split kernels: they see the UNROUNDED operands.

``conv16`` is that conv with its gradients, ``emulated(fn)`` runs an ``oracle.iodine_oracle`` entry with it in the decoder layers the
kernel covers.  Everything is computed in the dtype of the inputs (fp64 for the oracle): only the operand rounding is modelled, the device's
fp32 accumulation is not.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import iodine_oracle as O

CELL_H, CELL_W = 8, 16


def _pow2_scale(m):
    """power of two s with m * s in [2^12, 2^13); 1 where m is zero or not finite (fresh_scale / weight_scale_block)"""
    _, e = torch.frexp(m)                                    # m = f * 2^e, f in [0.5, 1)
    s = torch.ldexp(torch.ones_like(m), 13 - e)
    return torch.where((m > 0) & torch.isfinite(m), s, torch.ones_like(m))


def _to_f16_and_back(v):
    return v.half().to(v.dtype)                              # round to nearest even


def cell_scales(x):
    """(N, H, W) scale of every pixel of an NCHW tensor: one power of two per 8 x 16 cell, from the 3 x 3 neighbourhood maximum"""
    N, C, H, W = x.shape
    assert H % CELL_H == 0 and W % CELL_W == 0, 'whole cells only'
    m = x.detach().abs().amax(1)                                                         # over channels
    m = m.reshape(N, H // CELL_H, CELL_H, W // CELL_W, CELL_W).amax((2, 4))              # per cell
    m = F.max_pool2d(m[:, None], 3, stride=1, padding=1)[:, 0]                           # neighbourhood; the -inf padding = clamping
    return _pow2_scale(m).repeat_interleave(CELL_H, 1).repeat_interleave(CELL_W, 2)


def round_cells(x):
    """an NCHW tensor as the kernel's MFMA sees it: fp16 to nearest even at the cell scale, scale divided out again"""
    s = cell_scales(x)[:, None]
    return _to_f16_and_back(x * s) / s


def round_weights(w):
    s = _pow2_scale(w.detach().abs().amax())
    return _to_f16_and_back(w * s) / s


class _Conv16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.conv2d(round_cells(x), round_weights(w), b, padding=1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = F.conv_transpose2d(round_cells(g), round_weights(w), padding=1)
        if ctx.needs_input_grad[1]:
            gw = torch.nn.grad.conv2d_weight(x, w.shape, g, padding=1)                   # unrounded operands: the library's own kernels
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum((0, 2, 3))
        return gx, gw, gb


def conv16(x, w, b=None):
    """3 x 3 conv, padding 1, of the one-product kernel: forward and data gradient on rounded operands, weight / bias gradient exact"""
    return _Conv16.apply(x, w, b)


def covered(channels, kernel, stride, size):
    """does the weight-stationary kernel run this decoder layer?  (3 x 3, stride 1, 32 / 64 channels, power-of-two image size >= 16)"""
    return kernel == 3 and stride == 1 and channels in (32, 64) and size >= 16 and size & (size - 1) == 0


def _conv_stack16(orig, x, p, prefix, n_layers, kernel, stride, keep=None):
    w1 = p.get(f'{prefix}.layers.1.weight') if n_layers > 1 else None
    if prefix != 'decoder.mlc' or w1 is None or x.shape[-1] != x.shape[-2] or not covered(w1.shape[0], kernel, stride, x.shape[-1]):
        return orig(x, p, prefix, n_layers, kernel, stride, keep)
    for i in range(n_layers):
        w, b = p[f'{prefix}.layers.{i}.weight'], p[f'{prefix}.layers.{i}.bias']
        x = F.conv2d(x, w, b, stride=stride, padding=kernel // 2) if i == 0 else conv16(x, w, b)     # layer 0: the broadcast layer's kernel
        x = F.elu(x)
        if keep is not None:
            keep.append(x)
    return x


def emulated(fn):
    """``fn`` (O.reconstruct, O.train_step_grads, O.decoder, ...) running with conv16 in decoder layers 1 .. dec_layers - 1: the module's
    conv_stack is replaced for the duration of the call and restored afterwards"""
    @functools.wraps(fn)
    def run(*args, **kwargs):
        orig = O.conv_stack
        O.conv_stack = functools.partial(_conv_stack16, orig)
        try:
            return fn(*args, **kwargs)
        finally:
            O.conv_stack = orig
    return run


def abs_conv(x, w, transpose=False):
    """|w| (*) |x|: the per-element scale of the a-priori error bound"""
    f = F.conv_transpose2d if transpose else F.conv2d
    return f(x.abs(), w.abs(), padding=1)


# A-priori bound of one product: each operand is rounded to 11 significant bits (relative error <= 2^-11 per element while the scaled
# value stays a normal fp16, i.e. within 2^-26 of its cell's / tensor's maximum), so |w~ x~ - w x| <= (2 * 2^-11 + 2^-22) |w| |x|.
REL_BOUND = 2.0 ** -10 + 2.0 ** -22


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def kernel_inputs(C, S, N):
    """the inputs of test_conv_weight_stationary_f16x3 (test_gpu_ops.py): x, w, bias, gradient (its batch halves 1e-4 apart), ELU output"""
    x = _rand(N, C, S, S, seed=21)
    w = _rand(C, C, 3, 3, seed=22, scale=3.0 / (C * 9) ** 0.5)
    b = _rand(C, seed=23, scale=0.5)
    g = _rand(N, C, S, S, seed=24, scale=1e-3)
    g[N // 2:] *= 1e-4
    a = F.elu(_rand(N, C, S, S, seed=25, scale=2.0))
    return x, w, b, g, a


def elu_grad_from_out(a):
    return torch.where(a > 0, torch.ones_like(a), a + 1)
