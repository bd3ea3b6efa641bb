"""Kernel-level tests of the one-product form of the weight-stationary decoder conv (conv3x3_ws_f16x3_kernel<.., NPROD = 1>, option
conv_precision 2) through iodine_op_conv3x3 mode 17: against the CPU emulation that defines it (tests/f16x1_reference.py: the operands
are rounded identically on both sides, so only the fp32 accumulation differs - the tolerance of test_conv_weight_stationary_f16x3),
against the exact fp64 conv within the a-priori bound of the rounding, the row-sum epilogues, determinism, and that it is not the split.

Shapes: (32, 16, 2) is the smallest the kernel takes (one tile row, both C = 32 pixel groups, every neighbourhood clamped); N = 5 and
N = 70 give blocks that cross images and a short last XCD share; S = 128 has interior tiles."""
import functools

import pytest
import torch
import torch.nn.functional as F

import f16x1_reference as R
from iodine_amd import _lib, synth
from oracle import iodine_oracle as O
from util import make_hip_model, nchw, nhwc, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(64, 32, 3), (32, 16, 2), (64, 16, 5), (32, 32, 70), (64, 128, 1)]


def _conv_op(mode, x_nhwc, w, bias, aux, n, s, c, epi, tflip, out_shape):
    L = _lib.lib()
    out = torch.full(out_shape, float('nan'), device=DEV)
    args = [t.to(DEV).contiguous() if t is not None else None for t in (x_nhwc, w, bias, aux)]
    rc = L.iodine_op_conv3x3(None, mode, _lib.ptr(args[0]), _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]),
                             _lib.ptr(out), n, s, s, c, c, c, c, 1, epi, tflip)
    _lib.check(rc, None, 'iodine_op_conv3x3')
    torch.cuda.synchronize()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _case(C_, S, N):
    """inputs, the emulation and the exact results of one shape (fp64, NHWC), and the device's mode-17 outputs: computed once, read-only"""
    x, w, b, g, a = R.kernel_inputs(C_, S, N)
    xd, wd, bd, gd = x.double(), w.double(), b.double(), g.double()
    eg = R.elu_grad_from_out(a).double()
    gin = torch.zeros_like(xd).requires_grad_(True)
    R.conv16(gin, wd).backward(gd)                              # the data gradient of conv16 at the gradient batch
    c = dict(x=x, w=w, b=b, g=g, a=a,
             fwd16=nhwc(F.elu(R.conv16(xd, wd, bd))), fwd_exact=nhwc(F.elu(F.conv2d(xd, wd, bd, padding=1))),
             fwd_bound=nhwc(R.REL_BOUND * R.abs_conv(xd, wd)),
             dg16=nhwc(gin.grad * eg), dg_exact=nhwc(F.conv_transpose2d(gd, wd, padding=1) * eg),
             dg_bound=nhwc(R.REL_BOUND * R.abs_conv(gd, wd, transpose=True) * eg))
    c['fwd'] = _conv_op(17, nhwc(x), w, b, None, N, S, C_, 0, 0, c['fwd16'].shape)
    c['dg'] = _conv_op(17, nhwc(g), w, None, nhwc(a), N, S, C_, 1, 1, c['dg16'].shape)
    return c


def _halves(N):
    return [h for h in (slice(0, N // 2), slice(N // 2, N)) if h.stop > h.start]       # (N = 1: the whole batch is the small half)


@pytest.mark.parametrize('C_,S,N', SHAPES)
def test_forward_and_data_gradient_match_the_emulation(C_, S, N):
    """fails without the feature (mode 17 is refused); proves that ONE product ran and how it was rounded: the split's result is 3e-4
    away from conv16, truncated activations 2e-4"""
    c = _case(C_, S, N)
    e = rel_err(c['fwd'], c['fwd16'])
    print(f'[{C_}, {S}, {N}] forward vs conv16 {e:.2e} (vs exact {rel_err(c["fwd"], c["fwd_exact"]):.2e})')
    assert e <= 3e-6, e
    for half in _halves(N):
        e = rel_err(c['dg'][half], c['dg16'][half])
        print(f'[{C_}, {S}, {N}] data gradient vs conv16 {e:.2e} (vs exact {rel_err(c["dg"][half], c["dg_exact"][half]):.2e})')
        assert e <= 3e-6, e


@pytest.mark.parametrize('C_,S,N', SHAPES)
def test_every_element_within_the_a_priori_bound(C_, S, N):
    """|got - exact| <= (2^-10 + 2^-22) (|w| (*) |x|) x ELU'-factor + 4e-6 max |exact| (the forward's ELU is 1-Lipschitz: factor 1)"""
    c = _case(C_, S, N)
    d = (c['fwd'].double() - c['fwd_exact']).abs()
    lim = c['fwd_bound'] + 4e-6 * c['fwd_exact'].abs().max()
    print(f'[{C_}, {S}, {N}] forward: worst error / bound {(d / lim).max():.3f}')
    assert (d <= lim).all()
    for half in _halves(N):
        d = (c['dg'][half].double() - c['dg_exact'][half]).abs()
        lim = c['dg_bound'][half] + 4e-6 * c['dg_exact'][half].abs().max()
        print(f'[{C_}, {S}, {N}] data gradient: worst error / bound {(d / lim).max():.3f}')
        assert (d <= lim).all()


@pytest.mark.parametrize('C_,S,N', SHAPES)
def test_row_sum_epilogues(C_, S, N):
    """EPI_L0ROWS / EPI_L0ROWSX against the left / interior / right / x-weighted sums of the mode-17 EPI_MUL_ELUGRAD output"""
    c = _case(C_, S, N)
    tiles = S // 16
    r = c['dg'].view(N, S, tiles, 16, C_).double()
    want = torch.zeros(N, S, tiles, 3, C_, dtype=torch.float64)
    want[:, :, :, 1] = r.sum(3)
    want[:, :, 0, 0] = r[:, :, 0, 0]; want[:, :, 0, 1] -= r[:, :, 0, 0]
    want[:, :, -1, 2] = r[:, :, -1, 15]; want[:, :, -1, 1] -= r[:, :, -1, 15]
    lin = torch.linspace(-1, 1, S).double().view(1, 1, tiles, 16, 1)
    want4 = torch.cat([want, (r * lin).sum(3, keepdim=True)], 3)
    rows = _conv_op(17, nhwc(c['g']), c['w'], None, nhwc(c['a']), N, S, C_, 4, 1, (N, S, tiles, 3, C_))
    rows4 = _conv_op(17, nhwc(c['g']), c['w'], None, nhwc(c['a']), N, S, C_, 5, 1, (N, S, tiles, 4, C_))
    for half in _halves(N):
        e3, e4 = rel_err(rows[half], want[half].float()), rel_err(rows4[half], want4[half].float())
        print(f'[{C_}, {S}, {N}] row sums {e3:.2e}, with the weighted sum {e4:.2e}')
        assert e3 <= 5e-6, e3
        assert e4 <= 5e-6, e4


@pytest.mark.parametrize('C_,S,N', SHAPES)
def test_deterministic_and_not_the_split_kernel(C_, S, N):
    c = _case(C_, S, N)
    assert torch.equal(c['fwd'], _conv_op(17, nhwc(c['x']), c['w'], c['b'], None, N, S, C_, 0, 0, c['fwd'].shape))
    assert torch.equal(c['dg'], _conv_op(17, nhwc(c['g']), c['w'], None, nhwc(c['a']), N, S, C_, 1, 1, c['dg'].shape))
    split = _conv_op(10, nhwc(c['x']), c['w'], c['b'], None, N, S, C_, 0, 0, c['fwd'].shape)
    assert not torch.equal(split, c['fwd'])
    assert rel_err(split, c['fwd_exact']) < 3e-6 < rel_err(c['fwd'], c['fwd_exact'])
    split_d = _conv_op(10, nhwc(c['g']), c['w'], None, nhwc(c['a']), N, S, C_, 1, 1, c['dg'].shape)
    assert not torch.equal(split_d, c['dg'])


@pytest.mark.parametrize('chan', [32, 64])
def test_side_buffer_of_a_forward_feeds_the_next_layer(chan):
    """No op-level path exposes ``tmax_out``, so a two-layer decode: with three decoder layers the second weight-stationary launch takes
    its tile scales from the side buffer the first one wrote.  Its output must be conv16 of the first one's output (as the device left
    it): the emulation derives the scales from that tensor itself, i.e. from what launch_cell_max would give.  The slot-images get
    latents of very different size, so that cells in different binades exist."""
    arch = O.tiny_arch(img_size=32, dec_layers=3, chan=chan)
    pn = synth.make_params(O.param_shapes(arch), seed=17, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    m = make_hip_model(arch, params, options={'conv_precision': 2})
    B, K, S = 2, arch.slots, arch.img_size
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, K, arch.dim_latent, generator=g) * torch.tensor([3.0, 0.3, 0.01]).view(1, K, 1)
    m.decode(z.to(DEV))
    act = [nchw(m.debug_buffer(f'act{l}').cpu().view(B * K, S, S, chan)).double() for l in range(3)]
    scales = R.cell_scales(act[1])
    assert scales.unique().numel() > 1                          # (more than one binade among the cells)
    for l in (1, 2):
        w, b = params[f'decoder.mlc.layers.{l}.weight'].double(), params[f'decoder.mlc.layers.{l}.bias'].double()
        want = F.elu(R.conv16(act[l - 1], w, b))
        e = rel_err(act[l], want)
        print(f'[chan {chan}] layer {l} vs conv16 of the device\'s layer {l - 1}: {e:.2e}')
        assert e <= 3e-6, (l, e)
