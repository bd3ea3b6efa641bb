"""Option conv_precision 2 without a GPU: the CPU emulation that defines the mode (tests/f16x1_reference.py) - its rounding procedures,
the a-priori error bound of one conv, what the mode costs on the ``tiny`` golden, that the oracle is left as it was - and the engine's
command line."""
import pytest
import torch
import torch.nn.functional as F

import f16x1_reference as R
from oracle import iodine_oracle as O
from util import golden_setup, load_golden, rel_err


def _signed_magnitudes(*shape, seed, lo=0.5):
    """random signs, magnitudes in [lo, 1): no element is small against the maximum of its group (a uniform draw has elements arbitrarily
    close to zero, which fp16 at the GROUP's scale cannot hold to 2^-11 of their own size)"""
    g = torch.Generator().manual_seed(seed)
    m = lo + (1 - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)
    return torch.where(torch.rand(*shape, generator=g) < 0.5, -m, m)


def test_rounding_is_idempotent():
    x = R._rand(2, 32, 16, 32, seed=1).double()
    w = R._rand(32, 32, 3, 3, seed=2, scale=0.3).double()
    rx, rw = R.round_cells(x), R.round_weights(w)
    assert not torch.equal(rx, x) and not torch.equal(rw, w)
    assert torch.equal(R.round_cells(rx), rx) and torch.equal(R.round_weights(rw), rw)


def test_representable_values_are_unchanged():
    """multiples of 2^-10 up to 1.5: 11 significant bits whatever the power-of-two scale"""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-1536, 1537, (2, 32, 16, 16), generator=g).double() / 1024
    x[0, 0, 0, 0] = 1.5                                       # a cell maximum that is no power of two
    assert torch.equal(R.round_cells(x), x)
    w = torch.randint(-1536, 1537, (32, 32, 3, 3), generator=g).double() / 4096
    assert torch.equal(R.round_weights(w), w)


def test_all_zero_cell_and_tensor():
    x = R._rand(1, 32, 32, 64, seed=4).double()
    x[:, :, :, 32:] = 0                                       # cells (., 2) and (., 3) are zero; (., 3) has an all-zero neighbourhood
    r = R.round_cells(x)
    assert torch.isfinite(r).all() and torch.equal(r[:, :, :, 32:], x[:, :, :, 32:])
    assert rel_err(r[:, :, :, :32], x[:, :, :, :32]) < 2.0 ** -11
    z = torch.zeros(1, 32, 16, 16, dtype=torch.float64)
    assert torch.equal(R.round_cells(z), z) and torch.equal(R.round_weights(torch.zeros(32, 32, 3, 3)), torch.zeros(32, 32, 3, 3))
    assert (R.cell_scales(z) == 1).all()


def test_ranges_four_decades_apart():
    """cells get their own scale: a batch whose halves differ by 1e4 is rounded to 2^-11 of every ELEMENT in both halves; a weight tensor
    has ONE scale: its small half sits at 2^12 / 1e4 ~ 0.4 in fp16 - still normal numbers (>= 2^-14), so the same holds"""
    x = _signed_magnitudes(4, 32, 16, 16, seed=5)
    x[2:] *= 1e-4
    r = R.round_cells(x)
    assert torch.isfinite(r).all() and (r != 0).all()
    assert ((r - x).abs() / x.abs()).max() <= 2.0 ** -11
    s = R.cell_scales(x)
    assert (s[2:] > s[:2] * 4096).all()                       # (the small half is not rounded at the large half's scale)
    w = _signed_magnitudes(32, 32, 3, 3, seed=6) * 0.3
    w[16:] *= 1e-4
    rw = R.round_weights(w)
    assert torch.isfinite(rw).all() and (rw != 0).all()
    assert ((rw - w).abs() / w.abs()).max() <= 2.0 ** -11
    big = R._rand(1, 32, 16, 16, seed=7).double() * 6e4       # beyond the fp16 range unscaled
    assert rel_err(R.round_cells(big), big) < 2.0 ** -11


@pytest.mark.parametrize('C_,S,N', [(64, 32, 3), (32, 16, 2), (64, 16, 5)])
def test_conv16_within_the_a_priori_bound(C_, S, N):
    x, w, b, g, a = (t.double() for t in R.kernel_inputs(C_, S, N))
    exact = F.conv2d(x, w, b, padding=1)
    got = R.conv16(x, w, b)
    assert ((got - exact).abs() <= R.REL_BOUND * R.abs_conv(x, w)).all()
    assert 1e-5 < rel_err(got, exact) < 2e-3                  # ... and it IS rounded
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    R.conv16(xr, wr, b).backward(g)
    exact_d = F.conv_transpose2d(g, w, padding=1)
    assert ((xr.grad - exact_d).abs() <= R.REL_BOUND * R.abs_conv(g, w, transpose=True)).all()
    for half in (slice(0, N // 2), slice(N // 2, N)):
        assert 1e-5 < rel_err(xr.grad[half], exact_d[half]) < 2e-3
    # the weight gradient is the one of the unrounded operands
    xe, we = x.clone(), w.clone().requires_grad_(True)
    F.conv2d(xe, we, b, padding=1).backward(g)
    assert rel_err(wr.grad, we.grad) < 1e-12


def test_emulated_reconstruct_on_tiny_and_the_oracle_is_restored():
    g = load_golden('tiny')
    arch, params, x, eps, _ = golden_setup(g, torch.float64)
    before = O.reconstruct(x, eps, params, arch)
    stack = O.conv_stack
    emu = R.emulated(O.reconstruct)(x, eps, params, arch)
    assert O.conv_stack is stack                              # the patch is gone ...
    after = O.reconstruct(x, eps, params, arch)
    for k in before:
        assert torch.equal(before[k], after[k]), k            # ... and a plain call is what it was, bitwise
    dev = ((emu['elbos'] - before['elbos']).abs() / before['elbos'].abs()).max().item()
    print(f'tiny: ELBO deviation of the emulation, worst evaluation: {dev:.2e}; pred max abs {(emu["pred"] - before["pred"]).abs().max():.2e}')
    assert 0 < dev < 1e-3
    agree = (emu['mask'][:, :, 0].argmax(1) == before['mask'][:, :, 0].argmax(1)).double().mean().item()
    assert agree >= 0.999


def test_emulation_restores_the_oracle_after_an_exception():
    stack = O.conv_stack
    with pytest.raises(ZeroDivisionError):
        R.emulated(lambda: 1 / 0)()
    assert O.conv_stack is stack


def test_emulation_leaves_uncovered_decoders_alone():
    """img_size 48 (no power of two) runs on the LDS-tiled kernel, which conv_precision 2 does not change"""
    arch = O.tiny_arch(img_size=48)
    from iodine_amd import synth
    p = {k: torch.from_numpy(v).double() for k, v in synth.make_params(O.param_shapes(arch), seed=3, dec_gain=3.0, posterior_scale=0.05).items()}
    z = R._rand(1, arch.slots, arch.dim_latent, seed=8).double()
    a, b = O.decoder(z, p, arch), R.emulated(O.decoder)(z, p, arch)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    arch = O.tiny_arch()
    p = {k: torch.from_numpy(v).double() for k, v in synth.make_params(O.param_shapes(arch), seed=3, dec_gain=3.0, posterior_scale=0.05).items()}
    a, b = O.decoder(z, p, arch), R.emulated(O.decoder)(z, p, arch)
    assert not torch.equal(a[0], b[0])


def test_engine_parser_takes_conv_precision():
    from iodine_amd.engine import make_parser
    ap = make_parser()
    assert ap.parse_args([]).conv_precision == 1
    assert ap.parse_args(['--conv-precision', '2']).conv_precision == 2
    assert ap.parse_args(['--conv-precision', '2', '--resume', 'x.pt', '--eval-samples', '4']).conv_precision == 2
    with pytest.raises(SystemExit):
        ap.parse_args(['--conv-precision', '3'])
