"""Option gen_conv_precision 1: the split-fp16 (3 x v_mfma_f32_16x16x32_f16) forward / data-gradient and weight-gradient kernels of the
generic decoder's C -> C layers (kernels_gensplit.hip) - operator level against ATen in fp64, range / outlier behaviour, determinism, the
shapes it refuses, end to end against the reference's fixtures and the oracle, and the semantics of the option."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iodine_amd import _lib, synth
from oracle import iodine_oracle as O
from util import golden_setup, grad_views, load_golden, make_hip_model, nhwc, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SHAPES = [(5, 64, 128, 2), (5, 32, 64, 3), (5, 48, 72, 1), (7, 32, 64, 2), (3, 16, 24, 5), (5, 64, 16, 40), (7, 16, 20, 2), (3, 64, 8, 3)]   # k, C, S, N


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _op_rc(mode, x, w, bias, aux, out, n, si, c, k, elu, ci=None, ldc=None, s=1, gb=None):
    L = _lib.lib()
    t = [v.to(DEV).contiguous() if v is not None else None for v in (x, w, bias, aux)]
    rc = L.iodine_op_gen_conv_f16x3(None, mode, _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), _lib.ptr(out), _lib.ptr(gb),
                                    n, si, c if ci is None else ci, c if ldc is None else ldc, c, k, s, elu)
    torch.cuda.synchronize()
    return rc


def _op(mode, x, w, bias, aux, shape, n, si, c, k, elu):
    out = torch.full(shape, float('nan'), device=DEV)
    assert _op_rc(mode, x, w, bias, aux, out, n, si, c, k, elu) == 0, _lib.lib().iodine_last_error(None)
    return out.cpu()


def _elu_grad(a):
    return torch.where(a > 0, torch.ones_like(a), a + 1)


@pytest.mark.parametrize('elu', [1, 0], ids=['elu', 'linear'])
@pytest.mark.parametrize('k,C_,S,N', SHAPES)
def test_split_forward_against_fp64(k, C_, S, N, elu):
    x = _rand(N, C_, S, S, seed=1)
    w = _rand(C_, C_, k, k, seed=2, scale=3.0 / (C_ * k * k) ** 0.5)
    b = _rand(C_, seed=3, scale=0.5)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=k // 2)
    ref = nhwc(F.elu(ref) if elu else ref)
    got = _op(0, nhwc(x), w, b, None, ref.shape, N, S, C_, k, elu)
    e = rel_err(got, ref)
    print(f'[gen split fwd] k{k} C{C_} S{S} N{N} elu{elu}: rel err {e:.2e}')
    assert e < 3e-6


@pytest.mark.parametrize('gscale', [1e-3, 1e-2])
@pytest.mark.parametrize('k,C_,S,N', SHAPES)
def test_split_dgrad_times_elu_grad_against_fp64(k, C_, S, N, gscale):
    """gradients at the scales of tests/test_gpu_ops.py, half the batch 1e-4 smaller in the same launch (one scale per tile and chunk:
    the small images must keep their own accuracy)"""
    g = _rand(N, C_, S, S, seed=4, scale=gscale)
    g[N // 2:] *= 1e-4
    w = _rand(C_, C_, k, k, seed=5, scale=3.0 / (C_ * k * k) ** 0.5)
    a = F.elu(_rand(N, C_, S, S, seed=6, scale=2.0))
    ref = nhwc(F.conv_transpose2d(g.double(), w.double(), padding=k // 2) * _elu_grad(a).double())
    got = _op(1, nhwc(g), w, None, nhwc(a), ref.shape, N, S, C_, k, 0)
    e_all = rel_err(got, ref)
    e_small = rel_err(got[N // 2:], ref[N // 2:]) if N > 1 else 0.0
    print(f'[gen split dgrad] k{k} C{C_} S{S} N{N} scale {gscale:g}: rel err {e_all:.2e}, small half {e_small:.2e}')
    assert e_all < 3e-6 and e_small < 3e-6


def _wgrad(x_nchw, g_nchw, C_, k):
    N, S = x_nchw.shape[0], x_nchw.shape[2]
    gw, gb = torch.zeros(C_, C_, k, k, device=DEV), torch.zeros(C_, device=DEV)
    assert _op_rc(2, nhwc(x_nchw), None, None, nhwc(g_nchw), gw, N, S, C_, k, 0, gb=gb) == 0, _lib.lib().iodine_last_error(None)
    return gw.cpu(), gb.cpu()


@pytest.mark.parametrize('gscale', [1e-3, 1e-2])
@pytest.mark.parametrize('k,C_,S,N', SHAPES)
def test_split_weight_and_bias_gradient_against_fp64(k, C_, S, N, gscale):
    """weight + bias gradient (K = pixels) against autograd in fp64; activations are ELU outputs, gradients at the scales of
    tests/test_gpu_ops.py with half the batch 1e-4 smaller in the same launch"""
    a = F.elu(_rand(N, C_, S, S, seed=11, scale=2.0))
    g = _rand(N, C_, S, S, seed=12, scale=gscale)
    g[N // 2:] *= 1e-4
    w = torch.zeros(C_, C_, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(C_, dtype=torch.float64, requires_grad=True)
    F.conv2d(a.double(), w, b, padding=k // 2).backward(g.double())
    gw, gb = _wgrad(a, g, C_, k)
    ew, eb = rel_err(gw, w.grad), rel_err(gb, b.grad)
    print(f'[gen split wgrad] k{k} C{C_} S{S} N{N} scale {gscale:g}: weight {ew:.2e}, bias {eb:.2e}')
    assert ew < 3e-6 and eb < 3e-6
    if N > 1:                                                             # the small half alone: its own scales, its own accuracy
        w2 = torch.zeros(C_, C_, k, k, dtype=torch.float64, requires_grad=True)
        b2 = torch.zeros(C_, dtype=torch.float64, requires_grad=True)
        F.conv2d(a[N // 2:].double(), w2, b2, padding=k // 2).backward(g[N // 2:].double())
        gw2, gb2 = _wgrad(a[N // 2:], g[N // 2:], C_, k)
        assert rel_err(gw2, w2.grad) < 3e-6 and rel_err(gb2, b2.grad) < 3e-6


def test_split_weight_gradient_accumulates_into_its_outputs():
    k, C_, S, N = 5, 32, 24, 2
    a, g = _rand(N, C_, S, S, seed=13), _rand(N, C_, S, S, seed=14, scale=1e-2)
    gw, gb = _wgrad(a, g, C_, k)
    gw2, gb2 = (3.0 * torch.ones(C_, C_, k, k, device=DEV)), (2.0 * torch.ones(C_, device=DEV))
    assert _op_rc(2, nhwc(a), None, None, nhwc(g), gw2, N, S, C_, k, 0, gb=gb2) == 0
    assert rel_err(gw2.cpu() - 3.0, gw) < 1e-6 and rel_err(gb2.cpu() - 2.0, gb) < 1e-6


def test_split_extreme_ranges():
    """the construction of test_split_fp16_extreme_ranges at k = 5: gradient inputs down to 1e-8, weights up to 1e2"""
    k, C_, S, N = 5, 64, 32, 2
    a = F.elu(_rand(N, C_, S, S, seed=65, scale=2.0))
    for gs, ws in ((1e-8, 1.0), (1e-3, 1e2), (1e-8, 1e2), (1e4, 1e-4)):
        g = _rand(N, C_, S, S, seed=64, scale=gs)
        w = _rand(C_, C_, k, k, seed=62, scale=ws * 3.0 / (C_ * k * k) ** 0.5)
        ref = nhwc((F.conv_transpose2d(g.double(), w.double(), padding=k // 2) * _elu_grad(a).double()).float())
        got = _op(1, nhwc(g), w, None, nhwc(a), ref.shape, N, S, C_, k, 0)
        e = rel_err(got, ref)
        print(f'[gen split ranges] gradient scale {gs:g}, weight scale {ws:g}: rel err {e:.2e}')
        assert e < 3e-6, (gs, ws, e)


def _tile_outliers(t_nchw, factor, seed):
    """one element per 16 x 16 tile (and slot-image) multiplied up to `factor` x the tensor's RMS"""
    t = t_nchw.clone()
    N, C_, S, _ = t.shape
    rms = float(t.pow(2).mean().sqrt())
    g = torch.Generator().manual_seed(seed)
    hit = torch.zeros(N, S, S, dtype=torch.bool)
    for n in range(N):
        for cy in range(S // 16):
            for cx in range(S // 16):
                y, x, c = (int(torch.randint(0, m, (1,), generator=g)) for m in (16, 16, C_))
                t[n, c, cy * 16 + y, cx * 16 + x] = factor * rms
                hit[n, cy * 16 + y, cx * 16 + x] = True
    return t, hit


def test_split_outlier_in_every_tile():
    """the construction of test_split_fp16_outlier_in_every_cell at k = 5 with the gates of that test.  The scale granularity of this kernel
    is one staged 16 x 16-tile halo (20 x 20 pixels) x one channel chunk - coarser than the 8 x 16 cells of the tuned kernels - so the
    outliers are placed once per 16 x 16 TILE instead of once per cell, and the error unit of gate (1) is the largest output of the
    16 x 16 tile itself.  Gate (3) is the documented small-element bound that test_split_fp16_outlier_in_every_cell asserts."""
    k, C_, S, N = 5, 64, 32, 3
    w = _rand(C_, C_, k, k, seed=52, scale=3.0 / (C_ * k * k) ** 0.5)
    b = _rand(C_, seed=53, scale=0.5)
    for kind, factor in (('activation', 2.0 ** 24), ('activation', 2.0 ** 12), ('gradient', 2.0 ** 24)):
        if kind == 'activation':
            x, hit = _tile_outliers(_rand(N, C_, S, S, seed=51), factor, seed=60)
            ref = nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=k // 2))          # pre-activation: ELU would hide the error
            got = _op(0, nhwc(x), w, b, None, ref.shape, N, S, C_, k, 0).double()
        else:
            g, hit = _tile_outliers(_rand(N, C_, S, S, seed=54, scale=1e-3), factor, seed=61)
            a = F.elu(_rand(N, C_, S, S, seed=55, scale=2.0))
            ref = nhwc(F.conv_transpose2d(g.double(), w.double(), padding=k // 2) * _elu_grad(a).double())
            got = _op(1, nhwc(g), w, None, nhwc(a), ref.shape, N, S, C_, k, 0).double()
        reach = F.max_pool2d(hit[:, None].float(), k, stride=1, padding=k // 2)[:, 0] > 0   # outputs inside an outlier's k x k footprint
        err = (got - ref).abs()
        tilemax = F.max_pool2d(ref.abs().amax(-1)[:, None], kernel_size=16, stride=16)
        tilemax = tilemax.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, 0]
        e_tile = float((err.amax(-1) / tilemax).max())
        dom = reach[..., None].expand_as(ref) & (ref.abs() > 1e-3 * ref.abs().amax())
        e_dom = float((err[dom] / ref.abs()[dom]).max())
        far = ~reach
        e_small = float(err[far].max()) / float(ref[far].abs().median())
        print(f'[gen split outliers] {kind} x{factor:.0e}: err / tile max {e_tile:.1e}, rel err where the outlier dominates {e_dom:.1e}, '
              f'err of untouched outputs / their median magnitude {e_small:.1e}')
        assert e_tile < 1e-4, (kind, factor, e_tile)
        assert e_dom < 2e-5, (kind, factor, e_dom)
        assert e_small < 4e-3 if factor > 2.0 ** 20 else e_small < 2e-5, (kind, factor, e_small)


@pytest.mark.parametrize('k,C_,why', [(7, 64, 'slice does not fit the LDS'), (5, 20, 'not a multiple of 16'), (5, 8, 'fewer than 16 channels'),
                                      (5, 128, 'slice does not fit the LDS')])
def test_split_operator_refuses_uncovered_shapes(k, C_, why):
    S, N = 16, 1
    x, w = _rand(N, S, S, C_, seed=1), _rand(C_, C_, k, k, seed=2)
    out = torch.zeros(N, S, S, C_, device=DEV)
    for mode in (0, 1, 2):
        assert _op_rc(mode, x, w, None, x if mode else None, out, N, S, C_, k, 0, gb=out) == 1, why       # IODINE_ERR_INVALID
    assert float(out.abs().sum()) == 0.0


def test_split_operator_refuses_stride_2_and_rectangular_convs():
    S, N, C_, k = 16, 1, 32, 5
    x, w = _rand(N, S, S, C_, seed=1), _rand(C_, C_, k, k, seed=2)
    out = torch.zeros(N, S, S, C_, device=DEV)
    assert _op_rc(0, x, w, None, None, out, N, S, C_, k, 0, s=2) == 1
    assert _op_rc(0, x, w, None, None, out, N, S, C_, k, 0, ci=16, ldc=16) == 1
    assert _op_rc(0, x, w, None, None, out, N, S, C_, k, 0, ldc=36) == 1
    assert _op_rc(2, x, w, None, x, out, N, S, C_, k, 0, s=2, gb=out) == 1
    assert _op_rc(3, x, w, None, None, out, N, S, C_, k, 0) == 1
    assert float(out.abs().sum()) == 0.0


@pytest.mark.parametrize('k,C_,S,N', [(5, 64, 48, 3), (7, 32, 40, 2), (3, 48, 24, 2)])
def test_split_is_deterministic(k, C_, S, N):
    x = _rand(N, C_, S, S, seed=7)
    w = _rand(C_, C_, k, k, seed=8, scale=3.0 / (C_ * k * k) ** 0.5)
    b = _rand(C_, seed=9)
    a = F.elu(_rand(N, C_, S, S, seed=10, scale=2.0))
    shape = (N, S, S, C_)
    f1, f2 = (_op(0, nhwc(x), w, b, None, shape, N, S, C_, k, 1) for _ in range(2))
    d1, d2 = (_op(1, nhwc(x), w, None, nhwc(a), shape, N, S, C_, k, 0) for _ in range(2))
    assert torch.equal(f1, f2) and torch.equal(d1, d2)
    (w1, b1), (w2, b2) = (_wgrad(a, x * 1e-2, C_, k) for _ in range(2))
    assert torch.equal(w1, w2) and torch.equal(b1, b2)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _case(arch, B, seed):
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    imgs, _ = synth.make_images(B, arch.img_size, seed=seed + 1, kind='blobs')
    return params, torch.from_numpy(imgs), torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=seed + 2))


def _seen(m, cat):
    return m.profile_read('seen:' + cat)[1]


@pytest.mark.parametrize('case', ['testyaml_k6_t5_b1', 'defaults_k7_t5_b1'])
def test_reference_generic_architectures_with_split_decoder(case):
    """the body and gates of test_reference_generic_architectures_against_reference_goldens with gen_conv_precision 1: fixtures written by
    the unmodified reference (configs/test.yaml and lib/config/defaults.py, batch 1)"""
    g = load_golden(case)
    arch, params, x, eps, _ = golden_setup(g)
    m = make_hip_model(arch, params, options={'gen_conv_precision': 1, 'profile': 2})
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    assert abs(loss.item() - float(g['f64.train.loss'])) <= 1e-4 * abs(float(g['f64.train.loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f64.train.elbos']) < 1e-4
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), g['f64.train.gradfull.' + n])), n) for n, p in m.named_parameters())
    print(f'[{case}, gen_conv_precision 1] HIP vs reference fp64, element-wise: worst tensor {worst[1]} {worst[0]:.2e}')
    assert worst[0] <= 1e-3, worst
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f32.recon.elbos']) < 1e-4
    for nm, t in (('pred', pred), ('mask', mask), ('mean', mean)):
        a = t.double().cpu().flatten()
        ss = float((a * a).sum())
        assert abs(ss - float(g[f'f32.recon.{nm}.sumsq'])) <= 2e-4 * float(g[f'f32.recon.{nm}.sumsq']), nm
    amax = mask[:, :, 0].argmax(dim=1).cpu().numpy()
    assert (amax == g['f32.recon.argmax']).mean() >= 0.999
    assert _seen(m, 'gen_conv_f16x3') > 0


@pytest.mark.parametrize('what', ['dec5_clevr_128px', 'dec7_chan32_64px'])
def test_generic_decoder_at_full_image_sizes_with_split_decoder(what):
    """the cases and gates of test_generic_decoder_at_full_image_sizes (_step_vs_oracle) with gen_conv_precision 1"""
    arch, B = dict(dec5_clevr_128px=(dataclasses.replace(O.tiny_arch(slots=3, iters=1, img_size=128), dec_kernel=5, dec_chan=64, dec_layers=4, ref_chan=64,
                                                        ref_layers=4, dim_latent=64), 2),
                   dec7_chan32_64px=(dataclasses.replace(O.tiny_arch(slots=2, iters=1, img_size=64), dec_kernel=7, dec_chan=32, dec_layers=3), 2))[what]
    params, x, eps = _case(arch, B, seed=31)
    m = make_hip_model(arch, params, options={'gen_conv_precision': 1, 'profile': 2})
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    out, rg = O.train_step_grads(x, eps, params, arch)
    assert abs(loss.item() - float(out['loss'])) <= 1e-4 * abs(float(out['loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), out['elbos']) < 1e-4
    errs = [(rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy())), n) for n, p in m.named_parameters()]
    print(f'[{what}, gen_conv_precision 1] HIP vs oracle: worst tensor {max(errs)[1]} {max(errs)[0]:.2e}')
    bad = [e for e in errs if not e[0] < 2e-3]
    assert not bad, bad
    ref = O.reconstruct(x, eps, params, arch)
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']) < 1e-4
    assert rel_err(pred.cpu(), ref['pred']) < 2e-4 and rel_err(mask.cpu(), ref['mask']) < 2e-4
    p2, k2, m2 = m.reconstruct(xd, ed)
    assert torch.equal(p2, pred) and torch.equal(k2, mask)
    assert _seen(m, 'gen_conv_f16x3') > 0


# ---- semantics of the option ---------------------------------------------------------------------------------------------------------
def _run(m, xd, ed):
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    grads = [p.grad.clone() for p in m.parameters()]
    rec = [t.clone() for t in m.reconstruct(xd, ed)]
    return [loss.detach().clone()] + grads + rec


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _arch_k5(**kw):
    return dataclasses.replace(O.tiny_arch(slots=3, iters=2, img_size=32), dec_kernel=5, **kw)


def test_option_unset_equals_zero_and_toggle_returns_to_first_bits():
    arch = _arch_k5()
    params, x, eps = _case(arch, 2, seed=41)
    xd, ed = x.to(DEV), eps.to(DEV)
    base = _run(make_hip_model(arch, params), xd, ed)
    m = make_hip_model(arch, params, options={'gen_conv_precision': 0, 'profile': 2})
    first = _run(m, xd, ed)
    assert _same(base, first)
    assert _seen(m, 'gen_conv_f16x3') == 0 and _seen(m, 'gen_conv') > 0
    m.set_option('gen_conv_precision', 1)
    split = _run(m, xd, ed)
    assert _seen(m, 'gen_conv_f16x3') > 0
    assert not _same(first, split)                                         # another arithmetic: equal bits would mean it did not run
    assert rel_err(split[0].cpu(), first[0].cpu()) < 1e-5
    m.set_option('gen_conv_precision', 0)
    again = _run(m, xd, ed)
    assert _same(first, again) and _seen(m, 'gen_conv_f16x3') == 0
    with pytest.raises(RuntimeError):
        m.set_option('gen_conv_precision', 2)


def test_option_on_an_architecture_without_a_covered_layer_changes_nothing():
    """7 x 7 with 64 channels: the slice does not fit the LDS - every layer keeps its fp32 kernel, no error"""
    arch = dataclasses.replace(O.tiny_arch(slots=2, iters=1, img_size=16), dec_kernel=7, dec_chan=64)
    params, x, eps = _case(arch, 1, seed=43)
    xd, ed = x.to(DEV), eps.to(DEV)
    ref = _run(make_hip_model(arch, params, options={'gen_conv_precision': 0}), xd, ed)
    m = make_hip_model(arch, params, options={'gen_conv_precision': 1, 'profile': 2})
    got = _run(m, xd, ed)
    assert _same(ref, got) and _seen(m, 'gen_conv_f16x3') == 0 and _seen(m, 'gen_conv') > 0


def test_tuned_path_ignores_the_option():
    arch = dataclasses.replace(O.tiny_arch(slots=3, iters=2, img_size=32), dec_chan=64, ref_chan=64)
    params, x, eps = _case(arch, 2, seed=45)
    xd, ed = x.to(DEV), eps.to(DEV)
    ref = _run(make_hip_model(arch, params), xd, ed)
    m = make_hip_model(arch, params, options={'gen_conv_precision': 1, 'profile': 2})
    got = _run(m, xd, ed)
    assert _same(ref, got) and _seen(m, 'gen_conv_f16x3') == 0


def test_graph_replay_with_the_option_on_equals_eager():
    arch = _arch_k5()
    params, x, eps = _case(arch, 2, seed=47)
    eager = make_hip_model(arch, params, options={'gen_conv_precision': 1})
    graphed = make_hip_model(arch, params, options={'gen_conv_precision': 1, 'graph': 1})
    st = torch.cuda.Stream(device=DEV)
    xd, ed = x.to(DEV), eps.to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ref = _run(eager, xd, ed)
        for _ in range(3):                                                 # eager, capture, replay
            got = _run(graphed, xd, ed)
            assert _same(ref, got)
    torch.cuda.synchronize()
    assert graphed.profile_read('graph_replays')[1] > 0
