"""Kernel-level parity of the per-pixel mixture kernels against float64 (tests/pixel_reference.py: the model's formulae and autograd, not the
kernels' closed forms): x_to_nhwc4_kernel, pixel_pass1_kernel<K, STRICT>, pixel_finalize_elbo_kernel, pixel_sigma_grad_kernel and its
finalize, pixel_pass2_kernel<K, SPLIT, STRICT, STABLE> and final_out_kernel<K> through iodine_op_pixel_encode, which runs the library's
launchers in the library's order.  The shapes (pixel_reference.CASES) are the ones at which the kernels take another path: a partial wave,
exactly one wave, a wave plus a tail, one full block, a second loop trip for part of a block, blocks of ppb = ceil(P / nblk) pixels with
unaligned starts (S = 23, 33, 65, 68), the finalize's unrolled loop over 8 block partials with and without its remainder (S = 64, 65, 68),
more than 256 images, K = 16 (99 statistics: all of the finalize's LDS row) on several blocks, K L below a wave and above 256.

Measure: every (image, slot, channel) plane against the plane's own largest reference element - not the whole tensor's; scalars (ll_img, kl,
scal, sgrad) against their own magnitude; the layer-norm statistics in their own right (the mean on the scale of the standard deviation, 1 /
(sd + 1e-5) against itself).  Gate of a tensor: the same formulae are evaluated in torch fp32 on the CPU for the same cases; the gate is 4 x
(strict path: another summation order, another libm) or 16 x (default path: v_exp_f32 at |x| 2^-24 + 1 ulp per exp, v_rcp_f32 at 1 ulp + 1
rounding per reciprocal, pixel_terms.h) the worst error of that evaluation against fp64 over the cases, capped at 1e-5
(pixel_reference.gates).  test_pixel_cpu.py asserts that every compared (case, tensor) is conditioned to a quarter of the cap on the CPU.
A "far" case (p_k and the pixel likelihood underflow in fp32) does not compare channel 8 without stable_encoding, channels 13 and 14 and the
statistics of 13 and 14 (pixel_reference.FAR_EXCLUDED, by name); below S = 5 the layer-norm channels and statistics are not compared.

CPU fp32 against fp64, worst over the cases (computed when the tests run; one host gave):
  g 2.30e-6, sgrad 2.19e-6, ln_g_mean 2.27e-6, mask_posterior 1.57e-6, ln_g_mask 1.11e-6, ln_like 9.6e-7, ln_loo 8.6e-7, scal 4.8e-7,
  stat_like 4.5e-7, stat_g_mask 4.0e-7, stat_loo 3.9e-7, kl_img 3.4e-7, ll_img 3.2e-7, pred 3.0e-7, mask 2.2e-7, stat_g_mean 2.2e-7,
  mean / means 9.8e-8, image, mask_logits, logits, coord 0 (their gate is 0: the kernels copy them)
Observed on MI355X (worst over the cases and the forms of pass 2):
  strict   g 3.04e-6 (K = 16, P = 4), ln_g_mean 2.13e-6, mask_posterior 1.57e-6, ln_like 1.06e-6, ln_g_mask 1.03e-6, ln_loo 8.9e-7, stat_like 7.5e-7,
           scal 5.6e-7, stat_g_mask 4.9e-7, ll_img 4.9e-7, sgrad 4.6e-7, kl_img 3.4e-7, stat_loo 3.0e-7, pred 2.9e-7, mask 2.2e-7, stat_g_mean 1.5e-7,
           mean / means 1.0e-7; image, mask_logits, logits, coord 0
  default  g 3.04e-6, ln_g_mean 2.13e-6, mask_posterior 1.57e-6, ln_g_mask 1.53e-6, ln_loo 1.05e-6, ln_like 9.8e-7, sgrad 7.3e-7, stat_like 7.1e-7,
           scal 5.6e-7, ll_img 4.9e-7, stat_g_mask 4.5e-7, kl_img 3.4e-7, stat_loo 3.0e-7, pred 2.9e-7, mask 2.2e-7, stat_g_mean 1.5e-7, means 1.1e-7,
           mean 1.0e-7; image, mask_logits, logits, coord 0
  The default path stays inside the strict path's gate on every tensor: v_exp_f32 / v_rcp_f32 cost at most 1.5 x the strict figure (ln_g_mask,
  sgrad), far inside the 16 x its documented bound allows.  Both paths are at the level of the CPU's own fp32 evaluation.
  Exact properties: two runs, an image alone / in a batch of three, w = NULL / w = 1, split / plain pass 2, channel masks (also on an input
  whose p_k all underflow), repeat counts 1 / 2 / 3, any subset of final_out's outputs: the same bits throughout.
Every output buffer carries a sentinel tail and is poisoned with a NaN of its own bit pattern: no tail is written, no poison is left.
What a wrong kernel runs into (each tried once as a source change on an MI355X): pend one short in pass 1 - g keeps poison, every test;
nvalid * 4 for nvalid * 5 - enc keeps poison wherever the plain form runs; the rotated LDS read masked with 31 - ll_img, the statistics and the
LN channels in test_against_float64; cnt[0] = P - stat_g_mean 0.42, ln_g_mean; slot 0's statistics for every slot's g_mask - ln_g_mask; no
counter reset - test_ticket_counter_is_reset (scal stays NaN); beta ignored - scal of the beta = 0.5 cases; the two coordinates swapped -
coord in test_against_float64 and test_coordinates_are_the_table."""
import ctypes as C
import functools
import itertools

import pytest
import torch

import pixel_reference as R
from iodine_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.25e9
TAIL = 64
POISON = 0x7FC0DEAD                                             # a quiet NaN no arithmetic produces
OUT = ('g', 'lnstat', 'll_img', 'img_terms', 'scal', 'sgrad', 'enc', 'enc_sh', 'pred', 'mask', 'mean', 'logits')
FORMS = list(itertools.product((0, 1), (0, 1), (0, 1)))         # (strict, split, stable)


def _check(rc, what):
    if rc == 2:     # IODINE_ERR_HIP: a launch or kernel failed - the session ends, nothing more runs on a device that may have faulted
        pytest.exit(f'{what}: {_lib.lib().iodine_last_error(None).decode()}', 3)
    _lib.check(rc, None, what)


def _out(n):
    t = torch.full((n + TAIL,), SENTINEL, device=DEV)
    t[:n].view(torch.int32).fill_(POISON)
    return t


def _take(t, shape, name):
    n = t.numel() - TAIL
    c = t.cpu()
    assert bool((c[n:] == SENTINEL).all()), f'the sentinel tail of {name} was written'
    assert not bool((c[:n].view(torch.int32) == POISON).any()), f'{name}: elements the kernels never wrote'
    return c[:n].view(*shape)


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _dev(case):
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in R.case_inputs(case).items()}


def assemble(res, split):
    """the 17 channels (B, K, P, 17) from either form of pass 2"""
    if not split:
        return res['enc'][..., :17]
    B, K, P = res['enc'].shape[:3]
    enc = torch.empty(B, K, P, 17)
    for lane, ch in enumerate(R.SPLIT_SLOT):
        if ch >= 0:
            enc[..., ch] = res['enc'][..., lane]
    for lane, ch in enumerate(R.SPLIT_SHARED):
        if ch >= 0:
            enc[..., ch] = res['enc_sh'][:, None, :, lane]
    return enc


def run(inp, strict=0, split=0, stable=0, chmask=R.CH_FULL, repeat=1, want=OUT, rows=None):
    """one call of the entry point on device inputs ``inp`` -> {name: CPU tensor}; 'enc17' the assembled channels, 'kl_img' the KL column"""
    if rows is not None:
        inp = {k: (v[rows].contiguous() if k in ('x', 'w', 'dec', 'pm', 'plv') and v is not None else v) for k, v in inp.items()}
    B, K, P = inp['dec'].shape[:3]
    S, L = inp['lin'].numel(), inp['pm'].shape[2]
    shapes = {'g': (B, K, P, 4), 'lnstat': (B, K, 8), 'll_img': (B,), 'img_terms': (B, 2), 'scal': (3,), 'sgrad': (1,),
              'enc': (B, K, P, 12 if split else 20), 'enc_sh': (B, P, 8), 'pred': (B, 3, P), 'mask': (B, K, P), 'mean': (B, K, 3, P), 'logits': (B, K, P)}
    names = [k for k in OUT if k in want and (k != 'enc_sh' or split)]
    bufs = {k: _out(torch.Size(shapes[k]).numel()) for k in names}
    arr = (C.c_void_p * 12)(*[bufs[k].data_ptr() if k in bufs else None for k in OUT])
    flags = (1 if strict else 0) | (2 if inp['use_ln'] else 0) | (4 if stable else 0)
    rc = _lib.lib().iodine_op_pixel_encode(None, _lib.ptr(inp['x']), _lib.ptr(inp['w']), _lib.ptr(inp['dec']), _lib.ptr(inp['pm']), _lib.ptr(inp['plv']),
                                           _lib.ptr(inp['lin']), B, K, S, L, inp['sigma'], inp['beta'], flags, chmask, repeat, arr)
    _check(rc, f'iodine_op_pixel_encode B {B} K {K} S {S} strict {strict} split {split} stable {stable}')
    torch.cuda.synchronize()
    res = {k: _take(bufs[k], shapes[k], k) for k in names}
    res['kl_img'] = res['img_terms'][:, 1]
    if 'enc' in res:
        res['enc17'] = assemble(res, split)
    return res


# ---- 1. against float64 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(R.CASES))
def test_against_float64(case):
    """every output of every form at the CPU-derived gates; the statistics exactly {0, 1} without layer-norm; ll_img is img_terms' column"""
    ref, cpu = R.case_reference(case)
    c = R.CASES[case]
    worst = {}
    for strict, split, stable in FORMS:
        res = run(_dev(case), strict, split, stable)
        got = {k: res[k] for k in R.SCALARS + R.PLANES + ('lnstat',)}
        got['enc'] = res['enc17']
        e = R.errors(got, ref, case, stable)
        assert set(e) == set(cpu[stable]), 'the device compares what the CPU conditioning covers'
        gate = R.gates(strict)
        bad = {k: (v, gate[k]) for k, v in e.items() if not v <= gate[k]}
        assert not bad, (case, dict(strict=strict, split=split, stable=stable), bad)
        for k, v in e.items():
            worst[(strict, k)] = max(worst.get((strict, k), 0.0), v)
        assert same_bits(res['ll_img'], res['img_terms'][:, 0])
        if not c['use_ln']:
            assert torch.equal(res['lnstat'], torch.tensor([0.0, 1.0]).repeat(c['B'], c['K'], 4))
    for strict in (1, 0):
        print(f'[pixel] {case} {"strict " if strict else "default"}: ' + ', '.join(f'{k} {v:.2e}' for (s, k), v in worst.items() if s == strict and v > 0))


# ---- 2. exact properties --------------------------------------------------------------------------------------------------------------------
EXACT_CASES = ('near_k2_s5', 'near_k1_s9_w_kl3', 'near_k3_s23_w_beta', 'near_k16_s23_w_kl1024', 'near_k11_s65', 'raw_k16_s2', 'raw_k1_s2_b300_kl3',
               'far_k2_s9', 'far_k3_s23_sat_s03')


@pytest.mark.parametrize('case', EXACT_CASES)
def test_two_runs_give_the_same_bits(case):
    for strict, split in ((0, 0), (1, 1)):
        a, b = run(_dev(case), strict, split, 0), run(_dev(case), strict, split, 0)
        diff = [k for k in a if not same_bits(a[k], b[k])]
        assert not diff, (case, strict, split, diff)


@pytest.mark.parametrize('case', list(R.CASES))
def test_split_equals_plain_and_padding_is_zero(case):
    """the split form writes the plain form's bits, channel by channel: the per-slot group (3 - 12, 14) in enc[..][12], the shared group
    (0 - 2, 13, 15, 16) in enc_sh[..][8]; the padding of both forms is exactly 0"""
    for strict, stable in itertools.product((0, 1), (0, 1)):
        plain, split = run(_dev(case), strict, 0, stable), run(_dev(case), strict, 1, stable)
        for lane, ch in enumerate(R.SPLIT_SLOT):
            if ch >= 0:
                assert same_bits(split['enc'][..., lane], plain['enc'][..., ch]), (case, strict, stable, ch)
        for lane, ch in enumerate(R.SPLIT_SHARED):
            if ch >= 0:
                for k in range(plain['enc'].shape[1]):
                    assert same_bits(split['enc_sh'][..., lane], plain['enc'][:, k, :, ch]), (case, strict, stable, ch, k)
        assert not _bits(plain['enc'][..., 17:]).any() and not _bits(split['enc'][..., 11]).any() and not _bits(split['enc_sh'][..., 6:]).any()
        others = [k for k in plain if k not in ('enc', 'enc17') and not same_bits(plain[k], split[k])]
        assert not others, (case, others)


@pytest.mark.parametrize('case', ['near_k2_s5', 'near_k3_s23_w_beta', 'near_k7_s33_kl56', 'near_k11_s65', 'raw_k16_s2'])
def test_coordinates_are_the_table(case):
    """channel 15 = lin[p % S] (x, along a row), channel 16 = lin[p / S], the caller's table bit for bit, in both forms"""
    inp = R.case_inputs(case)
    S = inp['lin'].numel()
    p = torch.arange(S * S)
    for split in (0, 1):
        enc = run(_dev(case), 0, split, 0)['enc17']
        assert torch.equal(enc[..., 15], inp['lin'][p % S].expand_as(enc[..., 15]))
        assert torch.equal(enc[..., 16], inp['lin'][p // S].expand_as(enc[..., 16]))
        assert torch.equal(enc[..., :3], inp['x'].permute(0, 2, 1)[:, None].expand_as(enc[..., :3]))      # and the image is the caller's


@pytest.mark.parametrize('case', ['near_k7_s33_kl56', 'far_k3_s23_sat_s03', 'raw_k16_s2'])
def test_an_image_alone_and_in_a_batch_of_three(case):
    """g, enc, lnstat and ll_img of an image do not depend on the images around it"""
    for strict, split in ((0, 0), (0, 1), (1, 0)):
        full = run(_dev(case), strict, split, 0)
        for b in (0, 2):
            one = run(_dev(case), strict, split, 0, rows=slice(b, b + 1))
            keys = ['g', 'enc', 'lnstat', 'll_img', 'kl_img', 'pred', 'mask', 'mean', 'logits'] + (['enc_sh'] if split else [])
            diff = [k for k in keys if not same_bits(one[k][0], full[k][b])]
            assert not diff, (case, strict, split, b, diff)


@pytest.mark.parametrize('case', ['near_k2_s5', 'near_k1_s17', 'near_k7_s33_kl56', 'near_k16_s65_beta', 'far_k2_s9', 'raw_k3_s1'])
def test_unit_weights_change_no_bit(case):
    inp = _dev(case)
    assert inp['w'] is None
    B, _, P = inp['x'].shape
    ones = {**inp, 'w': torch.ones(B, P, device=DEV)}
    for strict, split in ((0, 0), (1, 1)):
        a, b = run(inp, strict, split, 0), run(ones, strict, split, 0)
        diff = [k for k in a if not same_bits(a[k], b[k])]
        assert not diff, (case, strict, split, diff)


@pytest.mark.parametrize('case', [k for k, c in R.CASES.items() if c['weighted']])
def test_unobserved_pixels_get_no_gradient(case):
    inp = R.case_inputs(case)
    zero = inp['w'] == 0
    assert zero.any()
    for strict in (0, 1):
        g = run(_dev(case), strict, 0, 0, want=OUT[:5])['g']                                   # (B, K, P, 4)
        assert not g.permute(0, 2, 1, 3)[zero].any(), (case, strict)
        assert g.permute(0, 2, 1, 3)[~zero].abs().amax(dim=(1, 2)).min() > 0                    # ... and only they


@functools.lru_cache(maxsize=None)
def _underflow_inputs():
    """a far input scaled until every p_k and the pixel likelihood underflow in fp32 (means at 0 / 1 against an image inside [0.05, 0.95],
    sigma 0.02: sum_c l_kc < -104 for every slot of most pixels): channel 8 of the reference is 0 / 0 there"""
    inp = R.make_inputs(**{**R.CASES['far_k7_s33_w_s03_beta'], 'sigma': R.f32(0.02)}, far_scale=6.0)
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in inp.items()}


@pytest.mark.parametrize('chmask', [R.CH_DEFAULT, R.CH_HOLES], ids=['default_encoding', 'holes'])
@pytest.mark.parametrize('which', ['near', 'underflow'])
def test_channel_mask(which, chmask):
    """an absent channel is exactly 0, a present one keeps its bits - also where the absent channel's value would be NaN"""
    inp = _dev('near_k3_s23_w_beta') if which == 'near' else _underflow_inputs()
    present = [c for c in range(17) if chmask >> c & 1]
    absent = [c for c in range(17) if not chmask >> c & 1]
    for strict, split, stable in ((0, 0, 1), (0, 1, 1), (1, 0, 1), (0, 0, 0), (0, 1, 0)):
        full, part = run(inp, strict, split, stable), run(inp, strict, split, stable, chmask=chmask)
        if which == 'underflow' and not stable:
            assert torch.isnan(full['enc17'][..., 8]).any(), 'the input does not underflow'
        assert same_bits(part['enc17'][..., present], full['enc17'][..., present]), (which, strict, split, stable)
        assert not _bits(part['enc17'][..., absent]).any(), (which, strict, split, stable)
        if stable or 8 in absent:
            assert not any(torch.isnan(part[k]).any() for k in OUT if k in part), (which, strict, split, stable)
        pad = part['enc'][..., 11] if split else part['enc'][..., 17:]
        assert not _bits(pad).any()
        rest = [k for k in full if k not in ('enc', 'enc_sh', 'enc17') and not same_bits(full[k], part[k])]
        assert not rest, rest


@pytest.mark.parametrize('case', ['near_k2_s5', 'near_k7_s33_kl56', 'near_k3_s23_w_beta', 'raw_k1_s2_b300_kl3', 'near_k11_s65'])
def test_ticket_counter_is_reset(case):
    """two finalize launches on one counter: the second elects a last block again (the entry point poisons scal in between), so scal - and
    everything else - has the bits of a single launch"""
    once, twice, thrice = run(_dev(case), 0, 0, 0), run(_dev(case), 0, 0, 0, repeat=2), run(_dev(case), 1, 1, 0, repeat=3)
    assert not torch.isnan(twice['scal']).any() and not torch.isnan(thrice['scal']).any()
    diff = [k for k in once if not same_bits(once[k], twice[k])]
    assert not diff, (case, diff)
    strict = run(_dev(case), 1, 1, 0)
    assert same_bits(strict['scal'], thrice['scal']) and same_bits(strict['img_terms'], thrice['img_terms'])


def test_final_out_with_any_subset_of_its_outputs():
    inp = _dev('near_k3_s23_w_beta')
    full = run(inp, 0, 0, 0)
    for keep in itertools.product((False, True), repeat=4):
        want = OUT[:5] + tuple(k for k, on in zip(OUT[8:], keep) if on)
        res = run(inp, 0, 0, 0, want=want)
        assert all(same_bits(res[k], full[k]) for k in want), keep
    # the optional steps alone: d LL / d sigma without the encoding, the encoding without d LL / d sigma
    a, b = run(inp, 0, 1, 0, want=OUT[:6]), run(inp, 0, 0, 0, want=OUT[:5] + ('enc',))
    assert same_bits(a['sgrad'], full['sgrad']) and same_bits(b['enc'], full['enc'])


def test_refusals_launch_nothing():
    inp = _dev('near_k2_s5')
    bufs = [_out(4096) for _ in OUT]
    arr = (C.c_void_p * 12)(*[t.data_ptr() for t in bufs])
    L = _lib.lib()
    for bad in (dict(K=17), dict(K=0), dict(S=0), dict(sigma=0.0), dict(repeat=0), dict(x=None), dict(lin=None)):
        rc = L.iodine_op_pixel_encode(None, _lib.ptr(bad.get('x', inp['x'])), None, _lib.ptr(inp['dec']), _lib.ptr(inp['pm']), _lib.ptr(inp['plv']),
                                      _lib.ptr(bad.get('lin', inp['lin'])), 1, bad.get('K', 2), bad.get('S', 5), 8, bad.get('sigma', inp['sigma']), 1.0, 0,
                                      R.CH_FULL, bad.get('repeat', 1), arr)
        assert rc == 1, bad
    torch.cuda.synchronize()
    for t in bufs:                                                                            # untouched: poison and tail as they were
        c = t.cpu()
        assert bool((c[:4096].view(torch.int32) == POISON).all()) and bool((c[4096:] == SENTINEL).all())
