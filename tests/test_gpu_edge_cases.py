"""Edge cases of the hot path against the CPU oracle on the same seeded inputs (reference semantics:
lib/modeling/iodine.py): one slot, the maximum slot count the pixel kernels are instantiated for, a single refinement
iteration, batch of one, layer-norms switched off (ARCH.LAYERNORM, iodine.py:376-395), another likelihood sigma
(ARCH.SIGMA, iodine.py:661-666), odd layer counts, an image size off the fast path, and unsupported configurations failing loudly."""
import dataclasses

import numpy as np
import pytest
import torch

from iodine_amd import synth
from oracle import iodine_oracle as O
from util import golden_setup, grad_views, load_golden, make_hip_model, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _case(arch, B, seed):
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    imgs, _ = synth.make_images(B, arch.img_size, seed=seed + 1, kind='blobs')
    x = torch.from_numpy(imgs)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, arch.slots, arch.dim_latent, seed=seed + 2))
    return params, x, eps


CASES = {
    'one_slot': (dataclasses.replace(O.tiny_arch(slots=1, iters=2)), 3),
    'twelve_slots': (dataclasses.replace(O.tiny_arch(slots=12, iters=2)), 2),
    'one_decoder_layer': (O.tiny_arch(slots=3, iters=2, dec_layers=1), 2),             # round 6: broadcast layer + output conv only (DEC.CONV_LAYERS 1)
    'one_decoder_layer_k5': (dataclasses.replace(O.tiny_arch(slots=3, iters=2, dec_layers=1), dec_kernel=5), 2),
    'one_refinement_layer': (O.tiny_arch(slots=3, iters=2, ref_layers=1), 2),
    'sixteen_slots': (dataclasses.replace(O.tiny_arch(slots=16, iters=2)), 2),       # round 6: K = 13 .. 16 instantiated (VERDICT r05 missing #6)
    'one_iteration_batch_one': (dataclasses.replace(O.tiny_arch(slots=3, iters=1)), 1),
    'no_layernorm': (dataclasses.replace(O.tiny_arch(slots=3, iters=2), layernorm=False), 2),
    'sigma_0p3': (dataclasses.replace(O.tiny_arch(slots=4, iters=2), sigma=0.3), 2),
    'deeper_stacks_32px': (O.tiny_arch(slots=2, iters=2, img_size=32, ref_layers=3, dec_layers=3), 2),
    'dsprites_k2_t1': (O.dsprites_arch(slots=2, iters=1), 1),
    # image size that is not a power of two: the weight-stationary conv and the row-sum forms do not apply, the LDS-tiled conv
    # and the stored-gradient reductions take over (dec_path() = DEC_TILE_F16); the fused output conv backward runs without side buffer
    'large_image_256px': (O.tiny_arch(slots=2, iters=1, img_size=256), 1),
    'not_a_power_of_two_48px': (O.tiny_arch(slots=3, iters=2, img_size=48), 2),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_reconstruct_and_train_step_match_oracle(name):
    arch, B = CASES[name]
    params, x, eps = _case(arch, B, seed=100 + sorted(CASES).index(name))
    ref = O.reconstruct(x, eps, params, arch)
    m = make_hip_model(arch, params)
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    assert rel_err(m.elbo_terms.cpu()[:, 0], ref['elbos']) < 1e-4
    assert rel_err(pred.cpu(), ref['pred']) < 2e-4 and rel_err(mask.cpu(), ref['mask']) < 2e-4
    assert abs(float(mask.sum(1).mean()) - 1.0) < 1e-5                      # masks are a softmax over slots
    out, grads = O.train_step_grads(x, eps, params, arch)
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV))
    loss.backward()
    assert abs(loss.item() - out['loss'].item()) <= 1e-5 * abs(out['loss'].item())
    bad = [(n, rel_l2(p.grad.cpu().numpy(), grads[n].numpy())) for n, p in m.named_parameters()
           if not rel_l2(p.grad.cpu().numpy(), grads[n].numpy()) < 1e-3]
    assert not bad, bad


def test_gather_family_reconstruct_matches_oracle():
    """A refinement stack with an odd layer input (48 pixels, five layers: 48, 24, 12, 6, 3) runs on the gather kernels, the one family of
    the stack that no entry of CASES reaches.  Reconstruct only: the family has no data gradient at odd sizes, a training step is refused
    (test_gpu_dispatch.py::test_gather_family_launch_counts)."""
    arch = O.tiny_arch(slots=2, iters=1, img_size=48, ref_layers=5)
    params, x, eps = _case(arch, 1, seed=120)
    ref = O.reconstruct(x, eps, params, arch)
    m = make_hip_model(arch, params)
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    assert rel_err(m.elbo_terms.cpu()[:, 0], ref['elbos']) < 1e-4
    assert rel_err(pred.cpu(), ref['pred']) < 2e-4 and rel_err(mask.cpu(), ref['mask']) < 2e-4


def test_unsupported_configurations_fail_loudly():
    from iodine_amd import IODINE
    from iodine_amd.model import arch_namespace
    ok = arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))
    IODINE(ok).to(DEV).reconstruct(torch.rand(1, 3, 16, 16, device=DEV))
    with pytest.raises((RuntimeError, ValueError)):                          # 17 slots: beyond the instantiated kernels
        IODINE(arch_namespace(8, 2, 17, 16, (32, 2, 32), (32, 2))).to(DEV).reconstruct(torch.rand(1, 3, 16, 16, device=DEV))
    with pytest.raises((RuntimeError, ValueError)):                          # REF.CONV_CHAN must divide 256 (head pooling)
        IODINE(arch_namespace(8, 2, 3, 16, (48, 2, 32), (48, 2))).to(DEV).reconstruct(torch.rand(1, 3, 16, 16, device=DEV))
    with pytest.raises((RuntimeError, ValueError)):                          # even kernel size
        IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2), kernels=(3, 4))).to(DEV).reconstruct(torch.rand(1, 3, 16, 16, device=DEV))
    # (round 6: DIM_LATENT / MLP_UNITS that are not multiples of 4 run - test_latent_and_mlp_widths_that_are_not_multiples_of_4)
    m = IODINE(ok).to(DEV)
    with pytest.raises((RuntimeError, ValueError)):                          # wrong image size for this ARCH
        m.reconstruct(torch.rand(1, 3, 32, 32, device=DEV))
    with pytest.raises((RuntimeError, ValueError)):                          # CPU tensors: no fallback path
        m.reconstruct(torch.rand(1, 3, 16, 16))
    big = IODINE(arch_namespace(64, 5, 7, 128, (64, 4, 256), (64, 4))).to(DEV)
    # 32-bit element offsets: the LIBRARY fails, it does not wrap (the wrapper cuts such a batch into chunks, IODINE.max_batch)
    assert big.max_batch() == 292 and big._chunks(300, big.max_batch()) == [(0, 150), (150, 300)]
    big.max_batch = lambda training=False: 10 ** 9
    with pytest.raises(RuntimeError, match='batch too large'):
        big.reconstruct(torch.empty(300, 3, 128, 128, device=DEV))


@pytest.mark.parametrize('L,H,prec,graph,dk', [(10, 30, 1, 0, 3), (10, 30, 0, 0, 3), (6, 32, 1, 0, 3), (8, 30, 1, 0, 3), (13, 33, 1, 0, 3), (10, 30, 1, 1, 3),
                                               (10, 30, 1, 0, 5)])       # dk 5: the generic decoder (its broadcast layer takes any latent width) behind the padded handle
def test_latent_and_mlp_widths_that_are_not_multiples_of_4(L, H, prec, graph, dk):
    """iodine.py:8-32,446-464 take any DIM_LATENT / REF.MLP_UNITS; the library's refinement head moves weight rows as 16-byte vectors and
    refused other widths until round 6.  Now such a model runs on a zero-padded inner handle (iodine_pad.cpp PadShim;
    the layer-norm over the latent axis keeps the real width) with the reference's shapes at the boundary: a whole training step, reconstruct,
    elbo() from the posterior the call left, and decode against the oracle; every parameter gradient in its reference shape."""
    arch = dataclasses.replace(O.tiny_arch(slots=3, iters=2, img_size=16), dim_latent=L, ref_mlp=H, dec_kernel=dk)
    params, x, eps = _case(arch, 2, seed=41)
    m = make_hip_model(arch, params, options={'conv_precision': prec, 'graph': graph})      # graph 1: the inner handle replays, the pad / unpad launches stay eager
    assert m.get_input_size() == (17, 4 * L) and tuple(m.refine.lstm.weight_ih.shape) == (4 * H, H + 4 * L)
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    out, rg = O.train_step_grads(x, eps, params, arch)
    assert abs(loss.item() - float(out['loss'])) <= 1e-4 * abs(float(out['loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), out['elbos']) < 1e-4
    for n, p in m.named_parameters():
        assert tuple(p.grad.shape) == tuple(params[n].shape), n
    bad = [(n, rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy()))) for n, p in m.named_parameters()
           if not rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy())) < 2e-3]
    assert not bad, bad
    assert rel_err(m.posterior.mean.cpu(), out['post_mean']) < 2e-4 and tuple(m.posterior.mean.shape) == (2, 3, L)
    # a second backward accumulates into .grad like autograd (the scatter of the padded gradient honours `accumulate`)
    g1 = {n: p.grad.clone() for n, p in m.named_parameters()}
    m(xd, ed).backward()
    for n, p in m.named_parameters():
        assert rel_l2(p.grad.cpu().numpy(), 2 * g1[n].cpu().numpy()) < 1e-5, n
    ref = O.reconstruct(x, eps, params, arch)
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']) < 1e-4
    assert rel_err(pred.cpu(), ref['pred']) < 2e-4 and rel_err(mask.cpu(), ref['mask']) < 2e-4
    assert tuple(m.z.shape) == (2, 3, L)
    z = m.encode(xd, ed)
    assert tuple(z.shape) == (2, 3, L) and rel_err(z.cpu(), ref['z']) < 2e-4
    p2, k2, m2 = m.decode(z)
    assert rel_err(p2.cpu(), ref['pred']) < 2e-4
    e1 = m.elbo(xd, ed[0])                                                   # samples from lambda_T the call above left (iodine.py:636-645)
    assert torch.isfinite(e1)
    # the chunked training path (batches beyond one library call): the library ADDS the second chunk's padded gradient into the flat
    # reference-shaped buffer (iodine_train_backward_flat, accumulate = 1 -> pad_scatter with accumulate)
    if graph == 0:
        whole = {n: g.clone() for n, g in g1.items()}
        m.set_option('batch_cap', 1)
        m.zero_grad(set_to_none=True)
        lc = m(xd, ed)
        lc.backward()
        m.set_option('batch_cap', 0)
        assert abs(lc.item() - loss.item()) <= 1e-6 * abs(loss.item())
        for n, p in m.named_parameters():
            assert rel_l2(p.grad.cpu().numpy(), whole[n].cpu().numpy()) < 1e-5, n


# ---- ARCH.ENCODING subsets (round 3): the reference's DEFAULT list has no 'coordinate' (lib/config/defaults.py:57-80) -----------
@pytest.mark.parametrize('case', ['tiny_default_enc', 'cfg1_default_enc'])
@pytest.mark.parametrize('opt', [None, ('refine_split', 0), ('conv_precision', 0)])
def test_default_encoding_without_coordinate(case, opt):
    """15 input channels: weights / gradients of the first refinement layer have the reference's shape (C, 15, 3, 3); against the
    goldens generated from the unmodified reference with its default ENCODING, and against the oracle"""
    g = load_golden(case)
    arch, params, x, eps, _ = golden_setup(g)
    assert 'coordinate' not in arch.encoding and params['refine.mlc.layers.0.weight'].shape[1] == 15
    m = make_hip_model(arch, params)
    assert m.get_input_size() == (15, 4 * arch.dim_latent)
    if opt:
        m.set_option(*opt)
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    assert abs(loss.item() - float(g['f32.train.loss'])) <= 1e-4 * abs(float(g['f32.train.loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f32.train.elbos']) < 1e-4
    out, rg = O.train_step_grads(x, eps, params, arch)
    bad = [(n, rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy()))) for n, p in m.named_parameters()
           if not rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy())) < 2e-3]
    assert not bad, bad
    assert tuple(m.refine.mlc.layers[0].weight.grad.shape) == (arch.ref_chan, 15, 3, 3)
    if case.startswith('tiny'):
        for n, p in m.named_parameters():
            assert rel_l2(*grad_views(n, p.grad.cpu().numpy(), g['f64.train.grad.' + n])) < 2e-3, n
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f32.recon.elbos']) < 1e-4
    ref = O.reconstruct(x, eps, params, arch)
    assert rel_err(pred.cpu(), ref['pred']) < 2e-4


def test_encoding_subset_in_the_middle_of_the_list():
    """an arbitrary subset of the image-shaped entries (here without 'mask_posterior' and 'grad_mask': 15 channels, holes in the
    middle of the code order) against the oracle; lists without both latent entries are refused"""
    g = load_golden('tiny')
    arch, _, x, eps, _ = golden_setup(g)
    arch.encoding = tuple(e for e in O.FULL_ENCODING if e not in ('mask_posterior', 'grad_mask'))
    pn = synth.make_params(O.param_shapes(arch), seed=5, dec_gain=3.0, posterior_scale=0.1)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    m = make_hip_model(arch, params)
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV))
    loss.backward()
    out, rg = O.train_step_grads(x, eps, params, arch)
    assert abs(loss.item() - float(out['loss'])) <= 1e-4 * abs(float(out['loss']))
    bad = [(n, rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy()))) for n, p in m.named_parameters()
           if not rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy())) < 2e-3]
    assert not bad, bad
    arch.encoding = tuple(e for e in O.FULL_ENCODING if e != 'posterior')
    with pytest.raises(RuntimeError, match='grad_post'):
        make_hip_model(arch, {k: torch.zeros(s) for k, s in O.param_shapes(arch).items()}).reconstruct(x.to(DEV), eps.to(DEV))


# ---- the GENERIC fallback path (round 3): KERNEL_SIZE 5 / 7 and channel counts other than 32 / 64 ----------------------------
def _step_vs_oracle(arch, params, x, eps, tol_grad=2e-3):
    m = make_hip_model(arch, params)
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    out, rg = O.train_step_grads(x, eps, params, arch)
    assert abs(loss.item() - float(out['loss'])) <= 1e-4 * abs(float(out['loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), out['elbos']) < 1e-4
    bad = [(n, rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy()))) for n, p in m.named_parameters()
           if not rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy())) < tol_grad]
    assert not bad, bad
    for n, p in m.named_parameters():
        assert tuple(p.grad.shape) == tuple(params[n].shape), n
    ref = O.reconstruct(x, eps, params, arch)
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']) < 1e-4
    assert rel_err(pred.cpu(), ref['pred']) < 2e-4 and rel_err(mask.cpu(), ref['mask']) < 2e-4
    p2, k2, m2 = m.reconstruct(xd, ed)
    assert torch.equal(p2, pred) and torch.equal(k2, mask)                  # deterministic (fixed-order sums)
    return m


def test_kernel_size_5_matches_the_reference_golden():
    """KERNEL_SIZE 5 in both stacks + the default ENCODING: tests/golden/tiny_k5.npz comes from the unmodified reference"""
    g = load_golden('tiny_k5')
    arch, params, x, eps, _ = golden_setup(g)
    assert (arch.ref_kernel, arch.dec_kernel) == (5, 5) and tuple(params['decoder.conv.weight'].shape) == (4, 32, 5, 5)
    m = _step_vs_oracle(arch, params, x, eps)
    m.zero_grad(set_to_none=True)
    loss = m(x.to(DEV), eps.to(DEV))
    loss.backward()
    assert abs(loss.item() - float(g['f32.train.loss'])) <= 1e-4 * abs(float(g['f32.train.loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f32.train.elbos']) < 1e-4
    for n, p in m.named_parameters():
        assert rel_l2(*grad_views(n, p.grad.cpu().numpy(), g['f64.train.grad.' + n])) < 2e-3, n
    pred, mask, mean = m.reconstruct(x.to(DEV), eps.to(DEV))
    assert rel_err(pred.cpu(), g['f32.recon.pred']) < 2e-4 and rel_err(mean.cpu(), g['f32.recon.mean']) < 2e-4


@pytest.mark.parametrize('what', ['dec5_ref3', 'ref5_dec3', 'k7', 'k7_size8', 'chan16', 'chan20_dec5', 'chan24_dec', 'chan48_dec', 'chan128', 'size24', 'size40',
                                  'ref_stride1', 'ref_stride3', 'ref_stride4_k5'])
def test_generic_path_configurations(what):
    """the reference's default kernel sizes (REF 3, DEC 5), KERNEL_SIZE 7, channel counts the tuned kernels are not built for, and image
    sizes that are not a multiple of 16 (the reference only asks for a multiple of 8, lib/config/defaults.py:45); k7_size8: the smallest image with
    the largest kernel - every pixel of the broadcast layer is a border pixel, most tap windows are clipped on both sides; chan20_dec5 / chan24_dec:
    channel counts that leave the last 16-channel chunk of the MFMA conv partly empty and the last 32-channel plane of the weight gradients ragged"""
    # (round 5: the two stacks fall back separately - dec5_ref3 = generic decoder + tuned refinement kernels, ref5_dec3 the other way round)
    kw = dict(dec5_ref3=dict(ref_kernel=3, dec_kernel=5), ref5_dec3=dict(ref_kernel=5, dec_kernel=3), k7=dict(ref_kernel=7, dec_kernel=7), k7_size8=dict(ref_kernel=3, dec_kernel=7, img_size=8), chan16=dict(ref_chan=16, dec_chan=16),
              chan20_dec5=dict(dec_chan=20, dec_kernel=5), chan24_dec=dict(dec_chan=24), chan48_dec=dict(dec_chan=48), chan128=dict(ref_chan=128, dec_chan=128), size24=dict(img_size=24), size40=dict(img_size=40),
              # round 6: REF.STRIDE other than 2 (RefinementNetwork takes any, iodine.py:446-459; every shipped config uses 2): the refinement stack on the generic kernels
              ref_stride1=dict(ref_stride=1), ref_stride3=dict(ref_stride=3), ref_stride4_k5=dict(ref_stride=4, ref_kernel=5, img_size=24))[what]
    arch = dataclasses.replace(O.tiny_arch(slots=3, iters=2, img_size=32 if what in ('dec5_ref3', 'ref5_dec3') else 16), **kw)
    params, x, eps = _case(arch, 2, seed=11)
    _step_vs_oracle(arch, params, x, eps)


@pytest.mark.parametrize('what', ['dec5_clevr_128px', 'dec7_chan32_64px', 'dec5_chan48_72px'])
def test_generic_decoder_at_full_image_sizes(what):
    """the generic decoder kernels at sizes where their persistent / multi-chunk / multi-slice structure is exercised (the CLEVR shapes with
    DEC.KERNEL_SIZE 5: 64 tiles per slot-image, four 16-channel chunks, XCD-grouped blocks, the deferred epilogue, the row-staged and GEMM-form
    weight gradients with their row slices; 7 x 7 on the MFMA kernels; a size that is not a multiple of 16 with a channel count that is not a
    multiple of the chunk) - few slots and one refinement iteration keep the oracle at seconds"""
    arch, B = dict(dec5_clevr_128px=(dataclasses.replace(O.tiny_arch(slots=3, iters=1, img_size=128), dec_kernel=5, dec_chan=64, dec_layers=4, ref_chan=64,
                                                        ref_layers=4, dim_latent=64), 2),
                   dec7_chan32_64px=(dataclasses.replace(O.tiny_arch(slots=2, iters=1, img_size=64), dec_kernel=7, dec_chan=32, dec_layers=3), 2),
                   dec5_chan48_72px=(dataclasses.replace(O.tiny_arch(slots=2, iters=2, img_size=72), dec_kernel=5, dec_chan=48, dec_layers=3), 1))[what]
    params, x, eps = _case(arch, B, seed=31)
    _step_vs_oracle(arch, params, x, eps)


def test_reference_test_yaml_arch():
    """configs/test.yaml:26-52 verbatim - ITERS 5, SLOTS 6, SIGMA 0.14, DIM_LATENT 16, IMG_SIZE 64, REF 32 x 3 with KERNEL_SIZE 5 (stride 2),
    MLP 128, DEC 32 x 5 with KERNEL_SIZE 5, the four-entry ENCODING: the one shipped configuration whose REFINEMENT stack is off the tuned
    path (kernels_gens2.hip: stride-2 5 x 5 convs on fp32 MFMA since round 5), against the oracle"""
    arch = O.Arch(dim_latent=16, iters=5, slots=6, sigma=0.14, img_size=64, ref_chan=32, ref_layers=3, ref_mlp=128, ref_kernel=5,
                  dec_chan=32, dec_layers=5, dec_kernel=5, encoding=('posterior', 'grad_post', 'image', 'leave_one_out_likelihood'))
    params, x, eps = _case(arch, 2, seed=23)
    m = _step_vs_oracle(arch, params, x, eps)
    assert m.get_input_size() == (4, 64) and tuple(m.refine.mlc.layers[0].weight.shape) == (32, 4, 5, 5)


@pytest.mark.parametrize('prec', [1, 0], ids=['default_precision', 'exact_fp32'])
@pytest.mark.parametrize('case', ['testyaml_k6_t5_b1', 'defaults_k7_t5_b1'])
def test_reference_generic_architectures_against_reference_goldens(case, prec):
    """Round 6: the generic kernels (kernels_generic.hip / kernels_genl0.hip / kernels_gens2.hip) at the REAL shapes of
    the two reference architectures that need them, against fixtures written by the UNMODIFIED reference (gen_goldens.py: configs/test.yaml:26-52
    and lib/config/defaults.py:35-100 verbatim, batch 1) - loss, ELBO trajectory, every gradient tensor element-wise against the fp64 run,
    reconstruct summaries and the arg-max masks; both precisions (the defaults architecture keeps the tuned split-fp16 refinement kernels
    beside its 5 x 5 decoder at conv_precision 1; the generic kernels themselves are exact fp32 either way)."""
    g = load_golden(case)
    arch, params, x, eps, _ = golden_setup(g)
    m = make_hip_model(arch, params, options={'conv_precision': prec})
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    assert abs(loss.item() - float(g['f64.train.loss'])) <= 1e-4 * abs(float(g['f64.train.loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f64.train.elbos']) < 1e-4
    worst = max((rel_l2(*grad_views(n, p.grad.cpu().numpy(), g['f64.train.gradfull.' + n])), n) for n, p in m.named_parameters())
    print(f'[{case}, conv_precision {prec}] HIP vs reference fp64, element-wise: worst tensor {worst[1]} {worst[0]:.2e}')
    assert worst[0] <= 1e-3, worst
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), g['f32.recon.elbos']) < 1e-4
    for nm, t in (('pred', pred), ('mask', mask), ('mean', mean)):
        a = t.double().cpu().flatten()
        ss = float((a * a).sum())
        assert abs(ss - float(g[f'f32.recon.{nm}.sumsq'])) <= 2e-4 * float(g[f'f32.recon.{nm}.sumsq']), nm
    amax = mask[:, :, 0].argmax(dim=1).cpu().numpy()
    assert (amax == g['f32.recon.argmax']).mean() >= 0.999


def test_reference_default_arch():
    """lib/config/defaults.py:35-100 verbatim - ITERS 5, SLOTS 7, SIGMA 0.13, DIM_LATENT 128, IMG_SIZE 32, REF 32 x 3 (k 3, stride 2),
    MLP 256, DEC 64 x 5 with KERNEL_SIZE 5, ENCODING without 'coordinate': the configuration a user of the reference gets without a
    yaml file constructs and runs (generic path for the decoder's 5 x 5 kernels), against the oracle"""
    arch = O.Arch(dim_latent=128, iters=5, slots=7, sigma=0.13, img_size=32, ref_chan=32, ref_layers=3, ref_mlp=256, ref_kernel=3,
                  dec_chan=64, dec_layers=5, dec_kernel=5, encoding=O.DEFAULT_ENCODING)
    params, x, eps = _case(arch, 2, seed=21)
    m = _step_vs_oracle(arch, params, x, eps)
    assert m.get_input_size() == (15, 512) and tuple(m.decoder.conv.weight.shape) == (4, 64, 5, 5)


@pytest.mark.parametrize('L,H,head_mfma', [(16, 4, 1), (24, 8, 1), (24, 8, 0), (8, 512, 1), (8, 512, 0), (8, 1024, 1)])
def test_head_widths_at_the_edges_of_its_lds_budget(L, H, head_mfma):
    """DIM_LATENT > 2 MLP_UNITS: the two posterior-update products' partial sums (32 L floats) are larger than the gate partial sums the head's
    LDS used to be sized by (64 H) and ran past the allocation.  MLP_UNITS 512 / 1024: the single-launch form does not fit 96 KB; the
    three-launch form runs, with option head_mfma = 0 as well (the option only chooses where both fit).  Whole training step, reconstruct and
    every gradient against the oracle, as test_latent_and_mlp_widths_that_are_not_multiples_of_4.  REF.CONV_CHAN > MLP_UNITS (the first two
    widths) takes the backward's launch sequence, the others its fused kernel."""
    arch = dataclasses.replace(O.tiny_arch(slots=3, iters=2, img_size=16), dim_latent=L, ref_mlp=H)
    params, x, eps = _case(arch, 2, seed=61)
    m = make_hip_model(arch, params, options={'head_mfma': head_mfma})
    xd, ed = x.to(DEV), eps.to(DEV)
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    loss.backward()
    out, rg = O.train_step_grads(x, eps, params, arch)
    assert abs(loss.item() - float(out['loss'])) <= 1e-4 * abs(float(out['loss']))
    assert rel_err(m.elbo_terms[:, 0].cpu(), out['elbos']) < 1e-4
    bad = [(n, rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy()))) for n, p in m.named_parameters()
           if not rel_l2(*grad_views(n, p.grad.cpu().numpy(), rg[n].numpy())) < 2e-3]
    assert not bad, bad
    assert rel_err(m.posterior.mean.cpu(), out['post_mean']) < 2e-4
    ref = O.reconstruct(x, eps, params, arch)
    pred, mask, mean = m.reconstruct(xd, ed)
    assert rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']) < 1e-4
    assert rel_err(pred.cpu(), ref['pred']) < 2e-4 and rel_err(mask.cpu(), ref['mask']) < 2e-4


def test_mlp_units_no_head_form_can_run_are_refused_with_the_bound():
    from iodine_amd import IODINE
    from iodine_amd.model import arch_namespace
    with pytest.raises((RuntimeError, ValueError), match='REF.MLP_UNITS = 364'):
        IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 364), (32, 2))).to(DEV).reconstruct(torch.rand(1, 3, 16, 16, device=DEV))
