"""Which kernels a setting selects: the launch counts of one training step per profile category (``seen:<category>`` of
iodine_profile_read at profile 2), as formulas in the layer counts and T read off the launch sequences in iodine_dispatch.cpp.  The parity
tests say the numbers are right under every option; this one says the option reached the launch sites it is meant to reach."""
import pytest

from util import golden_setup, load_golden, make_hip_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CATEGORIES = ('conv_tile_fwd', 'conv_tile_dgrad', 'conv_tile_wgrad', 'dec_out', 'dec_out_bwd', 'dec_out_dgrad', 'dec_out_wgrad',
              'refine_conv', 'refine_wgrad', 'refine_dgrad')


def expected_launches(Dd, Dr, T, fused_out):
    """A training step decodes T + 1 times, forward and backward with weight gradients each time (elbo_and_gradients), refines T
    times, and back-propagates the refinement conv stack once, over all iterations as one batch (train_backward_impl).
    fused_out: the output conv's data and weight gradient are one launch (split-fp16 paths with out_bwd_fused), else two.
    Refinement counts are those of a stack whose layer-1 / layer-0 backward is not fused (refine_bwd01 needs 64 channels)."""
    passes = T + 1
    return {
        'conv_tile_fwd': passes * (Dd - 1),            # layers 1 .. Dd-1; layer 0 is the broadcast layer (dec_l0)
        'conv_tile_dgrad': passes * (Dd - 1),
        'conv_tile_wgrad': passes * (Dd - 1),
        'dec_out': passes,
        'dec_out_bwd': passes if fused_out else 0,
        'dec_out_dgrad': 0 if fused_out else passes,
        'dec_out_wgrad': 0 if fused_out else passes,
        'refine_conv': T * (Dr - 1),                   # layers 1 .. Dr-1 of every refinement step; layer 0 is refine_l0
        'refine_wgrad': Dr,                            # one launch per layer over all T iterations
        'refine_dgrad': Dr - 1,                        # ... and one data gradient into every layer but the first
    }


@pytest.fixture(scope='module')
def case():
    g = load_golden('cfg1_dsprites_k4_t3_b4')
    arch, params, x, eps, _ = golden_setup(g)
    assert arch.ref_chan == 32                          # (see expected_launches: no fused layer-1 / layer-0 backward)
    return arch, params, x.to(DEV), eps.to(DEV)


@pytest.mark.parametrize('options,fused_out', [
    ({}, True),                                         # weight-stationary split-fp16
    ({'conv_variant': 1}, True),                        # LDS-tiled split-fp16: same launches, other kernels
    ({'conv_precision': 0}, False),                     # exact fp32: the fused output-conv backward is a split-fp16 kernel
    ({'wgrad_accum': 1}, True),                         # partial tiles kept over the passes: the reductions move, the launches stay
], ids=['default', 'conv_variant=1', 'conv_precision=0', 'wgrad_accum=1'])
def test_training_step_launch_counts(case, options, fused_out):
    arch, params, xd, ed = case
    m = make_hip_model(arch, params, options=options)
    m.set_option('profile', 2)
    m.zero_grad(set_to_none=True)
    m(xd, ed).backward()
    got = {c: m.profile_read('seen:' + c)[1] for c in CATEGORIES}
    print(options, got)
    assert got == expected_launches(arch.dec_layers, arch.ref_layers, arch.iters, fused_out)


REF_CATEGORIES = ('refine_l0f', 'pixel_pass2', 'refine_l0', 'refine_conv', 'refine_wgrad', 'refine_bwd01', 'refine_dgrad',
                  'refine_bias_grad', 'gen_conv')


def expected_refine_launches(Dr, T, family, split=True, l0_fused=True, bwd_fused=True):
    """The refinement conv stack of one training step: T forward passes, one backward over all iterations as one batch.
    family: 's2_f16' (tuned stride-2 kernels, split fp16) or 's2_f32' (the same kernels, exact fp32), see ref_family() in iodine_dispatch.cpp;
    split / l0_fused / bwd_fused: the options refine_split / refine_l0_fused / refine_bwd_fused.
    The fused forms exist in split fp16 only and need the split first layer; the shapes below allow both (64 channels, 64 pixels)."""
    l0f = family == 's2_f16' and split and l0_fused        # encoding + layer 0 in one kernel: no pixel_pass2, no refine_l0
    fuse01 = family == 's2_f16' and split and bwd_fused and Dr >= 2      # layer 1's data gradient + layer 0's weight gradient in one
    return {
        'refine_l0f': T if l0f else 0,
        'pixel_pass2': 0 if l0f else T,
        'refine_l0': 0 if l0f else (2 * T if split else T),    # split layer 0: the per-image and the per-slot channels, a launch each
        'refine_conv': T * (Dr - 1),                           # layers 1 .. Dr-1, weight-stationary or tiled: one category
        'refine_bwd01': 1 if fuse01 else 0,
        'refine_wgrad': Dr - (1 if fuse01 else 0),             # one launch per layer over all T iterations
        'refine_dgrad': Dr - 1 - (1 if fuse01 else 0),         # ... and one data gradient into every layer but the first
        'refine_bias_grad': 0,                                 # the tuned weight-gradient kernels sum the bias gradient themselves
        'gen_conv': 0,
    }


def _refine_case(arch, seed):
    from iodine_amd import synth
    from oracle import iodine_oracle as O
    import torch
    pn = synth.make_params(O.param_shapes(arch), seed=seed, dec_gain=3.0, posterior_scale=0.05)
    params = {k: torch.from_numpy(v) for k, v in pn.items()}
    imgs, _ = synth.make_images(1, arch.img_size, seed=seed + 1, kind='blobs')
    eps = torch.from_numpy(synth.make_eps(arch.iters, 1, arch.slots, arch.dim_latent, seed=seed + 2))
    return arch, params, torch.from_numpy(imgs).to(DEV), eps.to(DEV)


@pytest.fixture(scope='module')
def refine_case():
    """The smallest shape at which every form of the tuned stack is reachable: the fused layer 0 needs S >= 32 and 64 channels, the fused
    layer-1 / layer-0 backward S >= 64, a power of two, and 64 channels; three layers leave one data gradient outside of it."""
    from oracle import iodine_oracle as O
    return _refine_case(O.tiny_arch(slots=2, iters=2, img_size=64, chan=64, mlp=32, ref_layers=3, dec_layers=2), seed=500)


def _refine_launches(case, options):
    arch, params, xd, ed = case
    m = make_hip_model(arch, params, options=options)
    m.set_option('profile', 2)
    m.zero_grad(set_to_none=True)
    m(xd, ed).backward()
    got = {c: m.profile_read('seen:' + c)[1] for c in REF_CATEGORIES}
    print(options, got)
    return got


@pytest.mark.parametrize('options,form', [
    ({}, dict(family='s2_f16')),
    ({'refine_l0_fused': 0}, dict(family='s2_f16', l0_fused=False)),
    ({'refine_split': 0}, dict(family='s2_f16', split=False)),
    ({'refine_bwd_fused': 0}, dict(family='s2_f16', bwd_fused=False)),
    ({'refine_ws': 0}, dict(family='s2_f16')),                 # the tiled kernel in place of the weight-stationary one: same category
    ({'conv_precision': 0}, dict(family='s2_f32')),
], ids=['default', 'refine_l0_fused=0', 'refine_split=0', 'refine_bwd_fused=0', 'refine_ws=0', 'conv_precision=0'])
def test_refinement_stack_launch_counts(refine_case, options, form):
    arch = refine_case[0]
    assert _refine_launches(refine_case, options) == expected_refine_launches(arch.ref_layers, arch.iters, **form)


def test_gather_family_launch_counts():
    """The gather family: a stack one of whose layers has an odd input size.  REF.CONV_LAYERS 5 at 48 pixels is the smallest such stack that
    iodine_create accepts (layer inputs 48, 24, 12, 6, 3; at 16 pixels a fifth layer is refused: 16 >> 5 == 0).  Its forward is one
    pixel_pass2 and one gather conv per layer.  Its backward does not run: the gather data gradient takes even sizes only, so the pass is
    refused at the first odd layer - loudly, with the kernel's name, and not by running another family's kernels."""
    import torch
    from oracle import iodine_oracle as O
    arch, params, xd, ed = _refine_case(O.tiny_arch(slots=2, iters=1, img_size=48, ref_layers=5), seed=510)
    Dr, T = arch.ref_layers, arch.iters
    m = make_hip_model(arch, params)
    m.set_option('profile', 2)
    m.reconstruct(xd, ed)
    torch.cuda.synchronize()
    got = {c: m.profile_read('seen:' + c)[1] for c in REF_CATEGORIES}
    print(got)
    want = dict.fromkeys(REF_CATEGORIES, 0)
    want.update(pixel_pass2=T, refine_l0=T, refine_conv=T * (Dr - 1))
    assert got == want
    m.zero_grad(set_to_none=True)
    loss = m(xd, ed)
    with pytest.raises(RuntimeError, match='launch_conv3x3_gather_dgrad'):
        loss.backward()
