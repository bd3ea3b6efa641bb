"""Which kernels a setting selects: the launch counts of one training step per profile category (``seen:<category>`` of
iodine_profile_read at profile 2), as formulas in the layer counts and T read off the launch sequence in iodine_api.cpp.  The parity
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
