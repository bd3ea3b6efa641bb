"""Host-side checks behind the kernel-level tests of the refinement head (test_gpu_head.py, test_gpu_sgemm.py): the references are right
(autograd BPTT against a finite difference), the GEMM gate has teeth and is attainable for every case, the case tables agree with the
library's own form selection, and iodine_create accepts / refuses MLP_UNITS by the head's LDS budget with the bound in the message.
No GPU: validate and the form query are host arithmetic."""
import ctypes as C

import pytest
import torch

import head_reference as R
import test_gpu_head as TH
import test_gpu_sgemm as TS
from iodine_amd import _lib


def test_reference_bptt_agrees_with_a_finite_difference():
    L, H, Cr, N, T, B = 4, 4, 4, 2, 3, 1
    P = R.cast(R.make_params(Cr, H, L, seed=50), torch.float64)
    X = R.cast(R.bptt_inputs(L, H, Cr, N, T), torch.float64)
    var = R.VARIANTS['seed1']
    ref = R.head_bptt(P, X, T, B, var)

    def objective(Xp):
        steps, h, c = R.head_unroll(P, Xp, T)
        a, b = R.cotangents(Xp, var, T, B)
        return float(sum((a[i] * steps[i]['d_mean']).sum() + (b[i] * steps[i]['d_logvar']).sum() for i in range(T)) +
                     (Xp['dh_in'] * h[T]).sum() + (Xp['dc_in'] * c[T]).sum())

    eps = 1e-6
    for name, key in (('dpooled', 'pooled'), ('dh_out', 'h0'), ('dc_out', 'c0')):
        fd = torch.zeros_like(X[key])
        for idx in range(X[key].numel()):
            d = torch.zeros(X[key].numel(), dtype=torch.float64)
            d[idx] = eps
            d = d.view_as(X[key])
            fd.view(-1)[idx] = (objective({**X, key: X[key] + d}) - objective({**X, key: X[key] - d})) / (2 * eps)
        assert R.rel_max(ref[name], fd) < 1e-7, (name, R.rel_max(ref[name], fd))
    # the gradients at the pre-activations: chain them to the inputs by hand - dpooled_i = ds_i . W_mlp, and the gates' bias gradient
    assert R.rel_max(torch.einsum('tnh,hc->tnc', ref['ds'], P['mlp_w']), ref['dpooled']) < 1e-12
    Pb = {k: v.clone().requires_grad_(k == 'bih') for k, v in P.items()}
    steps, h, c = R.head_unroll(Pb, X, T)
    a, b = R.cotangents(X, var, T, B)
    (sum((a[i] * steps[i]['d_mean']).sum() + (b[i] * steps[i]['d_logvar']).sum() for i in range(T)) + (X['dh_in'] * h[T]).sum() +
     (X['dc_in'] * c[T]).sum()).backward()
    assert R.rel_max(ref['dgates'].sum((0, 1)), Pb['bih'].grad) < 1e-12
    assert torch.equal(ref['ddm'], a) and torch.equal(ref['ddv'], b)


def _teeth(ref, A_term, B_term, ref32, what):
    """ref: the fp64 product; one term a_ik b_kj removed from a single element must miss the gate, torch's fp32 product must pass it"""
    big = float(ref.abs().max())
    assert abs(A_term * B_term) / big > TS.GATE, (what, 'removing one term stays under the gate', abs(A_term * B_term) / big)
    e32 = float((ref32.double() - ref).abs().max()) / big
    assert e32 < TS.GATE, (what, 'the fp32 CPU product misses the gate', e32)


@pytest.mark.parametrize('case', TS.FORM0, ids=str)
def test_gemm_gate_has_teeth_and_is_attainable_form0(case):
    M, N, K, ta, tb, pa, pb = case
    A, B, C0 = TS.form0_operands(case)
    ref = TS.form0_reference(case, A, B)
    i, j, k = M - 1, N - 1, K // 2
    a = float(A[k, i] if ta else A[i, k])
    b = float(B[j, k] if tb else B[k, j])
    _teeth(ref, a, b, TS.form0_reference(case, A, B, torch.float32), case)
    # the same for the accumulating call: alpha 0.625, beta 1 over the known C
    ref1 = 0.625 * ref + C0.double()
    _teeth(ref1, 0.625 * a, b, 0.625 * TS.form0_reference(case, A, B, torch.float32) + C0, case)


@pytest.mark.parametrize('case', TS.MFMA, ids=str)
def test_gemm_gate_has_teeth_and_is_attainable_mfma(case):
    form, M, N, K, mc = case
    A, B, C0 = TS.mfma_operands(case)
    ref = TS.mfma_reference(case, A, B)
    i, j, k = M - 1, N - 1, K // 2
    a = float(A[i, k] if form == 2 else A[k, i])
    _teeth(ref, a, float(B[k, j]), TS.mfma_reference(case, A, B, torch.float32), case)
    ref1 = 0.625 * ref + C0.double()
    _teeth(ref1, 0.625 * a, float(B[k, j]), 0.625 * TS.mfma_reference(case, A, B, torch.float32) + C0, case)


def test_case_tables_match_the_library_form_selection():
    lib = _lib.lib()
    for (Cc, H, L, PL, N), forms in R.FWD_CASES.items():
        single = lib.iodine_op_refine_head_form(Cc, H, L, 0) == 0          # without a preference: the single launch wherever it fits
        split = lib.iodine_op_refine_head_form(Cc, H, L, 1) == 1
        assert forms == tuple(f for f, ok in ((0, single), (1, split)) if ok), (Cc, H, L, forms, single, split)
    assert any(L > 2 * H for (_, H, L, _, _) in R.FWD_CASES) and any(H > 256 and 0 in f for (_, H, _, _, _), f in R.FWD_CASES.items())
    for (L, H, Cr, N), forms in R.BPTT_CASES.items():
        assert (0 in forms) == (Cr <= H and L % 4 == 0 and H % 4 == 0 and Cr % 4 == 0) and 1 in forms
        assert N in R.BPTT_B and N % R.BPTT_B[N] == 0
    assert all(v in R.VARIANTS for T in R.BPTT_T for v in R.BPTT_VARIANTS[T])
    # every optional input of the backward is given in some variant and absent in another
    for key in ('wtab', 'dh_in', 'dc_in', 'carry_out'):
        assert {bool(v[key]) for v in R.VARIANTS.values()} == {False, True}
    assert {v['seeds'] for v in R.VARIANTS.values()} == {0, 1, 'T'} and {v['gl'] for v in R.VARIANTS.values()} == {None, 0.0, 0.37}
    for rows in TS.COLSUM_ROWS:
        for cols in TS.COLSUM_COLS:
            assert TS.colsum_tall_taken(rows, cols) == (rows >= 8192 and cols in (4, 256))


def _create(**kw):
    cfg = dict(dim_latent=16, iters=2, slots=2, img_size=16, img_channels=3, sigma=0.1, layernorm=1, stop_gradient=0, encoding=_lib.ENC_FULL,
               ref_conv_chan=32, ref_conv_layers=2, ref_mlp_units=128, ref_kernel_size=3, ref_stride=2, dec_conv_chan=32, dec_conv_layers=2,
               dec_kernel_size=3)
    cfg.update(kw)
    lib = _lib.lib()
    h = C.c_void_p()
    rc = lib.iodine_create(C.byref(_lib.Config(**cfg)), C.byref(h))
    msg = lib.iodine_last_error(None) or b''
    if h.value:
        lib.iodine_destroy(h)
    return rc, msg.decode()


@pytest.mark.parametrize('L,H', [(16, 4), (24, 8), (128, 32), (8, 356), (8, 360), (8, 512), (8, 1024), (256, 1024), (7, 357), (10, 1021)])
def test_create_accepts_widths_a_head_form_can_run(L, H):
    """validate passes (status 0, or 2 = no device to allocate on - never 1 = refused): DIM_LATENT > 2 MLP_UNITS, the largest single-launch
    width, and the widths only the three-launch form takes, padded ones (357 -> 360, 1021 -> 1024) included"""
    rc, msg = _create(dim_latent=L, ref_mlp_units=H)
    assert rc != 1, msg


@pytest.mark.parametrize('L,H,run_at', [(8, 364, 364), (8, 361, 364), (8, 1020, 1020), (64, 500, 500), (250, 357 + 4, 364)])
def test_create_refuses_widths_no_head_form_can_run_and_names_the_bound(L, H, run_at):
    rc, msg = _create(dim_latent=L, ref_mlp_units=H)
    assert rc == 1
    assert 'REF.MLP_UNITS' in msg and f'= {H} ' in msg and f'run at {run_at}' in msg and 'multiple of 8' in msg and '98304' in msg, msg
    assert _create(dim_latent=L, ref_mlp_units=1025)[0] == 1


def test_largest_single_launch_width_is_356_at_the_tested_shape():
    lib = _lib.lib()
    assert lib.iodine_op_refine_head_form(64, 356, 64, 0) == 0 and lib.iodine_op_refine_head_form(64, 360, 64, 0) == 1
    assert lib.iodine_op_refine_head_form(64, 364, 64, 0) == -1 and lib.iodine_op_refine_head_form(64, 364, 64, 1) == -1
    # DIM_LATENT > 2 MLP_UNITS: the update's partial sums set the size, and both forms still fit at the extremes
    assert lib.iodine_op_refine_head_form(4, 4, 256, 0) == 0 and lib.iodine_op_refine_head_form(256, 8, 256, 1) == 1


def test_case_tables_import_without_gpu_work():
    assert len(R.FWD_CASES) == 12 and len(R.BPTT_CASES) == 8 and len(TS.MFMA) >= 20 and len(TS.FORM0) >= 20
    assert TH.pytestmark.name == 'gpu' and TS.pytestmark.name == 'gpu'
