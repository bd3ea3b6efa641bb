"""Kernel-level parity of the refinement head's GEMMs and column sums (kernels_gemm.hip: sgemm_kernel<64 | 256>, sgemm_tn_mfma_kernel
<SPLITK, MODE, AROW>, colsum / colsum_tall) against float64, through iodine_op_sgemm / iodine_op_colsum.  C carries a sentinel ring (ldc > N,
rows past M); beta = 0 runs over a NaN-filled C, which must not be read; beta = 1 over a known C with alpha != 1.  The gate is the project's
gate of exact-fp32 kernels, 2e-6 of the largest reference element (test_gpu_gen_s2.py); test_head_cpu.py shows for every case that the
gate has teeth (the fp64 product with ONE a_ik b_kj term removed misses it) and is attainable (torch's fp32 CPU product passes it).
The case tables are imported by test_head_cpu.py: no GPU work at import.
Deviation from the issue's table: mode 1 (the broadcast layer's index map) needs M = L to be a multiple of 32, so `ldc = L + 2 = 10` cannot
be run; the cases are C = 32 with L + 2 = 34 and C = 64 with L + 2 = 66.
Observed on MI355X, relative to the largest reference element (worst over the cases; `pytest -s` prints each): the dispatch (form 0)
8.35e-7, the MFMA forms 4.75e-7, column sums 2.71e-7 (the tall form 1.6e-7)."""
import functools

import pytest
import torch

from iodine_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.25e9
GATE = 2e-6                                                     # exact-fp32 kernels (GATE in test_gpu_gen_s2.py)

# form 0, the library's dispatch: (M, N, K, ta, tb, pad_a, pad_b) - pad = leading dimension minus the row length
FORM0 = [
    (36, 128, 16, 0, 0, 0, 0), (8, 32, 512, 0, 0, 4, 8),            # vector path (everything a multiple of 4), BK = 64 and 256
    (36, 128, 16, 1, 0, 4, 0), (8, 32, 512, 1, 0, 0, 4),            # ... its A^T form (M not a multiple of 32: stays on sgemm_kernel)
    (7, 36, 20, 0, 0, 0, 0), (33, 30, 144, 0, 0, 3, 1),             # scalar path: a dimension that is not a multiple of 4
    (7, 36, 20, 1, 0, 1, 0), (33, 30, 144, 1, 0, 0, 2),
    (36, 128, 16, 0, 0, 1, 0), (36, 128, 16, 0, 0, 0, 3),           # scalar path through lda / ldb alone
    (20, 24, 63, 0, 0, 0, 0), (20, 24, 64, 0, 0, 0, 0), (20, 24, 65, 0, 0, 0, 0), (20, 24, 255, 0, 0, 0, 0),      # K around the BK steps
    (20, 24, 512, 0, 0, 0, 0), (20, 24, 520, 0, 0, 0, 0), (21, 24, 512, 0, 0, 0, 0), (21, 26, 520, 1, 0, 0, 0),
    (400, 336, 512, 0, 0, 0, 0),                                    # 525 blocks at K >= 512: BK = 64
    (19, 45, 100, 0, 0, 0, 0),                                      # M, N not multiples of 16
    (20, 24, 65, 0, 1, 0, 0), (36, 128, 16, 0, 1, 0, 4), (33, 30, 144, 1, 1, 1, 0),    # tb = 1
    (48, 40, 64, 1, 0, 0, 0), (40, 64, 96, 1, 0, 0, 0),             # ta = 1, M or N not a multiple of 32: sgemm_kernel
    (64, 32, 100, 1, 0, 0, 0),                                      # ta = 1, multiples of 32: dispatched to the MFMA kernel
]
# MFMA forms: (form, M, N, K, mode_c); form 1 A [K][M], 2 A row-major [M][K], 3 the broadcast layer's index map (N = 9 mode_c, ldc = M + 2)
MFMA = ([(f, 32, 32, k, 0) for f in (1, 2) for k in (1, 2, 3, 63, 64, 65, 66, 1120)] +
        [(1, 64, 256, 1120, 0),                                     # 16 tiles: split-K
         (1, 1024, 544, 96, 0),                                     # 544 tiles: not split
         (2, 32, 128, 48, 0), (2, 224, 1024, 768, 0),               # row-major A: K < 64 not split; the gate GEMM's shape
         (3, 32, 288, 3, 32), (3, 32, 288, 231, 32), (3, 64, 576, 77, 64)])
COLSUM_ROWS = (1, 255, 8191, 8192, 20000)
COLSUM_COLS = (4, 36, 256, 1024)


def colsum_tall_taken(rows, cols):
    return rows >= 8192 and cols % 4 == 0 and cols <= 256 and 256 % (cols // 4) == 0


def _rand(*shape, seed):
    """|x| in [0.5, 1), random sign: no term of a product is negligible"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.rand(*shape, generator=g, dtype=torch.float64) * 0.5 + 0.5
    sgn = torch.randint(0, 2, shape, generator=g, dtype=torch.float64) * 2 - 1
    return (mag * sgn).float()


def form0_operands(case):
    """A, B as stored (leading dimension = row length + pad), C0 the known prefill"""
    M, N, K, ta, tb, pa, pb = case
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)
    return _rand(ra, ca + pa, seed=11), _rand(rb, cb + pb, seed=12), _rand(M, N, seed=13) * 10


def form0_reference(case, A, B, dtype=torch.float64):
    M, N, K, ta, tb, pa, pb = case
    a = A[:, :M if ta else K].to(dtype)
    b = B[:, :K if tb else N].to(dtype)
    return (a.T if ta else a) @ (b.T if tb else b)


def mfma_operands(case):
    form, M, N, K, mc = case
    A = _rand(M, K + 3, seed=21) if form == 2 else _rand(K, M + 32, seed=21)          # lda > the row length
    return A, _rand(K, N + 32, seed=22), _rand(M, N, seed=23) * 10


def mfma_reference(case, A, B, dtype=torch.float64):
    form, M, N, K, mc = case
    a = A[:, :K].to(dtype).T if form == 2 else A[:, :M].to(dtype)
    return a.T @ B[:, :N].to(dtype)


def _check(rc, what):
    if rc == 2:     # IODINE_ERR_HIP: a launch or kernel failed - the session ends, nothing more runs on a device that may have faulted
        pytest.exit(f'{what}: {_lib.lib().iodine_last_error(None).decode()}', 3)
    _lib.check(rc, None, what)


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _run(form, ta, tb, M, N, K, alpha, A, B, beta, C0, mode_c=0):
    """-> the M x N result (mode 1: gathered back through the index map); asserts the sentinel ring"""
    Ad, Bd = A.to(DEV).contiguous(), B.to(DEV).contiguous()
    if form == 3:
        L, Cc = M, mode_c
        ldc = L + 2
        buf = torch.full((Cc, ldc, 9), SENTINEL, device=DEV)
        # gw[co][ci][tap] for row = ci < L, column = tap * Cc + co
        fill = float('nan') if beta == 0 else None
        if fill is not None:
            buf[:, :L] = fill
        else:
            buf[:, :L] = C0.view(L, 9, Cc).permute(2, 0, 1).to(DEV)
        rc = _lib.lib().iodine_op_sgemm(None, 3, 0, 0, M, N, K, alpha, _lib.ptr(Ad), A.shape[1], _lib.ptr(Bd), B.shape[1], beta, _lib.ptr(buf),
                                        ldc, mode_c)
        _check(rc, f'iodine_op_sgemm form 3 {(M, N, K, mode_c)}')
        torch.cuda.synchronize()
        out = buf.cpu()
        assert bool((out[:, L:] == SENTINEL).all()), 'the coordinate planes of gw were written'
        return out[:, :L].permute(1, 2, 0).reshape(L, N)
    ldc = N + 5
    buf = torch.full((M + 3, ldc), SENTINEL, device=DEV)
    buf[:M, :N] = float('nan') if beta == 0 else C0.to(DEV)
    rc = _lib.lib().iodine_op_sgemm(None, form, ta, tb, M, N, K, alpha, _lib.ptr(Ad), A.shape[1], _lib.ptr(Bd), B.shape[1], beta, _lib.ptr(buf),
                                    ldc, 0)
    _check(rc, f'iodine_op_sgemm form {form} {(M, N, K, ta, tb)}')
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[M:] == SENTINEL).all()) and bool((out[:, N:] == SENTINEL).all()), 'the ring around C was written'
    return out[:M, :N].contiguous()


def _both_betas(tag, form, ta, tb, M, N, K, A, B, C0, ref, mode_c=0):
    got0 = _run(form, ta, tb, M, N, K, 1.0, A, B, 0.0, C0, mode_c)
    assert bool(torch.isfinite(got0).all()), 'beta = 0 read the NaN prefill of C'
    e0 = _rel(got0, ref)
    ref1 = 0.625 * ref + C0.double()
    got1 = _run(form, ta, tb, M, N, K, 0.625, A, B, 1.0, C0, mode_c)
    e1 = _rel(got1, ref1)
    again = _run(form, ta, tb, M, N, K, 1.0, A, B, 0.0, C0, mode_c)
    print(f'[sgemm {tag}] beta 0: {e0:.2e}, alpha 0.625 beta 1: {e1:.2e}')
    assert e0 < GATE and e1 < GATE, (e0, e1)
    assert torch.equal(got0, again), 'two runs differ'


@pytest.mark.parametrize('case', FORM0, ids=str)
def test_sgemm_dispatch(case):
    M, N, K, ta, tb, pa, pb = case
    A, B, C0 = form0_operands(case)
    _both_betas(f'form 0 {case}', 0, ta, tb, M, N, K, A, B, C0, form0_reference(case, A, B))


@pytest.mark.parametrize('case', MFMA, ids=str)
def test_sgemm_mfma(case):
    form, M, N, K, mc = case
    A, B, C0 = mfma_operands(case)
    _both_betas(f'form {form} {case[1:]}', form, 0, 0, M, N, K, A, B, C0, mfma_reference(case, A, B), mc)


def test_sgemm_entry_refuses_what_a_form_does_not_take():
    A = torch.zeros(64, 64, device=DEV)
    L = _lib.lib()
    for args in [(1, 0, 0, 33, 32, 8, 1.0, _lib.ptr(A), 64, _lib.ptr(A), 64, 0.0, _lib.ptr(A), 64, 0),       # M not a multiple of 32
                 (3, 0, 0, 32, 32, 8, 1.0, _lib.ptr(A), 64, _lib.ptr(A), 64, 0.0, _lib.ptr(A), 34, 4),       # N != 9 mode_c
                 (0, 0, 0, 8, 8, 8, 1.0, _lib.ptr(A), 4, _lib.ptr(A), 64, 0.0, _lib.ptr(A), 64, 0)]:         # lda < K
        assert L.iodine_op_sgemm(None, *args) == 1
    assert L.iodine_op_colsum(None, 1, _lib.ptr(A), 64, 64, 64, 1.0, _lib.ptr(A)) == 1                       # too short for the tall form


@functools.lru_cache(maxsize=None)
def _colsum_src(rows, cols):
    return _rand(rows, cols + 4, seed=31)


@pytest.mark.parametrize('cols', COLSUM_COLS)
@pytest.mark.parametrize('rows', COLSUM_ROWS)
def test_colsum(rows, cols):
    src = _colsum_src(rows, cols)
    d0 = _rand(cols, seed=32) * 10
    alpha = -0.375
    e = {}
    for form, ld in ((0, cols + 4), (0, cols)) + (((1, cols),) if colsum_tall_taken(rows, cols) else ()):
        s = src if ld > cols else src[:, :cols].contiguous()
        ref = d0.double() + alpha * s[:, :cols].double().sum(0)
        dst = torch.full((cols + 8,), SENTINEL, device=DEV)
        dst[:cols] = d0.to(DEV)
        sd = s.to(DEV)
        _check(_lib.lib().iodine_op_colsum(None, form, _lib.ptr(sd), rows, cols, ld, alpha, _lib.ptr(dst)), f'iodine_op_colsum {(form, rows, cols, ld)}')
        torch.cuda.synchronize()
        out = dst.cpu()
        assert bool((out[cols:] == SENTINEL).all())
        # relative to the largest term of the result: the prefill or the sum
        e[(form, ld)] = float((out[:cols].double() - ref).abs().max() / ref.abs().max())
    print(f'[colsum] rows {rows} cols {cols}: ' + ', '.join(f'form {k[0]} ld {k[1]}: {v:.2e}' for k, v in e.items()))
    assert all(v < GATE for v in e.values()), e
