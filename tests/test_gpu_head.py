"""Kernel-level parity of the refinement head against float64 (tests/head_reference.py: the model's formulae and autograd, not the kernels):
refine_head_kernel<0 | 1 | 2> in its single-launch and three-launch form through iodine_op_refine_head, head_bptt_kernel<SEED> and the launch
sequence it replaces through iodine_op_head_bptt, pool_bwd through iodine_op_pool_bwd.  The shapes are the ones at which the head takes
another path: DIM_LATENT > 2 MLP_UNITS (the posterior-update partial sums are then the largest user of the LDS), MLP_UNITS > 256 (fewer than
16 K slices in the gate loop, the second 256-column pass of head_matvec), the largest width of the single-launch form, widths only the
three-launch form takes, REF.CONV_CHAN > MLP_UNITS (only the launch sequence), odd row counts (the clamped tail row of a block).
Gate: sigmoid, tanh and expf leave no closed bound, so the same formulae are evaluated in torch fp32 on the CPU for the same cases; the gate of
a tensor is 4 x the worst error of that evaluation against fp64 over the cases, relative to the tensor's largest element, capped at 1e-5
(head_gates / bptt_gates below; the margin covers another summation order and another libm).
The figure is computed when the tests run, so it is the host CPU's own BLAS that sets it: two hosts gave (worst over the cases)
  forward  h 9.2e-7 / 1.07e-6, c 5.3e-7 / 5.9e-7, pm 4.8e-7 / 2.7e-7, plv 3.5e-7 / 3.2e-7, d_mean 5.6e-7 / 4.1e-7, d_logvar 4.8e-7 / 4.5e-7,
           pooled 1.3e-7, s 2.5e-7, gates 1.82e-6 / 1.47e-6, xin 2.7e-7
  BPTT     ddm, ddv 9.8e-8, dgates 9.5e-7 / 1.12e-6, ds 7.2e-7 / 2.61e-6, dpooled 1.00e-6 / 2.15e-6, dh_out 7.4e-7 / 2.66e-6, dc_out 5.9e-7 / 9.9e-7
  pool_bwd 3.1e-8 ... 6.8e-8
Observed on MI355X (worst over the cases, forms and variants, relative to each tensor's largest element):
  forward  h 1.16e-6, c 8.6e-7, pm 2.6e-7, plv 3.1e-7, d_mean 4.3e-7, d_logvar 4.6e-7, pooled 1.2e-7, s 2.0e-7, gates 2.62e-6, xin 2.2e-7;
           two runs and a slot alone / in a batch of 33: the same bits, both forms
  BPTT     ddm, ddv 9.8e-8, dgates 8.8e-7, ds 2.42e-6, dpooled 1.57e-6, dh_out 2.35e-6, dc_out 9.3e-7; the fused kernel against the launch
           sequence: dgates 9.1e-7, ds 2.47e-6, dpooled 1.78e-6, dh_out 2.31e-6, dc_out 9.0e-7
  pool_bwd 3.1e-8 ... 6.9e-8
The case tables live in head_reference.py; test_head_cpu.py imports them: no GPU work at import."""
import ctypes as C
import functools

import pytest
import torch

import head_reference as R
from iodine_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.25e9
TAIL = 64


def _check(rc, what):
    if rc == 2:     # IODINE_ERR_HIP: a launch or kernel failed - the session ends, nothing more runs on a device that may have faulted
        pytest.exit(f'{what}: {_lib.lib().iodine_last_error(None).decode()}', 3)
    _lib.check(rc, None, what)


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _out(*shape, fill=None):
    """a flat device buffer of prod(shape) floats followed by a sentinel tail"""
    n = 1
    for s in shape:
        n *= s
    t = torch.full((n + TAIL,), SENTINEL, device=DEV)
    if fill is not None:
        t[:n] = fill.reshape(-1).to(DEV)
    return t


def _take(t, *shape):
    n = t.numel() - TAIL
    c = t.cpu()
    assert bool((c[n:] == SENTINEL).all()), 'a sentinel tail was written'
    return c[:n].view(*shape)


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_case(case):
    """parameters, inputs, the fp64 reference and the fp32-CPU evaluation's errors of a case: computed once, never modified"""
    Cc, H, L, PL, N = case
    P, X = R.make_params(Cc, H, L), R.head_inputs(Cc, H, L, PL, N)
    ref = R.head_forward(R.cast(P, torch.float64), **R.cast(X, torch.float64))
    f32 = R.head_forward(P, **X)
    return P, X, ref, {k: R.rel_max(f32[k], ref[k]) for k in R.FWD_OUT}


@functools.lru_cache(maxsize=None)
def head_gates():
    worst = {k: max(_fwd_case(c)[3][k] for c in R.FWD_CASES) for k in R.FWD_OUT}
    print('[head fwd] CPU fp32 against fp64, worst over the cases: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    return {k: min(4 * v, R.HEAD_GATE_CAP) for k, v in worst.items()}


def _run_fwd(form, case, P, X, rows=None):
    Cc, H, L, PL, N = case
    if rows is not None:
        X = {k: v[rows].contiguous() for k, v in X.items()}
        N = X['feat'].shape[0]
    ins = [P[k].to(DEV).contiguous() for k in R.PARAMS] + [X[k].to(DEV).contiguous() for k in ('feat', 'latent', 'h_prev', 'c_prev')]
    shapes = {'h': (N, H), 'c': (N, H), 'pm': (N, L), 'plv': (N, L), 'd_mean': (N, L), 'd_logvar': (N, L), 'pooled': (N, Cc), 's': (N, H),
              'gates': (N, 4 * H), 'xin': (N, H + 4 * L)}
    outs = {k: _out(*shapes[k], fill=X[k] if k in ('pm', 'plv') else None) for k in R.FWD_OUT}
    rc = _lib.lib().iodine_op_refine_head(None, form, _ptr_array(ins), _ptr_array([outs[k] for k in R.FWD_OUT]), N, PL, Cc, H, L)
    _check(rc, f'iodine_op_refine_head form {form} {case}')
    torch.cuda.synchronize()
    return {k: _take(outs[k], *shapes[k]) for k in R.FWD_OUT}


@pytest.mark.parametrize('case', list(R.FWD_CASES), ids=str)
def test_head_forward(case):
    P, X, ref, _ = _fwd_case(case)
    gates = head_gates()
    L = _lib.lib()
    for form in (0, 1):
        if form not in R.FWD_CASES[case]:
            ins = [P[k].to(DEV).contiguous() for k in R.PARAMS] + [X[k].to(DEV).contiguous() for k in ('feat', 'latent', 'h_prev', 'c_prev')]
            o = [_out(4) for _ in R.FWD_OUT]
            assert L.iodine_op_refine_head(None, form, _ptr_array(ins), _ptr_array(o), case[4], case[3], case[0], case[1], case[2]) == 1, \
                f'form {form} must be refused at {case}'
            continue
        got = _run_fwd(form, case, P, X)
        e = {k: R.rel_max(got[k], ref[k]) for k in R.FWD_OUT}
        print(f'[head fwd] {case} form {form}: ' + ', '.join(f'{k} {v:.2e}' for k, v in e.items()))
        bad = {k: (v, gates[k]) for k, v in e.items() if not v < gates[k]}
        assert not bad, bad
        again = _run_fwd(form, case, P, X)
        assert all(torch.equal(got[k], again[k]) for k in R.FWD_OUT), 'two runs differ'


@pytest.mark.parametrize('case,form', [((64, 256, 64, 64, 33), 0), ((64, 256, 64, 64, 33), 1), ((64, 512, 8, 4, 33), 1)], ids=str)
def test_head_forward_slot_bits_do_not_depend_on_the_batch(case, form):
    """a slot's outputs are the same bits alone (N = 1) and as row 0 of N = 33 - and as the last row, behind the padding rows of the gate GEMM"""
    P, X, _, _ = _fwd_case(case)
    full = _run_fwd(form, case, P, X)
    for row in (0, 32):
        one = _run_fwd(form, case, P, X, rows=slice(row, row + 1))
        diff = [k for k in R.FWD_OUT if not torch.equal(one[k][0], full[k][row])]
        assert not diff, (row, diff)


# ---- BPTT -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bptt_case(case, T):
    L, H, Cr, N = case
    return R.make_params(Cr, H, L, seed=50), R.bptt_inputs(L, H, Cr, N, T)


@functools.lru_cache(maxsize=None)
def _bptt_ref(case, T, vname):
    P, X = _bptt_case(case, T)
    B = R.BPTT_B[case[3]]
    ref = R.head_bptt(R.cast(P, torch.float64), R.cast(X, torch.float64), T, B, R.VARIANTS[vname])
    f32 = R.head_bptt(P, X, T, B, R.VARIANTS[vname])
    return ref, {k: R.rel_max(f32[k], ref[k]) for k in R.BPTT_OUT}


@functools.lru_cache(maxsize=None)
def bptt_gates():
    worst = {k: 0.0 for k in R.BPTT_OUT}
    for case in R.BPTT_CASES:
        for T in R.BPTT_T:
            for v in R.BPTT_VARIANTS[T]:
                for k, e in _bptt_ref(case, T, v)[1].items():
                    worst[k] = max(worst[k], e)
    print('[head bptt] CPU fp32 against fp64, worst over the cases: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    return {k: min(4 * v, R.HEAD_GATE_CAP) for k, v in worst.items()}


def _run_bptt(form, case, T, vname, P, X, ref):
    """the kernel gets the fp32 roundings of the fp64 forward's saved tensors"""
    L, H, Cr, N = case
    var = R.VARIANTS[vname]
    d = lambda t: t.float().to(DEV).contiguous()
    seeded = bool(var['seeds'])
    opt = [None] * 6
    if seeded:
        opt[0], opt[1] = (d(X['seedT_m']), d(X['seedT_v'])) if var['seeds'] == 'T' else (d(X['seed1_m']), d(X['seed1_v']))
        if var['gl'] is not None:
            opt[2] = torch.tensor([var['gl']], device=DEV)
    if var['wtab']:
        opt[3] = d(X['wtab'])
    if var['dh_in']:
        opt[4] = d(X['dh_in'])
    if var['dc_in']:
        opt[5] = d(X['dc_in'])
    ins = [d(X['g_pm']), d(X['g_plv']), d(ref['gates']), d(ref['c']), d(ref['s']), d(P['wm']), d(P['wv']), d(P['whh']), d(P['wih']), d(P['mlp_w'])] + opt
    shapes = {'ddm': (T, N, L), 'ddv': (T, N, L), 'dgates': (T, N, 4 * H), 'ds': (T, N, H), 'dpooled': (T, N, Cr), 'dh_out': (N, H), 'dc_out': (N, H)}
    outs = {k: _out(*shapes[k]) for k in R.BPTT_OUT}
    names = [k for k in R.BPTT_OUT if var['carry_out'] or k not in ('dh_out', 'dc_out')]
    rc = _lib.lib().iodine_op_head_bptt(None, form, _ptr_array(ins), _ptr_array([outs[k] if k in names else None for k in R.BPTT_OUT]),
                                        T, N, R.BPTT_B[N], L, H, Cr, N * L if var['seeds'] == 'T' else 0)
    _check(rc, f'iodine_op_head_bptt form {form} {case} T {T} {vname}')
    torch.cuda.synchronize()
    res = {k: _take(outs[k], *shapes[k]) for k in R.BPTT_OUT}
    for k in R.BPTT_OUT:
        if k not in names:
            assert bool((res[k] == SENTINEL).all())
    return {k: res[k] for k in names}


@pytest.mark.parametrize('T', R.BPTT_T)
@pytest.mark.parametrize('case', list(R.BPTT_CASES), ids=str)
def test_head_bptt(case, T):
    L, H, Cr, N = case
    P, X = _bptt_case(case, T)
    gates = bptt_gates()
    lib = _lib.lib()
    for vname in R.BPTT_VARIANTS[T]:
        ref, _ = _bptt_ref(case, T, vname)
        got = {}
        for form in (0, 1):
            if form not in R.BPTT_CASES[case]:
                continue
            got[form] = _run_bptt(form, case, T, vname, P, X, ref)
            e = {k: R.rel_max(v, ref[k]) for k, v in got[form].items()}
            print(f'[head bptt] {case} T {T} {vname} form {form}: ' + ', '.join(f'{k} {v:.2e}' for k, v in e.items()))
            bad = {k: (v, gates[k]) for k, v in e.items() if not v < gates[k]}
            assert not bad, (vname, form, bad)
        if len(got) == 2:                                       # fused against the launch sequence: rounding level
            e = {k: R.rel_max(got[0][k], got[1][k]) for k in got[0]}
            print(f'[head bptt] {case} T {T} {vname} fused against the sequence: ' + ', '.join(f'{k} {v:.2e}' for k, v in e.items()))
            bad = {k: (v, gates[k]) for k, v in e.items() if not v < gates[k]}
            assert not bad, (vname, bad)
        again = _run_bptt(R.BPTT_CASES[case][0], case, T, vname, P, X, ref)
        assert all(torch.equal(again[k], got[R.BPTT_CASES[case][0]][k]) for k in again), 'two runs differ'
    if 0 not in R.BPTT_CASES[case]:                             # REF.CONV_CHAN > MLP_UNITS: the fused kernel refuses, without a launch
        z = torch.zeros(8, device=DEV)
        assert lib.iodine_op_head_bptt(None, 0, _ptr_array([z] * 10 + [None] * 6), _ptr_array([z] * 5 + [None] * 2), T, N, 1, L, H, Cr, 0) == 1


def test_head_bptt_entry_refuses_carries_without_seeds():
    z = torch.zeros(64, device=DEV)
    for form in (0, 1):
        assert _lib.lib().iodine_op_head_bptt(None, form, _ptr_array([z] * 10 + [None, None, None, None, z, None]),
                                              _ptr_array([z] * 5 + [None] * 2), 1, 1, 1, 4, 4, 4, 0) == 1


@pytest.mark.parametrize('case', R.POOL_CASES, ids=str)
def test_pool_bwd(case):
    N, PL, Cc = case
    pre = R._rand(N, PL, Cc, seed=70, scale=2.0)
    dp = R._rand(N, Cc, seed=71)
    act64, ref = R.pool_bwd(pre.double(), dp.double())
    _, f32 = R.pool_bwd(pre, dp)
    gate = min(4 * R.rel_max(f32, ref), R.HEAD_GATE_CAP)
    out = _out(N, PL, Cc)
    a, dd = act64.float().to(DEV).contiguous(), dp.to(DEV).contiguous()
    _check(_lib.lib().iodine_op_pool_bwd(None, _lib.ptr(dd), _lib.ptr(a), _lib.ptr(out), N, PL, Cc), f'iodine_op_pool_bwd {case}')
    torch.cuda.synchronize()
    e = R.rel_max(_take(out, N, PL, Cc), ref)
    print(f'[pool bwd] {case}: {e:.2e} (CPU fp32 {gate / 4:.2e})')
    assert e < gate, (e, gate)
