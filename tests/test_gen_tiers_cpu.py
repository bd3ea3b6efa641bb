"""The kernel-level tests of the generic stride-1 convs and broadcast layer (test_gpu_gen_s1.py, test_gpu_gen_l0.py): what can be checked
without a GPU.  iodine_op_gen_conv_tier is the selector the launchers of kernels_generic.hip switch on (host arithmetic): the case table
of the GPU tests must reach every kernel it can choose at stride 1 - in every direction, with all four NP instantiations of the output
conv's weight gradient - and every case must sit on the tier it declares, so that a changed LDS budget shows up HERE, not as a kernel
that silently lost its test."""
import ctypes
import os
import re

import pytest

import test_gpu_gen_l0 as l0
import test_gpu_gen_s1 as s1
from iodine_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
T = s1.TIER


def _all_stride1_cases():
    """(ci, ldc, co, k, S) of everything test_gpu_gen_s1.py runs at stride 1 (the tile-loop cases at their fixed size)"""
    return [c[:5] for c in s1.CASES] + [(ci, ci, co, k, 40) for ci, co, k, _ in s1.TILE_LOOP]


@pytest.mark.parametrize('case', s1.CASES, ids=s1._id)
def test_every_case_sits_on_the_tier_it_declares(case):
    ci, ldc, co, k, S, N, t_f, t_d, t_w, np_ = case
    assert s1.tier_of(0, S, ci, ldc, co, k) == (T[t_f], 0)
    assert s1.tier_of(1, S, ci, ldc, co, k) == (T[t_d], 0)
    assert s1.tier_of(2, S, ci, ldc, co, k) == (T[t_w], np_)
    assert N * S * S * max(ldc, co) < 8 << 20                   # (the largest tensor of a test stays below 8 M floats)


def test_the_cases_reach_every_tier_of_stride_1():
    hit = {0: set(), 1: set(), 2: set()}
    for ci, ldc, co, k, S in _all_stride1_cases():
        for mode in range(3):
            hit[mode].add(s1.tier_of(mode, S, ci, ldc, co, k))
    # forward / data gradient: the MFMA kernel at its three chunk widths and the scalar kernels (S2_MFMA is stride 2's)
    for mode in (0, 1):
        assert {t for t, _ in hit[mode]} == {T['cch16'], T['cch8'], T['cch4'], T['scalar']}, (mode, hit[mode])
    # weight gradient: kernel sizes 3 / 5 / 7 at stride 1 never take the scalar form - GEMM form at NP 1 / 2 / 4 / 8, rows, per-tap MFMA
    assert hit[2] == {(T['out'], 1), (T['out'], 2), (T['out'], 4), (T['out'], 8), (T['rows'], 0), (T['wmfma'], 0)}, hit[2]
    assert {c[8] for c in s1.ACCUMULATE} == {'out', 'rows', 'wmfma'}        # one accumulating call per weight-gradient form


def test_long_sums_are_split_and_every_split_kernel_is_reached():
    """forward / data gradient: an output is one fp32 fmaf chain up to 1600 products (5 x 5 x 64 channels), beyond that segments of about
    800 - the MFMA kernel has a second instantiation for it per (kernel size, chunk width) the LDS budget lets a long sum reach"""
    hit = set()
    for ci, ldc, co, k, S in _all_stride1_cases():
        for mode in (0, 1):
            products, seg = (ci if mode == 0 else co) * k * k, s1.segment_of(mode, S, ci, ldc, co, k)
            assert (seg > 0) == (products > 1600), (mode, ci, co, k, seg)
            if seg:
                tier = s1.tier_of(mode, S, ci, ldc, co, k)[0]
                per = {T['cch16']: 16 * k * k, T['cch8']: 8 * k * k, T['cch4']: 4 * k * k, T['scalar']: 1}[tier]
                assert 400 <= seg * per <= 1000, (mode, ci, co, k, seg)     # products per segment
                hit.add((mode, tier, k))
        assert s1.segment_of(2, S, ci, ldc, co, k) == 0
    want = {(T['cch16'], 3), (T['cch8'], 3), (T['cch4'], 3), (T['cch8'], 5), (T['cch4'], 5), (T['cch4'], 7), (T['scalar'], 5), (T['scalar'], 7)}
    for mode in (0, 1):
        assert {(t, k) for m, t, k in hit if m == mode} == want, (mode, hit)


def test_strides_other_than_1_and_argument_checks():
    for ci, ldc, co, k, S, N, s in s1.STRIDED:
        for mode in range(3):
            assert s1.tier_of(mode, S, ci, ldc, co, k, s) == (T['scalar'], 0)
    for s in (3, 4):                                            # per stride: a last output column whose window the edge cuts, and an
        sizes = [(c[4], c[3]) for c in s1.STRIDED if c[6] == s] # image whose last pixel is not a window centre
        assert any(((S - 1) // s) * s + k // 2 >= S for S, k in sizes) and any((S - 1) % s != 0 for S, _ in sizes), sizes
    # stride 2 keeps its own kernels (test_gpu_gen_s2.py's first case), whatever the selector was refactored into
    for mode in range(3):
        assert s1.tier_of(mode, 64, 32, 32, 32, 5, 2) == (T['s2'], 0)
    L = _lib.lib()
    for bad in ((3, 16, 8, 8, 8, 3, 1), (0, 16, 8, 8, 8, 4, 1), (0, 16, 8, 8, 8, 3, 0), (0, 16, 8, 8, 8, 3, 9), (0, 16, 8, 4, 8, 3, 1)):
        assert L.iodine_op_gen_conv_tier(*bad) == -1, bad


def test_tile_loop_batches_give_unequal_tile_counts():
    for ci, co, k, per_cu in s1.TILE_LOOP:
        for n_cu in (256, 304, 64):                             # MI355X, MI300X, a partition
            N, nb = s1.tile_loop_batch(ci, co, per_cu, n_cu)
            assert N <= 256 and 9 * N >= 2 * nb + 1 and (9 * N) % nb != 0, (ci, n_cu, N, nb)
            assert N * 40 * 40 * max(ci, co) < 8 << 20


def test_broadcast_layer_cases():
    assert all(co % 4 == 0 for _, co, _, _, _ in l0.CASES)      # DEC.CONV_CHAN is a multiple of 4: the V = 4 forward
    assert any(S == k + 1 for _, _, k, S, _ in l0.CASES) and {k for _, _, k, _, _ in l0.CASES} == {3, 5, 7}
    assert all(N * S * S * co < 8 << 20 for _, co, _, S, N in l0.CASES)
    assert set(l0.STRUCTURED) <= set(l0.CASES)


def test_header_states_the_strides_the_entry_point_takes():
    assert 'stride s in 1..8' in HEADER
    assert 'stride s in {1, 2}' not in HEADER and 'takes the two it is tested at' not in HEADER    # the stale sentence


@pytest.mark.parametrize('name', ['iodine_op_gen_conv_tier', 'iodine_op_gen_l0'])
def test_entry_points_are_declared_listed_and_exported(name):
    assert re.search(r'\bint\s+' + name + r'\s*\(', HEADER)
    assert name in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(build.LIB), name)
