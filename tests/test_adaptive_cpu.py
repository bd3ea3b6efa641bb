"""Host-side checks of adaptive refinement (IODINE.reconstruct_adaptive, iodine_adaptive_select / iodine_adaptive_move /
iodine_reconstruct_adaptive): the numpy definition of the stopping rule on hand-made score tables, the Python argument refusals on a
CPU-only model, and the C entries' refusals - none of which touches a device.  The device side is tests/test_gpu_adaptive.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import adaptive_reference as A
from iodine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                      # IODINE_ERR_INVALID
NEW = ('iodine_adaptive_select', 'iodine_adaptive_move', 'iodine_reconstruct_adaptive')
INF = float('inf')


def test_header_exports_and_sources():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in NEW:
        assert re.search(r'\bint ' + name + r'\(', header) and name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    for word in ('iodine_adaptive_ctl', 'iodine_move_entry', '"adaptive_select"', '"adaptive_move"', 'tests/adaptive_reference.py'):
        assert word in header, word
    src = __import__('iodine_amd.build', fromlist=['SOURCES']).SOURCES
    assert 'kernels_adaptive.hip' in src and 'iodine_adaptive.cpp' in src
    assert _lib.lib().iodine_abi_version() == 3
    import iodine_amd.adaptive as ad
    from iodine_amd import model
    assert hasattr(model.IODINE, 'reconstruct_adaptive') and ad.Adaptive and ad.select and ad.move
    assert C.sizeof(_lib.AdaptiveCtl) == 32 and C.sizeof(_lib.MoveEntry) == 56


def _table(rows):
    """scores (T, B) -> (ll, kl) with beta = 1 and kl = 0: s = ll"""
    s = np.asarray(rows, np.float32)
    return s, np.zeros_like(s)


def test_rule_first_check_never_and_min_iters():
    # three images, 6 evaluations: flat from the start / rising by 10 / rising then flat after evaluation 3
    ll, kl = _table([[5, 0, 0], [5, 10, 10], [5, 20, 20], [5, 30, 30], [5, 40, 30.5], [5, 50, 30.6]])
    it, act = A.iterations(ll, kl, 1.0, 6, min_iters=2, tol=1.0)
    assert it.tolist() == [2, 6, 5] and act == [3, 3, 2, 2, 2, 1]          # the first check is t = 2: it compares evaluations 0 and 1
    # never stopping: tol = -inf; everything stops at max_iters and every round runs the whole batch
    it, act = A.iterations(ll, kl, 1.0, 6, tol=-INF)
    assert it.tolist() == [6, 6, 6] and act == [3] * 6
    # +inf: the first permitted check, which min_iters moves; min_iters below 2 is still 2 (two evaluations are needed)
    assert A.iterations(ll, kl, 1.0, 6, min_iters=1, tol=INF)[0].tolist() == [2, 2, 2]
    assert A.iterations(ll, kl, 1.0, 6, min_iters=4, tol=INF)[0].tolist() == [4, 4, 4]
    assert A.iterations(ll, kl, 1.0, 6, min_iters=1, tol=1.0)[0].tolist() == [2, 6, 5]
    # rtol alone: 0 < 0.02 * 5 -> image 0 at the first check; 0.5 < 0.02 * 30 -> image 2 at t = 5; image 1 (gain 10 on <= 40) never
    assert A.iterations(ll, kl, 1.0, 6, tol=0.0, rtol=0.02)[0].tolist() == [2, 6, 5]
    # beta enters the score: kl rising as fast as ll makes image 1 flat at beta = 1
    it = A.iterations(ll, np.stack([np.zeros(6), 10 * np.arange(6), np.zeros(6)], 1).astype(np.float32), 1.0, 6, tol=1.0)[0]
    assert it.tolist() == [2, 2, 5]


def test_rule_check_every_skips_and_compares_the_last_two():
    ll, kl = _table([[0, 0], [0, 10], [0, 20], [0, 20.5], [0, 30], [0, 40], [0, 50], [0, 60]])
    # R = 2: decisions at t = 2, 4, 6 only; image 1 is flat between evaluations 2 and 3 -> t = 4 sees it; R = 1 sees it too
    it, act = A.iterations(ll, kl, 1.0, 8, check_every=2, tol=1.0)
    assert it.tolist() == [2, 4] and act == [2, 1, 0, 0]
    assert A.iterations(ll, kl, 1.0, 8, check_every=1, tol=1.0)[0].tolist() == [2, 4]
    # R = 3: t = 3 compares evaluations 1 and 2 (gain 10), t = 6 evaluations 4 and 5: the flat pair (2, 3) is never compared
    it, act = A.iterations(ll, kl, 1.0, 8, check_every=3, tol=1.0)
    assert it.tolist() == [3, 8] and act == [2, 1, 1]
    # odd t are skipped at R = 2 even for +inf
    assert A.iterations(ll, kl, 1.0, 8, check_every=2, min_iters=3, tol=INF)[0].tolist() == [4, 4]
    # the last round is what is left: max_iters = 8 at R = 3 ends at 8, not 9
    it, act = A.iterations(ll, kl, 1.0, 8, check_every=3, tol=-INF)
    assert it.tolist() == [8, 8] and act == [2, 2, 2]


def test_rule_budget_against_tolerance():
    ll, kl = _table([[0, 0, 0], [10, 10, 0], [20, 20, 0], [30, 30, 0], [40, 40, 0], [50, 50, 0]])
    bud = np.array([1, 5, 6])
    # the budget stops before the tolerance would (image 0 at 1, before the first score check), the tolerance before the budget (image 2)
    it, act = A.iterations(ll, kl, 1.0, 6, tol=1.0, budget=bud)
    assert it.tolist() == [1, 5, 2] and act == [3, 2, 1, 1, 1, 0]
    # budget alone, rounded up to the next multiple of R and capped at max_iters
    for R, want in ((1, [1, 5, 6]), (2, [2, 6, 6]), (3, [3, 6, 6]), (4, [4, 6, 6])):
        assert A.iterations(ll, kl, 1.0, 6, check_every=R, budget=bud)[0].tolist() == want, R


def test_rule_nan_and_inf_scores_continue():
    nan = float('nan')
    ll, kl = _table([[0, 0, 0, 0], [nan, INF, -INF, 0], [nan, INF, -INF, nan], [0, 0, 0, 0], [0, 0, 0, 0]])
    it = A.iterations(ll, kl, 1.0, 5, tol=1.0)[0]
    # image 0: NaN on one side at t = 2, 3, 4 -> continues; flat pair (3, 4) is seen at t = 5 = max_iters anyway
    # image 1: +inf - 0 is no stop; inf - inf = NaN; 0 - inf = -inf, but the right side is 1 + 0 * |inf| = NaN: no stop before max_iters
    # image 2: -inf - 0 = -inf < 1 stops at t = 2;  image 3: 0 - 0 stops at t = 2
    assert it.tolist() == [5, 5, 2, 2]
    assert A.stops([0.0, nan, 0.0, INF], [nan, 0.0, 0.0, INF], INF, 0.0).tolist() == [False, False, True, False]
    assert not A.stops([0.0], [-1e300], -INF, 0.0).any()


def test_select_and_move_in_numpy():
    ll, kl, iters = np.full((4, 5), np.nan, np.float32), np.full((4, 5), np.nan, np.float32), np.zeros(5, np.int32)
    terms = np.zeros((2, 3, 2), np.float32)
    terms[:, :, 0] = [[0, 0, 0], [0, 10, 0]]
    out = A.select(terms, np.array([4, 1, 2]), 2, 5, ll, kl, iters, 4, 2, 2, 1.0, 0.0, 1.0)
    assert [o.tolist() for o in out] == [[1], [1], [4, 2], [0, 2]] and iters.tolist() == [0, 0, 2, 0, 2]
    assert ll[1, 1] == 10 and np.isnan(ll[:, 0]).all() and np.isnan(ll[2:]).all()
    src, dst = np.arange(12.0).reshape(4, 3), np.zeros((5, 3))
    A.move([(src, dst, np.array([3, 0]), np.array([1, 4]), 2)])
    assert dst[1].tolist() == [9, 10, 11] and dst[4].tolist() == [0, 1, 2] and dst[0].tolist() == [0, 0, 0]


def _model():
    from util import golden_setup, hip_arch, load_golden
    from iodine_amd import IODINE
    arch = golden_setup(load_golden('tiny'))[0]
    return IODINE(hip_arch(arch)), arch


def test_reconstruct_adaptive_refuses_bad_arguments_without_a_device():
    m, arch = _model()
    B, K, T, L, S = 2, arch.slots, arch.iters, arch.dim_latent, arch.img_size
    x = torch.rand(B, 3, S, S)
    with pytest.raises(ValueError, match='at least one of tol, rtol'):
        m.reconstruct_adaptive(x)
    with pytest.raises(ValueError, match='at least one of tol, rtol'):
        m.reconstruct_adaptive(x, rtol=0.0)
    with pytest.raises(ValueError, match='a clip is not supported'):
        m.reconstruct_adaptive(torch.rand(B, T, 3, S, S), tol=1.0)
    with pytest.raises(ValueError, match='x must be images'):
        m.reconstruct_adaptive(torch.rand(B, 3, S, S + 1), tol=1.0)
    with pytest.raises(ValueError, match='tol must not be NaN'):
        m.reconstruct_adaptive(x, tol=float('nan'))
    with pytest.raises(ValueError, match='tol must be a real number'):
        m.reconstruct_adaptive(x, tol='1')
    for bad in (-0.1, float('nan')):
        with pytest.raises(ValueError, match='rtol must be >= 0'):
            m.reconstruct_adaptive(x, tol=1.0, rtol=bad)
    for kw in (dict(min_iters=0), dict(min_iters=T + 1), dict(max_iters=3, min_iters=4)):
        with pytest.raises(ValueError, match='min_iters must be in 1..max_iters'):
            m.reconstruct_adaptive(x, tol=1.0, **kw)
    with pytest.raises(ValueError, match='iteration count'):
        m.reconstruct_adaptive(x, tol=1.0, max_iters=0)
    for bad in (0, -2):
        with pytest.raises(ValueError, match='check_every must be >= 1'):
            m.reconstruct_adaptive(x, tol=1.0, check_every=bad)
    with pytest.raises(ValueError, match='check_every must be an integer'):
        m.reconstruct_adaptive(x, tol=1.0, check_every=1.5)
    for bad in (torch.ones(B), torch.ones(B + 1, dtype=torch.int64), torch.ones(B, 1, dtype=torch.int32), [1, 1], torch.ones(B, dtype=torch.bool)):
        with pytest.raises(ValueError, match='budget must be an integer tensor'):
            m.reconstruct_adaptive(x, budget=bad)
    for bad in ([0, 1], [1, T + 1]):
        with pytest.raises(ValueError, match='budget values must be in 1..max_iters'):
            m.reconstruct_adaptive(x, budget=torch.tensor(bad))
    for shape in ((T, B, K, L), (T + 2, B, K, L), (T + 1, B + 1, K, L), (T + 1, B, K, L + 1)):
        with pytest.raises(ValueError, match='eps must have shape'):
            m.reconstruct_adaptive(x, tol=1.0, eps=torch.zeros(shape))
    with pytest.raises(ValueError, match='eps must have shape'):
        m.reconstruct_adaptive(x, tol=1.0, max_iters=3, eps=torch.zeros(T + 1, B, K, L))
    m.K = 17
    with pytest.raises(ValueError, match='slot count'):
        m.reconstruct_adaptive(x, tol=1.0)
    m.K = K
    # well-formed arguments get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match='ROCm device'):
        m.reconstruct_adaptive(x, tol=-INF, rtol=0.5, budget=torch.tensor([1, T]), eps=torch.zeros(T + 1, B, K, L))
    assert m.posterior.mean is None and m._state is None


def test_python_wrappers_refuse_before_the_device():
    from iodine_amd import adaptive as ad
    terms, iters, ll, kl = torch.zeros(1, 3, 2), torch.zeros(4, dtype=torch.int32), torch.zeros(5, 4), torch.zeros(5, 4)
    with pytest.raises(ValueError, match='terms must be float32'):
        ad.select(terms[..., :1], 1, iters, ll, kl, tol=0.0)
    with pytest.raises(ValueError, match='ll and kl must be float32'):
        ad.select(terms, 1, iters, ll, kl[:4], tol=0.0)
    with pytest.raises(ValueError, match='iters must be a 1-D int32'):
        ad.select(terms, 1, iters.long(), ll, kl, tol=0.0)
    with pytest.raises(ValueError, match='tol must not be NaN'):
        ad.select(terms, 1, iters, ll, kl, tol=float('nan'))
    with pytest.raises(RuntimeError, match='ROCm device'):
        ad.select(terms, 1, iters, ll, kl, tol=0.0)
    a, b = torch.zeros(4, 3), torch.zeros(4, 2)
    with pytest.raises(ValueError, match='rows of one size'):
        ad.move([(a, b, None, None, 2)])
    with pytest.raises(ValueError, match='src_index must be a 1-D int32'):
        ad.move([(a, torch.zeros(4, 3), torch.zeros(2), None, 2)])
    with pytest.raises(RuntimeError, match='ROCm device'):
        ad.move([(a, torch.zeros(4, 3), None, None, 2)])


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every one of these returns IODINE_ERR_INVALID before a launch, with the argument named: the pointers are never dereferenced on the
    host, so dummy non-null addresses stand in for device memory."""
    L = _lib.lib()
    p, q, null, st = C.c_void_p(4096), C.c_void_p(8192), None, C.c_void_p(0)
    err = lambda: L.iodine_last_error(None).decode()

    def ctl(max_iters=8, min_iters=2, check_every=1, tol=0.0, rtol=0.0):
        return C.byref(_lib.AdaptiveCtl(max_iters, min_iters, check_every, tol, rtol))

    def select(terms=p, idx_in=null, n=4, rounds=1, t=1, batch=4, c=None, beta=1.0, budget=null, idx_out=q, pos=p, sidx=p, spos=p, counts=p,
               iters=p, ll=p, kl=p):
        return L.iodine_adaptive_select(st, terms, idx_in, n, rounds, t, batch, c if c is not None else ctl(), beta, budget, idx_out, pos, sidx,
                                        spos, counts, iters, ll, kl)
    cases = [(dict(terms=null), 'terms is NULL'), (dict(idx_out=null), 'idx_out is NULL'), (dict(pos=null), 'pos_out is NULL'),
             (dict(sidx=null), 'stop_idx is NULL'), (dict(spos=null), 'stop_pos is NULL'), (dict(counts=null), 'counts is NULL'),
             (dict(iters=null), 'iters is NULL'), (dict(ll=null), 'll is NULL'), (dict(kl=null), 'kl is NULL'), (dict(n=0), 'n must be >= 1'),
             (dict(n=-3), 'n must be >= 1'), (dict(n=5), 'n must be <= batch'), (dict(rounds=0), 'rounds'), (dict(rounds=2, t=1), 'rounds'),
             (dict(t=9), 't must be <= max_iters'), (dict(beta=float('nan')), 'beta'), (dict(idx_in=q), 'idx_out must not be idx_in'),
             (dict(c=ctl(max_iters=0)), 'max_iters'), (dict(c=ctl(min_iters=0)), 'min_iters'), (dict(c=ctl(min_iters=9)), 'min_iters'),
             (dict(c=ctl(check_every=0)), 'check_every'), (dict(c=ctl(tol=float('nan'))), 'tol is NaN'), (dict(c=ctl(rtol=-1.0)), 'rtol'),
             (dict(c=ctl(rtol=float('nan'))), 'rtol')]
    for kw, word in cases:
        assert select(**kw) == INVALID, kw
        assert err().startswith('iodine_adaptive_select: ') and word in err(), (kw, err())
    assert L.iodine_adaptive_select(st, p, null, 4, 1, 1, 4, None, 1.0, null, q, p, p, p, p, p, p, p) == INVALID and 'ctl is NULL' in err()

    def move(n=1, **kw):
        f = dict(src=4096, dst=1 << 20, row_floats=8, src_index=None, dst_index=None, rows=4, src_rows=0, dst_rows=0)
        f.update(kw)
        e = _lib.MoveEntry(**f)
        return L.iodine_adaptive_move(st, C.byref(e), n)
    cases = [(dict(src=None), 'src is NULL'), (dict(dst=None), 'dst is NULL'), (dict(row_floats=0), 'row_floats'), (dict(rows=0), 'rows must be >= 1'),
             (dict(src_rows=3), 'src_rows'), (dict(dst_rows=2), 'dst_rows'), (dict(n=0), 'n_entries'), (dict(n=17), 'n_entries'),
             # aliasing rows: the same array, a destination inside the source, a source whose indexed extent reaches the destination
             (dict(dst=4096), 'overlap'), (dict(dst=4096 + 4 * 8 * 3), 'overlap'), (dict(src=(1 << 20) - 4 * 8 * 4 + 4), 'overlap'),
             (dict(src=(1 << 20) - 4 * 8 * 100, src_index=64, src_rows=101), 'overlap')]
    for kw, word in cases:
        assert move(**kw) == INVALID, kw
        assert err().startswith('iodine_adaptive_move: ') and word in err(), (kw, err())
    assert L.iodine_adaptive_move(st, None, 1) == INVALID and 'table is NULL' in err()

    # the handle entry: a null handle; on a handle (host-side create would need a device: none here) nothing more can be asked without one
    args = (st, 2, p, p, ctl(), null, None, p, p, p, p, p, p, p, p, p, p, p, None)
    assert L.iodine_reconstruct_adaptive(None, *args) == INVALID
