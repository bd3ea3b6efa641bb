"""Host-side checks of the matched-mask feature (iodine_amd.matching, iodine_mask_overlap / iodine_assign / iodine_assign_host /
iodine_mask_match / iodine_mask_match_backward): the exports, the argument checks the entry points make before they touch a device, the
host entry of the assignment solver - the function the device kernel runs - against a brute force and against scipy, its refusal of
non-finite costs, the Python layer's refusals, pack_gt, the score arithmetic on hand numbers and the engine's guard.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import match_reference as R
from iodine_amd import _lib, matching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                      # IODINE_ERR_INVALID
ENTRIES = ('iodine_mask_overlap', 'iodine_assign', 'iodine_assign_host', 'iodine_mask_match', 'iodine_mask_match_backward')


def host_assign(cost, valid=None):
    """iodine_assign_host on one (G, K) matrix -> (assign list, total float32)"""
    c = np.ascontiguousarray(cost, dtype=np.float32)
    G, K = c.shape
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    a = np.full(G, -7, dtype=np.int32)
    t = np.full(1, -7.0, dtype=np.float32)
    rc = _lib.lib().iodine_assign_host(c.ctypes.data_as(C.c_void_p), None if v is None else v.ctypes.data_as(C.c_void_p), G, K,
                                       a.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return a.tolist(), t[0]


def check_map(a, total, cost, valid):
    """injective, exactly min(|R|, K) real rows matched, padding rows -1, the matched costs sum to the total"""
    G, K = cost.shape
    real = [g for g in range(G) if valid is None or valid[g]]
    got = [g for g in range(G) if a[g] >= 0]
    assert all(g in real for g in got) and all(0 <= a[g] < K for g in got)
    assert len({a[g] for g in got}) == len(got) == min(len(real), K)
    assert float(total) == float(np.float32(sum(float(cost[g, a[g]]) for g in got)))


def test_exports_and_header():
    import iodine_amd
    for name in ('pack_gt', 'overlap', 'assign', 'match_masks', 'matched_mask_loss', 'segmentation_scores', 'SegmentationEvaluator'):
        assert getattr(iodine_amd, name) is getattr(matching, name) and name in iodine_amd.__all__
    assert 'matching' in iodine_amd.__all__
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(L, name) and f'int {name}(' in header, name
    from iodine_amd import build
    assert 'kernels_match.hip' in build.SOURCES
    assert L.iodine_abi_version() == 3


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every one of these returns IODINE_ERR_INVALID before a launch: the pointers are never dereferenced, so dummy non-null addresses
    stand in for device (and, in the host entry, host) memory."""
    L = _lib.lib()
    p, null, st = C.c_void_p(4096), None, C.c_void_p(0)
    last = lambda: L.iodine_last_error(None)

    def overlap(mask=p, gt=p, batch=1, slots=2, n_gt=2, size=8, eps=1e-6, inter=p, nll=p, area=p, n=p):
        return L.iodine_mask_overlap(st, mask, gt, batch, slots, n_gt, size, eps, inter, nll, area, n)
    for kw in (dict(mask=null), dict(gt=null), dict(inter=null), dict(area=null), dict(n=null), dict(batch=0), dict(slots=0), dict(slots=17),
               dict(n_gt=0), dict(n_gt=17), dict(size=0), dict(size=1025), dict(eps=0.0), dict(eps=-1e-6), dict(eps=float('nan'))):
        assert overlap(**kw) == INVALID, kw
    assert b'iodine_mask_overlap' in last()

    def assign(cost=p, valid=null, batch=1, rows=2, cols=2, a=p, t=p):
        return L.iodine_assign(st, cost, valid, batch, rows, cols, a, t)
    for kw in (dict(cost=null), dict(a=null), dict(t=null), dict(batch=0), dict(rows=0), dict(rows=17), dict(cols=0), dict(cols=17)):
        assert assign(**kw) == INVALID, kw
    assert b'iodine_assign:' in last()

    def assign_host(cost=p, valid=null, rows=2, cols=2, a=p, t=p):
        return L.iodine_assign_host(cost, valid, rows, cols, a, t)
    for kw in (dict(cost=null), dict(a=null), dict(t=null), dict(rows=0), dict(rows=17), dict(cols=-1), dict(cols=17)):
        assert assign_host(**kw) == INVALID, kw
    assert b'iodine_assign_host' in last()

    def match(inter=p, nll=p, area=p, n=p, batch=1, slots=2, n_gt=2, mk=0, lk=1, a=p, loss=p, coef=p):
        return L.iodine_mask_match(st, inter, nll, area, n, batch, slots, n_gt, mk, lk, a, loss, coef, null, null)
    for kw in (dict(inter=null), dict(area=null), dict(n=null), dict(a=null), dict(loss=null), dict(coef=null), dict(batch=0), dict(slots=0),
               dict(slots=17), dict(n_gt=0), dict(n_gt=17), dict(mk=2), dict(lk=-1), dict(nll=null, mk=0, lk=1), dict(nll=null, mk=1, lk=0)):
        assert match(**kw) == INVALID, kw
    assert b'iodine_mask_match:' in last()

    def backward(mask=p, gt=p, a=p, coef=p, gl=p, batch=1, slots=2, n_gt=2, size=8, lk=1, eps=1e-6, grad=p):
        return L.iodine_mask_match_backward(st, mask, gt, a, coef, gl, batch, slots, n_gt, size, lk, eps, grad)
    for kw in (dict(mask=null), dict(gt=null), dict(a=null), dict(coef=null), dict(gl=null), dict(grad=null), dict(batch=0), dict(slots=17),
               dict(n_gt=0), dict(size=0), dict(size=1025), dict(lk=2), dict(eps=0.0)):
        assert backward(**kw) == INVALID, kw
    assert b'iodine_mask_match_backward' in last()


VALID_PATTERNS = {1: [None, [0]], 2: [None, [0, 1], [0, 0]], 3: [None, [1, 0, 1], [0, 0, 1]], 4: [None, [1, 0, 0, 1], [0, 1, 1, 1]],
                  5: [None, [1, 0, 1, 0, 1], [0, 1, 1, 1, 1], [0, 0, 0, 0, 0]]}


@pytest.mark.parametrize('G', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('K', [1, 2, 3, 4, 5])
def test_host_solver_matches_brute_force(G, K):
    """Small-integer costs are exact in fp32 and in every sum the solver forms, so the totals are compared with ==.  The row-valid patterns
    put padding in the middle and cover |R| > K and |R| = 0."""
    rng = np.random.default_rng(100 * G + K)
    for trial in range(12):
        cost = rng.integers(-9, 10, size=(G, K)).astype(np.float32)
        if trial % 3 == 0:
            cost = rng.integers(0, 3, size=(G, K)).astype(np.float32)       # many ties
        for valid in VALID_PATTERNS[G]:
            a, total = host_assign(cost, valid)
            check_map(a, total, cost, valid)
            ref_a, ref_total, _ = R.brute_force(cost, valid) if (valid is None or any(valid)) else ([-1] * G, 0.0, 0.0)
            assert float(total) == ref_total, (cost, valid, a, ref_a)
            assert host_assign(cost, valid)[0] == a                          # the same input gives the same map


@pytest.mark.parametrize('shape', [(16, 16), (16, 7), (7, 16)])
def test_host_solver_matches_scipy_at_full_size(shape):
    lsa = pytest.importorskip('scipy.optimize').linear_sum_assignment
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    for trial in range(20):
        cost = rng.integers(-50, 51, size=shape).astype(np.float32)
        a, total = host_assign(cost)
        check_map(a, total, cost, None)
        r, c = lsa(cost.astype(np.float64))
        assert float(total) == float(cost[r, c].sum())
    valid = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1][:shape[0]], dtype=np.uint8)
    cost = rng.integers(0, 100, size=shape).astype(np.float32)
    a, total = host_assign(cost, valid)
    check_map(a, total, cost, valid)
    rows = np.flatnonzero(valid)
    r, c = lsa(cost[rows].astype(np.float64))
    assert float(total) == float(cost[rows][r, c].sum())


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_host_solver_refuses_non_finite_costs(bad):
    """A non-finite cost in a real row: all -1, a NaN total, and the call returns.  In a padding row it is never read."""
    for G, K, pos in ((1, 1, (0, 0)), (3, 4, (1, 2)), (5, 2, (4, 0)), (16, 16, (7, 9))):
        cost = np.arange(G * K, dtype=np.float32).reshape(G, K)
        cost[pos] = bad
        a, total = host_assign(cost)
        assert a == [-1] * G and np.isnan(total)
        if G > 1:
            valid = np.ones(G, dtype=np.uint8)
            valid[pos[0]] = 0
            a, total = host_assign(cost, valid)
            assert np.isfinite(total) and a[pos[0]] == -1
            check_map(a, total, np.where(np.isfinite(cost), cost, 0).astype(np.float32), valid)
    a, total = host_assign(np.full((4, 4), bad, dtype=np.float32))
    assert a == [-1] * 4 and np.isnan(total)


def test_python_layer_refuses_cpu_tensors_and_wrong_shapes():
    mask, gt = torch.rand(2, 3, 1, 8, 8), torch.zeros(2, 2, 8, 8, dtype=torch.uint8)
    for fn in (matching.overlap, matching.match_masks, matching.matched_mask_loss, matching.segmentation_scores):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(mask, gt)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        matching.assign(torch.zeros(2, 3, 3))
    with pytest.raises(ValueError, match='torch tensors'):
        matching.overlap(mask.numpy(), gt)
    with pytest.raises(ValueError, match="'iou' or 'ce'"):
        matching.matched_mask_loss(mask, gt, loss='dice')
    with pytest.raises(ValueError, match="'iou' or 'ce'"):
        matching.match_masks(mask, gt, cost='l2')
    with pytest.raises(ValueError, match='reduction'):
        matching.matched_mask_loss(mask, gt, reduction='sum')
    with pytest.raises(ValueError, match='torch tensor'):
        matching.assign([[0.0]])
    with pytest.raises(ValueError, match='eps must be > 0'):
        matching._eps(0.0, 'overlap')


def test_python_layer_shape_checks_on_device_tensors(monkeypatch):
    """_check_pair's ValueErrors, reached with the device test stubbed out (the checks themselves need no device)"""
    class Dev:
        type = 'cuda'

        def __eq__(self, other):
            return True

        def __ne__(self, other):
            return False

    def fake(t):
        class T(torch.Tensor):
            device = Dev()
        return t.as_subclass(T)
    mask, gt = fake(torch.rand(2, 3, 1, 8, 8)), fake(torch.zeros(2, 2, 8, 8, dtype=torch.uint8))
    assert matching._check_pair(mask, gt, 't') == ((2,), 2, 3, 2, 8)
    assert matching._check_pair(fake(torch.rand(4, 2, 3, 1, 8, 8)), fake(torch.zeros(4, 2, 5, 8, 8, dtype=torch.uint8)), 't') == ((4, 2), 8, 3, 5, 8)
    for m, g, word in ((fake(torch.rand(2, 3, 8, 8)), gt, 'mask must be'), (fake(torch.rand(2, 3, 1, 8, 4)), gt, 'mask must be'),
                       (fake(torch.rand(2, 3, 1, 8, 8).double()), gt, 'float32'), (mask, fake(torch.zeros(2, 2, 8, 8)), 'uint8'),
                       (mask, fake(torch.zeros(3, 2, 8, 8, dtype=torch.uint8)), 'gt must be'),
                       (mask, fake(torch.zeros(2, 2, 4, 4, dtype=torch.uint8)), 'gt must be'),
                       (mask, fake(torch.zeros(2, 17, 8, 8, dtype=torch.uint8)), '1..16'),
                       (fake(torch.rand(2, 17, 1, 8, 8)), gt, '1..16')):
        with pytest.raises(ValueError, match=word):
            matching._check_pair(m, g, 't')


def test_pack_gt_on_ragged_none_and_empty_inputs():
    S = 4
    a = np.zeros((2, S, S), dtype=np.float32)
    a[0, :2], a[1, 2:] = 1.0, 3.0                                            # non-zero counts as inside
    b = torch.zeros(3, S, S)
    b[2, 1, 1] = 1.0
    packed = matching.pack_gt((a, None, b, np.zeros((0, S, S), dtype=np.uint8)))
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (4, 3, S, S) and packed.device.type == 'cpu'
    assert torch.equal(packed[0, :2], torch.from_numpy((a != 0).astype(np.uint8))) and not packed[0, 2].any()
    assert not packed[1].any() and not packed[3].any()
    assert torch.equal(packed[2], b.to(torch.uint8)) and int(packed.max()) == 1
    none = matching.pack_gt((None, None), size=S)
    assert tuple(none.shape) == (2, 1, S, S) and not none.any()
    with pytest.raises(ValueError, match='image size'):
        matching.pack_gt((None, None))
    with pytest.raises(ValueError, match='image size'):
        matching.pack_gt((a, np.zeros((1, 5, 5))))
    with pytest.raises(ValueError, match=r'\(N, S, S\)'):
        matching.pack_gt((np.zeros((S, S)),))
    with pytest.raises(ValueError, match='at most 16'):
        matching.pack_gt((np.zeros((17, S, S)),))
    through = matching.pack_gt(packed)
    assert through is packed
    assert matching.pack_gt(packed.float() * 2).dtype == torch.uint8 and torch.equal(matching.pack_gt(packed.float() * 2), packed)
    with pytest.raises(ValueError, match=r'\(B, G, S, S\)'):
        matching.pack_gt(torch.zeros(3, S, S))


def test_score_arithmetic_on_hand_numbers(monkeypatch):
    """Two objects, three slots, 16 pixels.  Object 0 (n = 6): 4 pixels in slot 0, 2 in slot 1.  Object 1 (n = 4): 1 in slot 0, 3 in slot 1.
    Background (6 pixels): 1 in slot 0, 5 in slot 2.  Hard areas: slot 0 = 6, slot 1 = 5, slot 2 = 5.
    IoU_00 = 4 / (6 + 6 - 4) = 1/2, IoU_01 = 2 / (6 + 5 - 2) = 2/9, IoU_10 = 1 / (4 + 6 - 1) = 1/9, IoU_11 = 3 / (4 + 5 - 3) = 1/2,
    column 2 is 0.  Best matching: 0 -> 0, 1 -> 1: mIoU = (1/2 + 1/2) / 2 = 1/2; max_k the same: mSC = 1/2, SC = (6 / 2 + 4 / 2) / 10 = 1/2.
    A third, empty row and an image without objects: the first changes nothing, the second scores NaN.  The assignment - the one device
    step - is served by the host entry of the same solver here."""
    def host(cost, row_valid=None):
        c, v = cost.numpy(), row_valid.numpy()
        out = [host_assign(c[b], v[b]) for b in range(c.shape[0])]
        return torch.tensor([o[0] for o in out], dtype=torch.int32), torch.tensor([float(o[1]) for o in out])
    monkeypatch.setattr(matching, 'assign', host)
    T = np.array([[[4, 2, 0], [0, 0, 0], [1, 3, 0]], [[0, 0, 0]] * 3], dtype=np.int64)
    h = np.array([[6, 5, 5], [16, 0, 0]], dtype=np.float64)
    s = matching.scores_from_tables(T, h, 'cpu')
    assert s.miou[0] == 0.5 and s.msc[0] == 0.5 and s.sc[0] == 0.5
    assert all(np.isnan(v[1]) for v in s)
    # one object covered by two slots, the other missed: object 0 (n = 8) is 4 + 4 in slots 0 / 1 of area 4 each, object 1 (n = 2) sits in
    # slot 2 (area 4) with 2 background pixels... IoU_00 = IoU_01 = 4 / 8, IoU_12 = 2 / 4, everything else 0
    T = np.array([[[4, 4, 0], [0, 0, 2]]], dtype=np.int64)
    h = np.array([[4, 4, 4]], dtype=np.float64)
    s = matching.scores_from_tables(T, h, 'cpu')
    assert s.miou[0] == 0.5 and s.msc[0] == 0.5 and s.sc[0] == (8 * 0.5 + 2 * 0.5) / 10
    ev = matching.SegmentationEvaluator()
    assert ev.per_image == ('aris', 'mious', 'scs', 'mscs') and ev.mious == [] and 'mIoU' in ev.get_results()
    ev.mious = [0.25, float('nan'), 0.75]
    assert 'mIoU: 0.5' in ev.get_results()


def test_reference_gaps_of_the_planted_inputs():
    """The GPU tests compare assignments on planted inputs only: their best and second-best totals are far apart (the reference side of
    the gap assertion those tests make again on their own inputs)."""
    for K, G in ((5, 4), (3, 5), (5, 5), (4, 1)):
        mask, gt = R.planted(2, K, G, 16, seed=K * 10 + G)
        st = R.stats(mask, gt)
        for kind in R.KINDS:
            cost = R.pair_values(kind, *st)
            for b in range(2):
                valid = [bool(v) for v in (st[3][b] > 0)]
                _, _, gap = R.brute_force(cost[b].numpy(), valid)
                assert gap >= 1e-3, (K, G, kind, b, gap)


def test_engine_refuses_mask_loss_with_bptt():
    from iodine_amd import engine
    with pytest.raises(ValueError, match='mask_loss is not combined with bptt'):
        engine.train(None, None, [], 'cpu', 1, bptt='truncated', mask_loss=1.0)
    with pytest.raises(ValueError, match="'iou' or 'ce'"):
        engine.train(None, None, [], 'cpu', 1, mask_loss=1.0, mask_loss_kind='dice')
    with pytest.raises(ValueError, match='mask_loss must be >= 0'):
        engine.train(None, None, [], 'cpu', 1, mask_loss=-1.0)
    args = engine.make_parser().parse_args(['--mask-loss', '0.5', '--mask-loss-kind', 'iou', '--mask-match', 'ce', '--metrics'])
    assert (args.mask_loss, args.mask_loss_kind, args.mask_match, args.metrics) == (0.5, 'iou', 'ce', True)
    assert engine.make_parser().parse_args([]).mask_loss == 0.0
