"""iodine_slot_table / iodine_seg_overlap and reconstruct(objects=True) on the device against the float64 restatement in
objects_reference.py.

Tolerances (from the arithmetic the header promises, not from what the kernel gives):
  seg, hard_area, the box, peak     exact (integers / a maximum of the inputs)
  hard_cx, hard_cy                  2^-23 relative: one rounding of an exact integer quotient formed in double to fp32
  soft_area                         2e-5 relative: all summands are >= 0, so any order with fp32 chains of at most 256 terms has a relative
                                    error of at most 257 * 2^-24 = 1.5e-5
  soft_cx, soft_cy, r, g, b         4e-5 relative: ratios of two such sums (the numerators are sums of non-negative terms as well)
"""
import functools

import numpy as np
import pytest
import torch

import objects_reference as R
from iodine_amd import objects
from iodine_amd.ari import ari_tables, compute_ari
from util import golden_setup, load_golden, make_hip_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
COL = {n: i for i, n in enumerate(R.COLUMNS)}
EXACT = [COL[n] for n in ('hard_area', 'x0', 'y0', 'x1', 'y1', 'peak')]
SHAPES = [(1, 1, 8), (3, 2, 8), (2, 7, 16), (2, 5, 23), (2, 16, 24), (2, 7, 64), (2, 7, 128), (1, 2, 1024)]


def _inputs(B, K, S, seed):
    g = torch.Generator().manual_seed(seed)
    mask = torch.softmax(4.0 * torch.randn(B, K, 1, S, S, generator=g), dim=1)
    mean = torch.sigmoid(torch.randn(B, K, 3, S, S, generator=g))
    return mask, mean


@functools.lru_cache(maxsize=None)
def _case(B, K, S):
    """inputs, float64 reference and the device result of one shape, computed once and shared (treated as read-only)"""
    mask, mean = _inputs(B, K, S, seed=1000 + 97 * B + 13 * K + S)
    ref_t, ref_seg = R.slot_table(mask, mean)
    md, cd = mask.to(DEV), mean.to(DEV)
    table, seg = objects.slot_table(md, cd, segmentation=True)
    return md, cd, ref_t, ref_seg, table, seg


def _check_table(got, ref, what=''):
    """got: float32 table from the device (any leading dims), ref: float64 reference of the same shape"""
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape
    err = lambda c: float(((got[..., c] - ref[..., c]).abs() / ref[..., c].abs().clamp_min(1e-300)).max())
    figures = {R.COLUMNS[c]: err(c) for c in range(14) if c not in EXACT}
    print(what, {k: f'{v:.2e}' for k, v in figures.items()})
    for c in EXACT:
        assert torch.equal(got[..., c], ref[..., c].to(torch.float32).to(torch.float64)), (what, R.COLUMNS[c])
    for n in ('hard_cx', 'hard_cy'):
        assert figures[n] <= 2.0 ** -23, (what, n, figures[n])
    assert figures['soft_area'] <= 2e-5, (what, figures['soft_area'])
    for n in ('soft_cx', 'soft_cy', 'r', 'g', 'b'):
        assert figures[n] <= 4e-5, (what, n, figures[n])


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-K%d-S%d' % s)
def test_slot_table_matches_float64_reference(shape):
    B, K, S = shape
    md, cd, ref_t, ref_seg, table, seg = _case(*shape)
    assert table.shape == (B, K, 14) and table.dtype == torch.float32 and table.device.type == 'cuda'
    assert seg.shape == (B, S, S) and seg.dtype == torch.uint8
    assert torch.equal(seg.cpu(), ref_seg)
    _check_table(table, ref_t, str(shape))
    assert int(ref_t[..., 1].sum()) == B * S * S                              # every pixel belongs to exactly one slot


@pytest.mark.parametrize('shape', [(2, 5, 23), (2, 7, 128), (1, 2, 1024)], ids=lambda s: 'B%d-K%d-S%d' % s)
def test_two_calls_are_bitwise_equal(shape):
    md, cd, _, _, table, seg = _case(*shape)
    t2, s2 = objects.slot_table(md, cd, segmentation=True)
    assert torch.equal(t2.view(torch.int32), table.view(torch.int32)) and torch.equal(s2, seg)
    assert torch.equal(objects.slot_table(md, cd).view(torch.int32), table.view(torch.int32))      # without the map: the same table


def test_side_stream_gives_the_same_bits():
    """the launch follows the caller's current stream: B = 2, K = 3, S = 16 on a side stream against the default stream"""
    mask, mean = _inputs(2, 3, 16, seed=7)
    md, cd = mask.to(DEV), mean.to(DEV)
    table, seg = objects.slot_table(md, cd, segmentation=True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        t2, s2 = objects.slot_table(md, cd, segmentation=True)
    side.synchronize()
    assert torch.equal(t2.view(torch.int32), table.view(torch.int32)) and torch.equal(s2, seg)


def test_leading_dimensions_and_mean_none():
    """(T+1, B, ...) inputs give (T+1, B, K, 14); without mean the colour columns are 0 and every other column keeps its bits"""
    md, cd, _, _, table, seg = _case(2, 7, 16)
    m2, c2 = torch.stack([md, md.flip(0)]), torch.stack([cd, cd.flip(0)])
    t2, s2 = objects.slot_table(m2, c2, segmentation=True)
    assert t2.shape == (2, 2, 7, 14) and s2.shape == (2, 2, 16, 16)
    assert torch.equal(t2[0], table) and torch.equal(t2[1], table.flip(0)) and torch.equal(s2[0], seg) and torch.equal(s2[1], seg.flip(0))
    plain = objects.slot_table(md)
    keep = [c for c in range(14) if c not in (10, 11, 12)]
    assert float(plain[..., 10:13].abs().max()) == 0.0
    assert torch.equal(plain[..., keep].view(torch.int32), table[..., keep].view(torch.int32))
    with pytest.raises(ValueError, match='mask must be'):
        objects.slot_table(md[:, :, 0])
    with pytest.raises(ValueError, match='mean must be'):
        objects.slot_table(md, cd[:, :3])
    with pytest.raises(ValueError, match='K must be'):
        objects.slot_table(torch.zeros(1, 17, 1, 8, 8, device=DEV))


def test_edge_inputs():
    S, K = 16, 4
    mean = _inputs(1, K, S, seed=5)[1]
    # all slots equal: every pixel goes to slot 0
    flat = torch.full((1, K, 1, S, S), 1.0 / K)
    t, seg = objects.slot_table(flat.to(DEV), mean.to(DEV), segmentation=True)
    t = t.cpu()
    assert int(seg.max()) == 0 and t[0, :, 1].tolist() == [float(S * S), 0.0, 0.0, 0.0]
    assert torch.equal(t[0, 1:, 4:10], torch.full((3, 6), -1.0)) and t[0, 0, 6:10].tolist() == [0.0, 0.0, 15.0, 15.0]
    _check_table(t, R.slot_table(flat, mean)[0], 'flat')
    # one-hot, slot 3 identically 0
    hot = torch.zeros(1, K, 1, S, S)
    hot[0, 0, 0, :, :8], hot[0, 1, 0, :5, 8:], hot[0, 2, 0, 5:, 8:] = 1.0, 1.0, 1.0
    t, seg = objects.slot_table(hot.to(DEV), mean.to(DEV), segmentation=True)
    t = t.cpu()
    ref_t, ref_seg = R.slot_table(hot, mean)
    assert torch.equal(seg.cpu(), ref_seg)
    assert t[0, 3, [0, 1, 2, 3, 10, 11, 12]].tolist() == [0.0] * 7 and t[0, 3, 4:10].tolist() == [-1.0] * 6
    assert t[0, 1, 6:10].tolist() == [8.0, 0.0, 15.0, 4.0] and t[0, 2, 6:10].tolist() == [8.0, 5.0, 15.0, 15.0]
    _check_table(t, ref_t, 'one-hot')
    # a single hard pixel in a corner: the box is that pixel
    for (y, x) in ((15, 15), (0, 0), (0, 15)):
        one = torch.zeros(1, 2, 1, S, S)
        one[0, 0] = 0.75
        one[0, 1] = 0.25
        one[0, 0, 0, y, x], one[0, 1, 0, y, x] = 0.25, 0.75
        t = objects.slot_table(one.to(DEV)).cpu()
        assert t[0, 1, 1] == 1.0 and t[0, 1, 4:10].tolist() == [float(x), float(y), float(x), float(y), float(x), float(y)]
        assert t[0, 0, 1] == S * S - 1 and t[0, 0, 6:10].tolist() == [0.0, 0.0, 15.0, 15.0]
        _check_table(t, R.slot_table(one)[0], f'corner {y},{x}')


@pytest.mark.parametrize('shape', [(2, 7, 5, 23), (1, 16, 16, 64)], ids=lambda s: 'B%d-ka%d-kb%d-S%d' % s)
def test_overlap_table_is_exact(shape):
    B, ka, kb, S = shape
    g = torch.Generator().manual_seed(31 + S)
    a = torch.randint(0, ka, (B, S, S), generator=g, dtype=torch.uint8)
    b = torch.randint(0, kb, (B, S, S), generator=g, dtype=torch.uint8)
    got = objects.overlap_table(a.to(DEV), b.to(DEV), ka, kb)
    assert got.shape == (B, ka, kb) and got.dtype == torch.int32 and got.device.type == 'cuda'
    assert torch.equal(got.cpu().to(torch.int64), R.overlap_table(a, b, ka, kb))
    assert int(got.sum()) == B * S * S
    # labels beyond the table are left out, everything else stays exact
    a2 = torch.randint(0, 256, (B, S, S), generator=g, dtype=torch.uint8)
    b2 = torch.randint(0, kb + 3, (B, S, S), generator=g, dtype=torch.uint8)
    got2 = objects.overlap_table(a2.to(DEV), b2.to(DEV), ka, kb).cpu().to(torch.int64)
    assert torch.equal(got2, R.overlap_table(a2, b2, ka, kb))
    assert int(got2.sum()) == int(((a2 < ka) & (b2 < kb)).sum()) < B * S * S


def test_overlap_of_a_segmentation_with_itself_and_with_ari_tables():
    """ARI of a map with itself is 1; the per-slot pixel counts of seg are the column sums of ari_tables run with one all-ones
    ground-truth mask on the same soft masks."""
    B, K, S = 2, 7, 64
    md, cd, ref_t, ref_seg, table, seg = _case(B, K, S)
    ov = objects.overlap_table(seg, seg, K, K).cpu().numpy()
    iou = objects.slot_iou(ov)
    for b in range(B):
        assert compute_ari(ov[b]) == 1.0
        assert np.array_equal(ov[b], np.diag(np.diag(ov[b])))
        assert torch.equal(torch.diagonal(iou[b]), torch.tensor(np.diag(ov[b]) > 0, dtype=torch.float64))
    counts = ari_tables(md, [np.ones((1, S, S), dtype=np.uint8)] * B)[:, 0]                  # (B, K)
    assert np.array_equal(counts, np.stack([np.bincount(seg[b].cpu().numpy().ravel(), minlength=K) for b in range(B)]))
    assert np.array_equal(counts, table[..., 1].cpu().numpy().astype(np.int64))
    assert np.array_equal(counts, np.diagonal(ov, axis1=1, axis2=2))


# ---- the module: reconstruct(objects=True) -----------------------------------------------------
@pytest.fixture(scope='module')
def tiny():
    g = load_golden('tiny')
    arch, params, x, eps, _ = golden_setup(g)
    assert x.shape[0] >= 2
    return arch, make_hip_model(arch, params), x[:2].to(DEV), eps[:, :2].contiguous().to(DEV)


def _kl_per_slot(m):
    pm, plv = m.posterior.mean.double(), m.posterior.logvar.double()
    return 0.5 * (plv.exp() + pm * pm - 1.0 - plv).sum(-1)


def test_reconstruct_objects(tiny):
    arch, m, x, eps = tiny
    K, S = arch.slots, arch.img_size
    plain = m.reconstruct(x, eps)
    assert m.objects is None
    outs = m.reconstruct(x, eps, objects=True)
    for a, b in zip(plain, outs):
        assert torch.equal(a, b)
    ob = m.objects
    assert set(ob) == {'table', 'segmentation', 'kl'}
    assert ob['table'].shape == (2, K, 14) and ob['segmentation'].shape == (2, S, S) and ob['segmentation'].dtype == torch.uint8
    t, seg = objects.slot_table(outs[1], outs[2], segmentation=True)
    assert torch.equal(ob['table'].view(torch.int32), t.view(torch.int32)) and torch.equal(ob['segmentation'], seg)
    _check_table(ob['table'], R.slot_table(outs[1].cpu(), outs[2].cpu())[0], 'module')
    # per-slot KL of lambda_T against N(0, 1), and its total against torch.distributions
    kl = _kl_per_slot(m)
    assert ob['kl'].shape == (2, K) and ob['kl'].dtype == torch.float32
    assert float(((ob['kl'].double() - kl).abs() / kl.abs()).max()) <= 2.0 ** -24         # formed in double, rounded once to fp32
    post = torch.distributions.Normal(m.posterior.mean.double(), (0.5 * m.posterior.logvar.double()).exp())
    prior = torch.distributions.Normal(torch.zeros_like(post.loc), torch.ones_like(post.scale))
    total = torch.distributions.kl_divergence(post, prior).sum((1, 2)).mean()
    assert abs(float(ob['kl'].double().sum(1).mean()) - float(total)) <= 1e-6 * abs(float(total))
    m.reconstruct(x, eps)
    assert m.objects is None
    m.reconstruct(x, eps, objects=True)
    m.encode(x, eps)
    assert m.objects is None


def test_reconstruct_objects_with_trajectory(tiny):
    arch, m, x, eps = tiny
    K, S, T = arch.slots, arch.img_size, arch.iters
    pred, mask, mean = m.reconstruct(x, eps, trajectory=True, objects=True)
    tr, ob = m.trajectory, m.objects
    assert tr['table'].shape == (T + 1, 2, K, 14) and tr['segmentation'].shape == (T + 1, 2, S, S)
    assert tr['segmentation'].dtype == torch.uint8
    assert torch.equal(tr['table'][T].view(torch.int32), ob['table'].view(torch.int32))
    assert torch.equal(tr['segmentation'][T], ob['segmentation'])
    t0, s0 = objects.slot_table(tr['mask'][0], tr['mean'][0], segmentation=True)
    assert torch.equal(tr['table'][0].view(torch.int32), t0.view(torch.int32)) and torch.equal(tr['segmentation'][0], s0)
    tT = objects.slot_table(mask, mean)
    assert torch.equal(ob['table'].view(torch.int32), tT.view(torch.int32))
    m.reconstruct(x, eps, trajectory=True)
    assert m.objects is None and 'table' not in m.trajectory


def test_reconstruct_objects_chunked(tiny):
    """batch_cap 1 runs the two images as two library calls; the tables are read from the joined tensors afterwards"""
    arch, m, x, eps = tiny
    m.set_option('batch_cap', 1)
    try:
        pred, mask, mean = m.reconstruct(x, eps, objects=True)
        ob = m.objects
    finally:
        m.set_option('batch_cap', 0)
    assert ob['table'].shape[0] == 2 and ob['kl'].shape[0] == 2
    for i in range(2):
        ti, si = objects.slot_table(mask[i:i + 1], mean[i:i + 1], segmentation=True)
        assert torch.equal(ob['table'][i:i + 1].view(torch.int32), ti.view(torch.int32)) and torch.equal(ob['segmentation'][i:i + 1], si)
        m.reconstruct(x[i:i + 1], eps[:, i:i + 1].contiguous(), objects=True)
        assert torch.equal(m.objects['table'].view(torch.int32), ob['table'][i:i + 1].view(torch.int32))
        assert torch.equal(m.objects['segmentation'], ob['segmentation'][i:i + 1])
        assert torch.equal(m.objects['kl'], ob['kl'][i:i + 1])
